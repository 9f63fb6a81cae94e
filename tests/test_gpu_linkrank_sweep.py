"""Full-candidate filtered link ranking (A15) past one destination tile per workgroup.

tests/test_gpu_linkrank.py keeps ``k_rank_sweep`` at one tile per workgroup (few query blocks, few tiles: every split
is one tile).  Here a workgroup walks several tiles — the per-tile accumulator reset, the counters carried in
registers across tiles, the prefetch of the next tile's first K stage under the last stage of the current one, the
shorter last split — up to the regime of tools/bench_linkrank.py (512 query blocks or more: one split, every tile in
one workgroup).  Counts are exact against the float64 reference on integer-valued embeddings; the reference is
evaluated a few thousand queries at a time (tests/test_linkrank_host.py::ref_full_ranks_chunked).

Every test reads ``splits=`` from the sweep's launch tag and recomputes the launch arithmetic of
``hgin_link_full_rank_f32`` (128-query blocks, 128-destination tiles, 512 target workgroups), so a retuning that
moves a shape out of its regime fails here instead of silently testing less."""
import numpy as np
import pytest
import torch

from test_gpu_linkrank import DEV, N_SRC, _int_inputs, _run, _superset
from test_linkrank_host import ref_full_bands, ref_full_ranks_chunked

pytestmark = pytest.mark.gpu

TILE, TARGET_BLOCKS = 128, 512


def _cdiv(a, b):
    return -(-a // b)


def _plan(E, n_dst):
    """(query blocks, tiles, tiles per split, splits) as hgin_link_full_rank_f32 launches them."""
    n_qblocks, n_tiles = _cdiv(E, TILE), _cdiv(n_dst, TILE)
    splits0 = min(_cdiv(TARGET_BLOCKS, n_qblocks), n_tiles)
    tiles_per_split = _cdiv(n_tiles, splits0)
    return n_qblocks, n_tiles, tiles_per_split, _cdiv(n_tiles, tiles_per_split)


def _traced_run(zs, zd, pos, known, vec):
    """The three counts, with the sweep's launch tag checked: returns (counts, splits the library launched)."""
    from hgin import _lib
    with _lib.trace_launches() as tr:
        got = _run(zs, zd, pos, known)
    tags = [t for t in tr.kernels if t.startswith("k_rank_sweep")]
    assert len(tags) == 1 and tags[0].startswith(f"k_rank_sweep<{vec}> splits="), tr.kernels
    return got, int(tags[0].split("splits=")[1])


def _assert_regime(E, n_dst, splits_launched, tiles_per_split, splits):
    plan = _plan(E, n_dst)
    assert splits_launched == plan[3], ("the library's split count left the formula", splits_launched, plan)
    assert plan[2] == tiles_per_split >= 2 and plan[3] == splits, plan
    return plan


def _assert_exact(got, zs, zd, pos, known, tag):
    want = ref_full_ranks_chunked(zs.numpy(), zd.numpy(), pos.numpy(), None if known is None else known.numpy())
    for name, a, b in zip(("n_greater", "n_equal", "n_cand"), got, want):
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, (tag, name, bad.size, bad[:5].tolist(), a[bad[:5]].tolist(), b[bad[:5]].tolist())
    return want


def _sliced(zs_w, zd_w, offset, F):
    """Device column windows [offset, offset + F) of wider tensors (row stride > F) and their contiguous host copies."""
    zs_d, zd_d = zs_w.to(DEV)[:, offset:offset + F], zd_w.to(DEV)[:, offset:offset + F]
    assert zs_d.stride(0) == zs_w.size(1) and not zs_d.is_contiguous() and not zd_d.is_contiguous()
    return zs_d, zd_d, zs_w[:, offset:offset + F].contiguous(), zd_w[:, offset:offset + F].contiguous()


# (E, n_dst, tiles_per_split, splits, query blocks, tiles, rows of the last tile, tiles of the last split)
SHAPES = {
    "3qb_401tiles": (300, 51209, 3, 134, 3, 401, 9, 2),
    "100qb_11tiles": (12700, 1283, 2, 6, 100, 11, 3, 1),
    "512qb_one_split": (65500, 300, 3, 1, 512, 3, 44, 3),
}
# F = 8: one K stage, every prefetch crosses a tile boundary; 64: two stages; 100 read through a column window at an
# odd offset: scalar loads, four stages, the last one ragged.  Every regime meets F = 8 and a multi-stage width.
CASES = [("3qb_401tiles", 8, False), ("3qb_401tiles", 64, False), ("3qb_401tiles", 100, True),
         ("100qb_11tiles", 8, False), ("100qb_11tiles", 100, True),
         ("512qb_one_split", 8, False), ("512qb_one_split", 64, False)]


@pytest.mark.parametrize("kind", ["none", "superset"])
@pytest.mark.parametrize("shape,F,sliced", CASES)
def test_exact_with_several_tiles_per_workgroup(shape, F, sliced, kind):
    E, n_dst, tps, splits, n_qb, n_tiles, last_rows, last_split_tiles = SHAPES[shape]
    assert (n_qb, n_tiles) == (_cdiv(E, TILE), _cdiv(n_dst, TILE)) and n_dst - (n_tiles - 1) * TILE == last_rows
    assert n_tiles - (splits - 1) * tps == last_split_tiles
    if sliced:
        pos, zs_w, zd_w, g = _int_inputs(E, n_dst, F + 12, seed=4000 + F + E)
        zs_d, zd_d, zs, zd = _sliced(zs_w, zd_w, 3, F)
    else:
        pos, zs, zd, g = _int_inputs(E, n_dst, F, seed=4000 + F + E)
        zs_d, zd_d = zs, zd
    known = None if kind == "none" else _superset(pos, N_SRC, n_dst, g)
    got, launched = _traced_run(zs_d, zd_d, pos, known, 1 if sliced else 4)
    _assert_regime(E, n_dst, launched, tps, splits)
    want = _assert_exact(got, zs, zd, pos, known, (shape, F, kind))
    assert int(want[1].sum()) > 0 and int(want[0].min()) < int(want[0].max())   # ties and a spread of ranks
    if known is not None:
        assert int((want[2] < n_dst - 1).sum()) > E // 2   # the filter removed something for most queries


COPIES = [5, 130, 260, 390, 515, 777, 1000, 1199]   # eight different 128-destination tiles


@pytest.mark.parametrize("integer", [True, False])
def test_copies_of_the_positive_row_are_ties_across_the_tiles_of_one_workgroup(integer):
    """Eight rows of z_dst in eight tiles are copies of query 0's destination row, and one workgroup scores all ten
    tiles (512 query blocks: one split): all eight land in n_equal, none in n_greater.  In
    tests/test_gpu_linkrank.py's version of this test each copy is scored by another workgroup."""
    E, n_dst, F = 65500, 1200, 64
    pos, zs, zd, g = _int_inputs(E, n_dst, F, seed=12)
    if not integer:
        zs, zd = torch.randn(N_SRC, F, generator=g) * 0.5, torch.randn(n_dst, F, generator=g) * 0.5
    pos[1, 0] = 600
    pos[:, 40000] = pos[:, 0]   # the same query again, in query block 312
    zd[COPIES] = zd[600].clone()
    got, launched = _traced_run(zs, zd, pos, None, 4)
    plan = _plan(E, n_dst)
    assert launched == plan[3] == 1 and plan[2] == plan[1] == 10   # one split: the workgroup walks all ten tiles
    if integer:
        _assert_exact(got, zs, zd, pos, None, "copies")
        assert got[1][0] >= 8
    else:
        assert got[1][0] == 8
        lo, hi, _, _, _ = ref_full_bands(zs.numpy(), zd.numpy(), pos[:, :1].numpy(), None)
        assert lo[0] <= got[0][0] <= hi[0] - 8   # the copies are inside the band and must not count as greater
    assert all(x[40000] == x[0] for x in got)   # another query block, the same counts


def test_repeatable_and_equal_for_a_query_repeated_in_another_query_block():
    """Random floats, three tiles per workgroup, filtered: two runs are bitwise equal, queries repeated in another
    128-query block get equal counts, and the counts lie in the float64 rounding bands."""
    E, n_dst, F = 300, 51209, 64
    g = torch.Generator().manual_seed(98)
    p0 = torch.stack([torch.randint(0, N_SRC, (200,), generator=g), torch.randint(0, n_dst, (200,), generator=g)])
    pos = torch.cat([p0, p0[:, 3:4], p0[:, :99]], 1)   # query 200 = query 3; queries 201.. = queries 0..98
    assert pos.size(1) == E
    zs, zd = torch.randn(N_SRC, F, generator=g) * 0.5, torch.randn(n_dst, F, generator=g) * 0.5
    known = _superset(pos, N_SRC, n_dst, g)
    a, launched = _traced_run(zs, zd, pos, known, 4)
    _assert_regime(E, n_dst, launched, 3, 134)
    b = _run(zs, zd, pos, known)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    for x in a:
        assert x[3] == x[200] and np.array_equal(x[:99], x[201:300])   # block 0 against blocks 1 and 2
    lo, hi, ge_lo, ge_hi, nc = ref_full_bands(zs.numpy(), zd.numpy(), pos.numpy(), known.numpy())
    gt, eq, cand = a
    assert np.array_equal(cand, nc)
    assert bool(((lo <= gt) & (gt <= hi)).all()), np.nonzero((gt < lo) | (gt > hi))[0][:5].tolist()
    assert bool(((ge_lo <= gt + eq) & (gt + eq <= ge_hi)).all())
    assert int(gt.max()) > 3 * TILE   # more above the positive than the three tiles of one split hold


@pytest.mark.parametrize("F,sliced", [(8, False), (100, True)])
def test_hub_sources_in_the_filter(F, sliced):
    """The filter's ``__any(t < deg)`` loop with most lanes idle: in the first 32-query wave two queries come from
    hub sources (about 600 distinct known destinations each, 200 of them listed twice, the query's own destination
    among them) and thirty from sources without a known edge; in the second wave one query's source is connected to
    every destination (no candidate left at n_dst > 128) and the rest have none; the third wave mixes ordinary
    sources with the hubs again."""
    E, n_dst, n_src = 96, 700, N_SRC
    width = F + 12 if sliced else F
    pos, zs_w, zd_w, g = _int_inputs(E, n_dst, width, seed=77 + F, n_src=n_src)
    hub_a, hub_b, hub_all = 290, 291, 292
    pos[0, :64] = torch.arange(200, 264)           # sources 200..263: no known edge at all
    pos[0, 5], pos[0, 17], pos[0, 40] = hub_a, hub_b, hub_all
    pos[0, 64:] = torch.randint(0, 100, (32,), generator=g)
    pos[0, 70], pos[0, 71], pos[0, 90] = hub_a, hub_all, hub_b
    parts = []
    for hub, q in ((hub_a, 5), (hub_b, 17)):
        perm = torch.randperm(n_dst, generator=g)
        # 599 distinct destinations and the query's own, which is a known edge too; 200 entries listed twice
        dsts = torch.cat([pos[1, q:q + 1], perm[perm != pos[1, q]][:599]])
        dsts = torch.cat([dsts, dsts[100:300]])
        parts.append(torch.stack([torch.full_like(dsts, hub), dsts]))
    parts.append(torch.stack([torch.full((n_dst,), hub_all), torch.arange(n_dst)]))
    parts.append(torch.stack([torch.randint(0, 100, (400,), generator=g), torch.randint(0, n_dst, (400,), generator=g)]))
    parts.append(pos[:, 64:])
    known = torch.cat(parts, 1)[:, torch.randperm(sum(p.size(1) for p in parts), generator=g)]
    deg = torch.bincount(known[0], minlength=n_src)
    assert int(deg[200:264].sum()) == 0 and int(deg[hub_a]) >= 800 and int(deg[hub_all]) >= n_dst
    if sliced:
        zs_d, zd_d, zs, zd = _sliced(zs_w, zd_w, 3, F)
    else:
        zs_d, zd_d, zs, zd = zs_w, zd_w, zs_w, zd_w
    got, _ = _traced_run(zs_d, zd_d, pos, known, 1 if sliced else 4)
    want = _assert_exact(got, zs, zd, pos, known, ("hubs", F))
    gt, eq, nc = got
    assert nc[40] == nc[71] == 0 and gt[40] == eq[40] == gt[71] == eq[71] == 0
    assert nc[5] == nc[17] == 100   # 700 - 1 - the 599 known destinations other than the query's own
    assert nc[70] in (99, 100) and nc[90] in (99, 100)   # the same hubs queried for another destination
    idle = [q for q in range(64) if q not in (5, 17, 40)]
    assert bool((nc[idle] == n_dst - 1).all())
    assert int(want[0][idle].max()) > 0 and int(want[1].sum()) > 0
