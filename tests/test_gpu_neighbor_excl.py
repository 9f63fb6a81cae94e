"""Neighbour sampling with an excluded set (include/hgin.h A25) on the device: the two kernels and the subgraph against
the numpy restatement of tests/test_neighbor_excl_host.py bit for bit, the equivalence with a graph the pairs were
removed from, and the link layer's ``exclude_targets``."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from test_gpu_neighbor import SEEDS, _assert_sub, _dev_seeds, _graphs, _model
from test_neighbor_excl_host import pair_set, ref_picks_excl, ref_sample_excl
from test_neighbor_host import ref_csr, ref_sample

DEV = "cuda"
pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789
FANOUTS = [1, 5, 8, 9, 32, 33, 128, -1]       # both sides of each lane-group width (8 / 16 / 64 lanes)
FRONTIERS = [1, 65, 257, 1100]
N_SRC, N_DST = 500, 1200
N_MODES = 9


# ---------------------------------------------------------------------------------------------------
# one hop, one relation: the kernels themselves
# ---------------------------------------------------------------------------------------------------
def _drop_to(srcs, target):
    """Distinct sources of a row whose removal (every copy) leaves exactly ``target`` positions, or as close above it as
    the multiplicities allow."""
    left, gone = len(srcs), []
    mult = {}
    for s in srcs:
        mult[s] = mult.get(s, 0) + 1
    for s, m in mult.items():
        if left - m >= target:
            gone.append(s)
            left -= m
        if left == target:
            break
    return gone


@functools.lru_cache(maxsize=None)
def _rows(f):
    """Destination rows whose degrees cycle through 0, 1, f - 1, f, f + 1, f + 3, 300 (f = 5 for the all-neighbours
    case) in shuffled edge order; with 500 sources the rows of 300 hold repeated pairs.  Row v's exclusions are chosen by
    (v // 7) % 9: none; the first position; the last; one repeated pair; down to d' = f; to d' = f + 1; half the row
    (150 of 300); the whole row; keys that name no edge of the row.  The rows outside a frontier supply the keys of
    non-frontier rows.  (edge_index cpu, (rowptr, col, perm) numpy, the excluded {(src, dst)}); no device is used."""
    fe = 5 if f == -1 else f
    degs = [0, 1, max(fe - 1, 0), fe, fe + 1, fe + 3, 300]
    g = torch.Generator().manual_seed(100 + fe)
    dst = torch.cat([torch.full((degs[v % 7],), v, dtype=torch.long) for v in range(N_DST)])
    src = torch.randint(0, N_SRC, (dst.numel(),), generator=g)
    order = torch.randperm(dst.numel(), generator=g)
    ei = torch.stack([src[order], dst[order]])
    ref = ref_csr(ei, N_DST)
    rowptr, col, _ = ref
    pairs, left = set(), {}
    for v in range(N_DST):
        row = col[rowptr[v]:rowptr[v + 1]].tolist()
        mode = (v // 7) % N_MODES
        gone = []
        if mode == 8:
            gone = [u for u in range(N_SRC) if u not in set(row)][:3]
        elif row:
            if mode == 1:
                gone = [row[0]]
            elif mode == 2:
                gone = [row[-1]]
            elif mode == 3:
                gone = [s for s in row if row.count(s) > 1][:1] or [row[len(row) // 2]]
            elif mode == 4:
                gone = _drop_to(row, fe)
            elif mode == 5:
                gone = _drop_to(row, fe + 1)
            elif mode == 6:
                gone = _drop_to(row, len(row) // 2)
            elif mode == 7:
                gone = sorted(set(row))
        pairs |= {(u, v) for u in gone}
        if v % 7 == 6:
            left.setdefault(mode, set()).add(sum(u not in gone for u in row))
    # the rows of 300: untouched, one position gone, a repeated pair gone, d' = f, f + 1, 150, 0
    few = left[1] | left[2] | left[3]
    assert left[0] == {300} and 290 <= min(few) and max(few) == 299 and max(left[3]) <= 298, left
    assert left[4] == {fe} and left[5] == {fe + 1} and left[6] == {150} and left[7] == {0} and left[8] == {300}, left
    return ei, ref, pairs


@functools.lru_cache(maxsize=None)
def _bipartite(f):
    """``_rows(f)`` on the device: (edge_index cpu, (rowptr, col, perm) numpy, the device Csr, the excluded {(src, dst)},
    the ascending device keys dst * 2^32 + src, some of them repeated)."""
    from hgin import ops
    ei, ref, pairs = _rows(f)
    csr = ops.build_csr(ei.to(DEV), 1, N_DST, N_SRC)
    assert np.array_equal(csr.rowptr.cpu().numpy(), ref[0]) and np.array_equal(csr.col.cpu().numpy(), ref[1])
    assert np.array_equal(csr.perm.cpu().numpy(), ref[2])
    keys = sorted((v << 32) | u for u, v in pairs)
    keys = sorted(keys + keys[::5])                    # repeats are allowed
    return ei, ref, csr, pairs, torch.tensor(keys, dtype=torch.int64, device=DEV)


def _one_hop(csr, frontier, f, seed, offset, slot, excl):
    """(off, src, eid) as numpy: excl = None through the A22 entry points, else through A25's with these keys."""
    from hgin import _lib, ops
    n = int(frontier.numel())
    off = torch.full((n + 1,), -7, dtype=torch.int64, device=DEV)
    size = ctypes.c_size_t(0)
    _lib.call("hgin_neighbor_sample_workspace_size", n, ctypes.byref(size))
    ws = torch.empty(size.value, dtype=torch.uint8, device=DEV)
    st = ops._stream(off)
    xp = None if excl is None or excl.numel() == 0 else ops._p(excl)
    nx = 0 if excl is None else int(excl.numel())
    if excl is None:
        _lib.call("hgin_neighbor_sample_offsets", ops._p(csr.rowptr), csr.n_rows, ops._p(frontier), n, f, ops._p(off),
                  ops._p(ws), size.value, st)
    else:
        _lib.call("hgin_neighbor_sample_offsets_excl", ops._p(csr.rowptr), ops._p(csr.col), csr.n_rows,
                  ops._p(frontier), n, f, xp, nx, ops._p(off), ops._p(ws), size.value, st)
    tot = int(off[-1])
    src = torch.full((tot,), -7, dtype=torch.int64, device=DEV)
    eid = torch.full((tot,), -7, dtype=torch.int64, device=DEV)
    if excl is None:
        _lib.call("hgin_neighbor_sample", ops._p(csr.rowptr), ops._p(csr.col), ops._p(csr.perm), csr.n_rows,
                  ops._p(frontier), n, f, seed, offset, slot, ops._p(off), ops._p(src), ops._p(eid), tot, st)
    else:
        _lib.call("hgin_neighbor_sample_excl", ops._p(csr.rowptr), ops._p(csr.col), ops._p(csr.perm), csr.n_rows,
                  ops._p(frontier), n, f, seed, offset, slot, xp, nx, ops._p(off), ops._p(src), ops._p(eid), tot, st)
    return off.cpu().numpy(), src.cpu().numpy(), eid.cpu().numpy()


def _ref_one_hop(ref, frontier, f, seed, offset, slot, excl_set):
    rowptr, col, perm = ref
    off, src, eid = [0], [], []
    for v in frontier:
        v = int(v)
        if 0 <= v < len(rowptr) - 1:
            for p in ref_picks_excl(rowptr, col, v, f, seed, offset, slot, excl_set):
                src.append(int(col[rowptr[v] + p]))
                eid.append(int(perm[rowptr[v] + p]))
        off.append(len(src))
    return np.asarray(off), np.asarray(src, dtype=np.int64), np.asarray(eid, dtype=np.int64)


def _frontier(f, n):
    g = torch.Generator().manual_seed(7 * n + (f & 0xFF))
    if n == 1:
        return torch.tensor([48])                 # a row of 300 cut to 150
    frontier = torch.randperm(N_DST, generator=g)[:n]
    if n == 257:                                   # ids outside [0, n_rows) count as empty rows
        frontier[100], frontier[200] = N_DST + 3, -1
    return frontier


@pytest.mark.parametrize("n", FRONTIERS)
@pytest.mark.parametrize("f", FANOUTS)
def test_one_hop_matches_the_restatement(f, n):
    ei, ref, csr, excl_set, excl = _bipartite(f)
    frontier = _frontier(f, n)
    for offset, slot in ((0, 0), (2**32 - 1, 3)):
        got = _one_hop(csr, frontier.to(DEV), f, SEED, offset, slot, excl)
        want = _ref_one_hop(ref, frontier.numpy(), f, SEED, offset, slot, excl_set)
        for a, b, what in zip(got, want, ("off", "src", "eid")):
            assert np.array_equal(a, b), (what, f, n, offset)
    # no emitted edge is an excluded pair
    rowptr, col, perm = ref
    e = ei.numpy()[:, got[2]]
    assert not (set(zip(e[0].tolist(), e[1].tolist())) & excl_set)
    assert np.array_equal(e[0], got[1])
    if n >= 65:
        plain = _ref_one_hop(ref, frontier.numpy(), f, SEED, offset, slot, set())
        assert not np.array_equal(plain[0], want[0])          # the exclusion had work to do


@pytest.mark.parametrize("f", FANOUTS)
def test_no_keys_is_a22_bit_for_bit(f):
    _, _, csr, _, excl = _bipartite(f)
    frontier = _frontier(f, 257).to(DEV)
    a22 = _one_hop(csr, frontier, f, SEED, 3, 2, None)
    none = _one_hop(csr, frontier, f, SEED, 3, 2, torch.empty(0, dtype=torch.int64, device=DEV))     # excl = NULL
    for a, b in zip(a22, none):
        assert np.array_equal(a, b)
    # keys that only name rows outside the frontier, or nothing at all, change nothing either
    far = torch.tensor(sorted([((N_DST + 5) << 32) | 1, (2**31 - 1) << 32, 5]), dtype=torch.int64, device=DEV)
    for a, b in zip(a22, _one_hop(csr, frontier, f, SEED, 3, 2, far)):
        assert np.array_equal(a, b)


def test_empty_frontier_and_a_relation_without_edges():
    from hgin import ops
    _, _, csr, _, excl = _bipartite(5)
    off, src, eid = _one_hop(csr, torch.empty(0, dtype=torch.int64, device=DEV), 5, SEED, 0, 0, excl)
    assert off.tolist() == [0] and src.size == 0 and eid.size == 0
    none = ops.build_csr(torch.empty((2, 0), dtype=torch.int64, device=DEV), 1, N_DST, N_SRC)
    frontier = torch.arange(0, 300, dtype=torch.int64, device=DEV)
    for f in (3, -1):
        off, src, eid = _one_hop(none, frontier, f, SEED, 0, 0, excl)
        assert off.tolist() == [0] * 301 and src.size == 0


# ---------------------------------------------------------------------------------------------------
# the subgraph
# ---------------------------------------------------------------------------------------------------
FANS = [[3], [3, 2], [-1, 2], [128, 1, 5]]


@functools.lru_cache(maxsize=None)
def _exclusion():
    """Pairs of three relations of ``_graphs()``: every third path -> link edge (the hub link 0's among them) and their
    flips in link -> path, every fourth node -> link edge.  ({relation: cpu int64 [2, M]}, {relation: {(src, dst)}})."""
    from hgin.data import REL_LP, REL_NL, REL_PL
    cpu, _ = _graphs()
    pl = cpu.edge_index[REL_PL][:, ::3].contiguous()
    ex = {REL_PL: pl, REL_LP: pl.flip(0).contiguous(), REL_NL: cpu.edge_index[REL_NL][:, ::4].contiguous()}
    return ex, {r: pair_set(e) for r, e in ex.items()}


def _dev_excl(ex):
    return {r: e.to(DEV) for r, e in ex.items()}


def _no_excluded_edge(sub, sets):
    for r, s in sets.items():
        e = sub.graph.edge_index[r]
        back = torch.stack([sub.n_id[r[0]][e[0]], sub.n_id[r[2]][e[1]]])
        assert not (pair_set(back) & s), r


@pytest.mark.parametrize("fanouts", FANS, ids=lambda f: "-".join(map(str, f)))
@pytest.mark.parametrize("case", list(SEEDS))
def test_subgraph_matches_the_restatement(case, fanouts):
    import hgin
    cpu, dev = _graphs()
    rels = list(cpu.edge_index.keys())
    ex, sets = _exclusion()
    sampler = hgin.NeighborSampler(dev, fanouts=fanouts, seed=SEED)
    for offset in (0, 5):
        sub = sampler.sample_excluding(_dev_seeds(SEEDS[case]), _dev_excl(ex), offset=offset)
        ref = ref_sample_excl(cpu, rels, fanouts, SEEDS[case], SEED, offset, sets)
        _assert_sub(sub, ref, cpu, rels)
        _no_excluded_edge(sub, sets)
    plain = ref_sample(cpu, rels, fanouts, SEEDS[case], SEED, offset)
    if len(fanouts) > 1:      # (one hop of three around a few seeds can miss every excluded pair)
        assert any(not np.array_equal(plain[2][r], ref[2][r]) for r in rels)
    for m in sampler._maps.values():
        assert bool((m == -1).all())


def test_the_cases_the_exclusion_is_about_occur():
    """On the reference: the hub row (link 0, a hop-1 row of the first seed case) loses positions and is still cut to
    the fanout, other hop-1 rows lose positions, and so does a row that is only expanded at hop 2."""
    from hgin.data import REL_LP, REL_PL
    cpu, _ = _graphs()
    rels = list(cpu.edge_index.keys())
    _, sets = _exclusion()
    seeds = SEEDS["two types with repeats"]
    rowptr, col, _ = ref_csr(cpu.edge_index[REL_PL], int(cpu.x["link"].shape[0]))
    hub = col[rowptr[0]:rowptr[1]].tolist()
    gone = sum((u, 0) in sets[REL_PL] for u in hub)
    assert 50 < gone < len(hub) - 50
    n_id, edges, e_id, n_seed = ref_sample_excl(cpu, rels, [3, 2], seeds, SEED, 0, sets)
    assert (edges[REL_PL][1] == 0).sum() == 3
    for r in (REL_PL, REL_LP):
        rp, c, _ = ref_csr(cpu.edge_index[r], int(cpu.x[r[2]].shape[0]))
        hit = [v for v in n_id[r[2]].tolist() if any((int(u), v) in sets[r] for u in c[rp[v]:rp[v + 1]])]
        local = {v: i for i, v in enumerate(n_id[r[2]].tolist())}
        assert any(local[v] < n_seed[r[2]] for v in hit), r                         # a hop-1 row
        expanded = set(edges[r][1].tolist())
        assert any(local[v] >= n_seed[r[2]] and local[v] in expanded for v in hit), r   # a row expanded at hop 2


def test_an_empty_exclusion_is_sample_tensor_for_tensor():
    import hgin
    from hgin.data import REL_LP, REL_PL
    cpu, dev = _graphs()
    rels = list(cpu.edge_index.keys())
    sampler = hgin.NeighborSampler(dev, fanouts=[3, 2], seed=SEED)
    seeds = _dev_seeds(SEEDS["two types with repeats"])
    none = torch.empty((2, 0), dtype=torch.int64, device=DEV)
    for o in (0, 4):
        want = sampler.sample(seeds, o)
        for exclude in ({}, {REL_PL: none}, {REL_PL: none, REL_LP: none}):
            got = sampler.sample_excluding(seeds, exclude, o)
            assert got.n_seed == want.n_seed
            for t in want.n_id:
                assert torch.equal(got.n_id[t], want.n_id[t]) and torch.equal(got.graph.x[t], want.graph.x[t])
                assert torch.equal(got.graph.batch[t], want.graph.batch[t])
            assert torch.equal(got.graph.y, want.graph.y)
            for r in rels:
                assert torch.equal(got.graph.edge_index[r], want.graph.edge_index[r])
                assert torch.equal(got.e_id[r], want.e_id[r])


def test_state_is_clean_after_a_call_and_after_an_error():
    import hgin
    from hgin.data import REL_PL
    cpu, dev = _graphs()
    rels = list(cpu.edge_index.keys())
    ex, sets = _exclusion()
    seeds = SEEDS["two types with repeats"]
    one = hgin.NeighborSampler(dev, fanouts=[3, 2], seed=1)
    one.sample_excluding(_dev_seeds(seeds), _dev_excl(ex), 0)
    for m in one._maps.values():
        assert bool((m == -1).all())
    with pytest.raises(IndexError, match="excluded"):
        one.sample_excluding(_dev_seeds(seeds), {REL_PL: torch.tensor([[0, 180], [1, 2]], device=DEV)}, 2)
    with pytest.raises(IndexError, match="seed"):
        one.sample_excluding({"path": torch.tensor([0, 180], device=DEV)}, _dev_excl(ex), 2)
    with pytest.raises(ValueError, match="several devices"):
        one.sample_excluding(_dev_seeds(seeds), {REL_PL: ex[REL_PL]}, 2)             # pairs left on the host
    for m in one._maps.values():
        assert bool((m == -1).all())
    _assert_sub(one.sample_excluding(_dev_seeds(seeds), _dev_excl(ex), 0),
                ref_sample_excl(cpu, rels, [3, 2], seeds, 1, 0, sets), cpu, rels)
    _assert_sub(one.sample(_dev_seeds(seeds), 0), ref_sample(cpu, rels, [3, 2], seeds, 1, 0), cpu, rels)


# ---------------------------------------------------------------------------------------------------
# the point of it: the batch's own edges carry no message
# ---------------------------------------------------------------------------------------------------
def _reduced(dev, pos):
    """``dev`` without the edges of the pairs ``pos`` in path -> link and of their flips in link -> path: an
    order-preserving boolean mask over each relation."""
    from hgin.data import REL_LP, REL_PL, HeteroGraph
    n_link = int(dev.x["link"].size(0))
    keys = torch.unique(pos[0] * n_link + pos[1])
    ei = dict(dev.edge_index)
    pl, lp = dev.edge_index[REL_PL], dev.edge_index[REL_LP]
    ei[REL_PL] = pl[:, ~torch.isin(pl[0] * n_link + pl[1], keys)].contiguous()
    ei[REL_LP] = lp[:, ~torch.isin(lp[1] * n_link + lp[0], keys)].contiguous()
    assert ei[REL_PL].size(1) < pl.size(1) and ei[REL_LP].size(1) == ei[REL_PL].size(1)
    return HeteroGraph(dev.x, ei, dev.y, dev.batch)


def _positives(dev, which):
    from hgin.data import REL_PL
    pl = dev.edge_index[REL_PL]
    return pl if which == "all" else pl[:, 1::2].contiguous()


def test_encode_of_the_batch_without_its_targets_matches_the_graph_without_them():
    """fanouts = [-1] * layers: the seeds' embeddings on ``link_neighbor_batch_excl``'s subgraph are those of the graph
    the batch's pairs were removed from (in both relations), not those of the graph that still holds them."""
    import hgin
    from hgin.data import REL_LP, REL_PL
    _, dev = _graphs()
    model, layers = _model()
    pos = dev.edge_index[REL_PL][:, 40:200].contiguous()
    assert bool((pos[1] == 0).any())                       # the hub link is a destination of the batch
    sampler = hgin.NeighborSampler(dev, fanouts=[-1] * layers, seed=0)
    batch = hgin.link_neighbor_batch_excl(sampler, REL_PL, pos, None, offset=0)
    sub = batch.sub
    assert torch.equal(sub.n_id["path"][batch.pos[0]], pos[0]) and torch.equal(sub.n_id["link"][batch.pos[1]], pos[1])
    red = _reduced(dev, pos)
    with torch.no_grad():
        z_red = model.encode(red.x_dict(), red.edge_index_dict())
        z_full = model.encode(dev.x_dict(), dev.edge_index_dict())
        z_sub = model.encode(sub.graph.x_dict(), sub.graph.edge_index_dict())
    for t in ("path", "link"):
        n = sub.n_seed[t]
        assert n > 0
        want, got = z_red[t][sub.n_id[t][:n]].double(), z_sub[t][:n].double()
        d, nz = float((got - want).norm()), float(want.norm())
        leak = float((got - z_full[t][sub.n_id[t][:n]].double()).norm())
        print(f"{t}: {n} seed rows, ||dz|| / ||z|| = {d / nz:.3g}, bit-equal: {torch.equal(got, want)}; "
              f"against the unreduced graph {leak / nz:.3g}")
        assert nz > 0 and d <= 1e-5 * nz + 1e-9, (t, d, nz)
        assert leak > 1e-3 * nz, (t, leak, nz)             # they differ from the embeddings that see the targets
    batch_pairs = pair_set(pos)
    _no_excluded_edge(sub, {REL_PL: batch_pairs, REL_LP: {(d, s) for s, d in batch_pairs}})
    # the plain batch does hold them
    plain = hgin.link_neighbor_batch(sampler, REL_PL, pos, None, offset=0).sub
    e = plain.graph.edge_index[REL_PL]
    assert pair_set(torch.stack([plain.n_id["path"][e[0]], plain.n_id["link"][e[1]]])) & batch_pairs


# ---------------------------------------------------------------------------------------------------
# the predictor
# ---------------------------------------------------------------------------------------------------
def _grads(model):
    return {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


def _assert_close(got, full, g_got, g_full, what):
    got, full = float(got.detach()), float(full.detach())
    dl = abs(got - full)
    print(f"{what}: loss {full:.6g}, |dloss| / |loss| = {dl / abs(full):.3g}")
    assert set(g_got) == set(g_full)
    for n, want in g_full.items():
        d, nz = float((g_got[n].double() - want.double()).norm()), float(want.double().norm())
        print(f"  {n}: ||dg|| / ||g|| = {d / max(nz, 1e-300):.3g} (||g|| = {nz:.3g})")
    assert dl <= 1e-5 * abs(full), (dl, full)
    for n, want in g_full.items():
        d, nz = float((g_got[n].double() - want.double()).norm()), float(want.double().norm())
        assert d <= 1e-5 * nz + 1e-9, (n, d, nz)


@pytest.mark.parametrize("which", ["all", "half"])
@pytest.mark.parametrize("objective", ["bce", "softmax"])
def test_batch_loss_without_targets_matches_the_loss_on_the_reduced_graph(objective, which):
    """All the positives in one batch at full fanout.  "all": every path -> link edge is a positive, so the reduced graph
    has none left in either relation; "half": every other edge, the rest still carries messages."""
    import hgin
    from hgin.data import REL_PL
    _, dev = _graphs()
    model, layers = _model()
    pos = _positives(dev, which)
    red = _reduced(dev, pos)
    step = 2
    pred = hgin.LinkPredictor(model, REL_PL, k=3, seed=11, objective=objective, exclude_targets=True)
    sampler = hgin.NeighborSampler(dev, fanouts=[-1] * layers, seed=5)
    model.zero_grad()
    full = pred.loss(red, pos=pos, step=step)
    full.backward()
    g_full = _grads(model)
    model.zero_grad()
    got = pred.batch_loss(sampler, pos, step=step)
    got.backward()
    _assert_close(got, full, _grads(model), g_full, f"{objective} / {which}")
    # and it is not the loss of the graph that still holds the targets
    with torch.no_grad():
        leaky = hgin.LinkPredictor(model, REL_PL, k=3, seed=11, objective=objective).batch_loss(sampler, pos, step=step)
    assert abs(float(leaky) - float(full.detach())) > 1e-4 * abs(float(full.detach()))


@pytest.mark.parametrize("which", ["all", "half"])
def test_batch_full_loss_without_targets_matches_the_reduced_graph(which):
    import hgin
    from hgin.data import REL_PL
    _, dev = _graphs()
    model, layers = _model()
    pos = _positives(dev, which)
    red = _reduced(dev, pos)
    pred = hgin.LinkPredictor(model, REL_PL, k=3, seed=11, temperature=0.7, exclude_targets=True)
    sampler = hgin.NeighborSampler(dev, fanouts=[-1] * layers, seed=5)
    # the batch's candidates are its destination seeds: the unique destinations of pos, ascending
    u = torch.unique(pos[1])
    local = torch.stack([pos[0], torch.searchsorted(u, pos[1].contiguous())])
    model.zero_grad()
    z = model.encode(red.x_dict(), red.edge_index_dict())
    full = hgin.full_softmax_link_loss(z["path"], z["link"][u], local, 0.7, known=local)
    full.backward()
    g_full = _grads(model)
    model.zero_grad()
    got = pred.batch_full_loss(sampler, pos, step=1)
    got.backward()
    _assert_close(got, full, _grads(model), g_full, f"full softmax / {which}")


def test_exclude_targets_off_is_the_predictor_without_the_keyword():
    import hgin
    from hgin.data import REL_PL
    _, dev = _graphs()
    model, _ = _model()
    pos = dev.edge_index[REL_PL][:, 40:200].contiguous()
    sampler = hgin.NeighborSampler(dev, fanouts=[3, 2], seed=5)
    old = hgin.LinkPredictor(model, REL_PL, k=4, seed=21, filter_negatives=True)
    off = hgin.LinkPredictor(model, REL_PL, k=4, seed=21, filter_negatives=True, exclude_targets=False,
                             rev_relation=None)
    on = hgin.LinkPredictor(model, REL_PL, k=4, seed=21, filter_negatives=True, exclude_targets=True)
    with torch.no_grad():
        assert torch.equal(old.batch_loss(sampler, pos, step=3), off.batch_loss(sampler, pos, step=3))
        assert torch.equal(old.batch_full_loss(sampler, pos, step=3), off.batch_full_loss(sampler, pos, step=3))
        assert not torch.equal(old.batch_loss(sampler, pos, step=3), on.batch_loss(sampler, pos, step=3))
        # the drawn negatives are seeds but never excluded pairs: the batch built by hand from them gives the bits
        from hgin.linkpred import negative_edges
        B = int(pos.size(1))
        neg = negative_edges(pos, int(dev.x["link"].size(0)), 4, 21, 3 * B * 4, known=dev.edge_index[REL_PL])[1]
        batch = hgin.link_neighbor_batch_excl(sampler, REL_PL, pos, neg.view(B, 4), offset=3)
        z = model.encode(batch.sub.graph.x_dict(), batch.sub.graph.edge_index_dict())
        want = hgin.sampled_link_loss(z["path"], z["link"], batch.pos, 0, 21, 0, neg_dst=batch.neg_dst)
        assert torch.equal(on.batch_loss(sampler, pos, step=3), want)
        assert torch.equal(batch.sub.n_id["link"][batch.neg_dst.long()], neg.view(B, 4))


def test_five_minibatch_steps_with_exclusion_are_reproducible():
    import hgin
    from hgin.data import REL_PL
    _, dev = _graphs()
    pos = dev.edge_index[REL_PL]
    runs = []
    for exclude in (True, True, False):
        model, _layers = _model(seed=5)
        opt = torch.optim.Adam(model.parameters(), lr=1e-2)
        pred = hgin.LinkPredictor(model, REL_PL, k=3, seed=8, exclude_targets=exclude)
        sampler = hgin.NeighborSampler(dev, fanouts=[3, 2], seed=2)
        losses = [hgin.link_minibatch_step(model, opt, sampler, pred, pos[:, 64 * s:64 * s + 64].contiguous(), s)
                  for s in range(5)]
        runs.append((torch.stack(losses), [p.detach().clone() for p in model.parameters()]))
    (l1, p1), (l2, p2), (l3, _) = runs
    assert bool(torch.isfinite(l1).all())
    assert torch.equal(l1, l2)
    assert all(torch.equal(a, b) for a, b in zip(p1, p2))
    assert not torch.equal(l1, l3)                     # the exclusion changes what the batches see
