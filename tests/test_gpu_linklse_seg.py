"""Graph-local candidates for the full softmax link loss (A24) on the MI355X.  The reference is the float64 restatement
of tests/test_linklse_host.py with ``known`` augmented by every (source, out-of-segment destination) pair
(tests/test_linklse_seg_host.py shows on the CPU that this is the segmented loss written graph by graph); the bounds are
the project's own, evaluated on the augmented known set: ``ref_lse_tol`` for the forward and
(4 tol.max() + (n + F + 64) U) A for a gradient element with magnitude A (n = the largest candidate count for G_src, the
number of queries for G_dst), as tests/test_gpu_linklse.py::_check_grads has it.  Elements nothing contributes to must be
exact zeros.

Geometry (csrc/hgin_linklse.hip): 128 queries x 128 destinations per tile.  The forward and bwd_src cut the tiles a
query block's segments cover into the unsegmented plan's number of splits (slices may be empty); bwd_dst sweeps the
plan's query blocks and skips those whose covered destinations miss its tile."""
import functools

import numpy as np
import pytest
import torch

from test_linklse_host import (U, inv_t_of, lse_candidate_mask, ref_full_softmax, ref_lse, ref_lse_grads, ref_lse_probs,
                               ref_lse_tol)
from test_linklse_seg_host import augment_known, dst_ptr_of

DEV = "cuda"
pytestmark = pytest.mark.gpu

SIZES = (1, 126, 1, 0, 172)        # segment ends at 127 and 128: either side of the tile boundary; one empty graph
BIG = (32768, 600, 8)              # 256 query blocks, 5 destination tiles; bwd_dst: 86 splits of 3 query blocks
BIG_SIZES = (100, 28, 200, 72, 0, 200)
# queries per graph at BIG, sorted by graph: graph 3 ends inside block 180, the destination-less graph 4 owns block 181
# whole, graph 5 starts inside block 182; blocks 180 .. 182 are one bwd_dst slice
BIG_COUNTS = (5000, 4000, 11000, 3100, 200, 9468)


def _t(a, dtype=None):
    return None if a is None else torch.as_tensor(a, dtype=dtype).to(DEV)


def _segments(src_seg, sizes):
    from hgin.linkpred import LinkSegments
    return LinkSegments(_t(src_seg, torch.int64), _t(np.repeat(np.arange(len(sizes)), sizes), torch.int64), len(sizes))


def _run(zs, zd, src, g_up, T, known, seg):
    """(lse, G_src, G_dst as numpy, launch tags) of ``link_lse(segments=seg)`` forward + backward."""
    from hgin import _lib
    from hgin.linkpred import link_lse
    zs_d = (zs if isinstance(zs, torch.Tensor) else _t(zs)).detach().requires_grad_(True)
    zd_d = (zd if isinstance(zd, torch.Tensor) else _t(zd)).detach().requires_grad_(True)
    with _lib.trace_launches() as tr:
        lse = link_lse(zs_d, zd_d, _t(src), T, _t(known), segments=seg)
        lse.backward(_t(g_up, torch.float32))
    assert lse.dtype == torch.float32 and tuple(lse.shape) == (len(src),)
    return lse.detach().cpu().numpy(), zs_d.grad.cpu().numpy(), zd_d.grad.cpu().numpy(), tr.kernels


def _ref(zs, zd, src, g_up, T, aug):
    """The float64 reference and its bounds on the augmented known set, computed once per case."""
    want_s, want_d, A_s, A_d = ref_lse_grads(zs, zd, src, g_up, T, aug)
    return {"lse": ref_lse(zs, zd, src, T, aug), "tol": ref_lse_tol(zs, zd, src, T, aug), "G_src": want_s,
            "G_dst": want_d, "A_src": A_s, "A_dst": A_d, "F": zs.shape[1], "src": np.asarray(src),
            "n_cand": int(lse_candidate_mask(src, zs.shape[0], zd.shape[0], aug).sum(1).max())}


def _check(tag, ref, lse, G_src, G_dst, perm=None):
    """``perm``: the run's queries are the reference's in the order ``perm`` (the gradients do not depend on it)."""
    want = ref["lse"] if perm is None else ref["lse"][perm]
    tol = ref["tol"] if perm is None else ref["tol"][perm]
    empty = ~np.isfinite(want)
    assert np.array_equal(np.isneginf(lse), empty), (tag, "a query without candidates must give -inf and only it")
    err = np.abs(lse[~empty].astype(np.float64) - want[~empty])
    worst = float((err / tol[~empty]).max()) if err.size else 0.0
    print(f"{tag}: max |lse - ref| / tol = {worst:.3f} over {err.size} queries ({int(empty.sum())} empty)")
    assert worst <= 1.0, (tag, worst)
    for name, got, n in (("G_src", G_src, ref["n_cand"]), ("G_dst", G_dst, len(ref["src"]))):
        A = ref["A_" + name[2:]]
        assert np.isfinite(got).all(), (tag, name)
        bound = (4.0 * ref["tol"].max() + (n + ref["F"] + 64) * U) * A
        e = np.abs(got.astype(np.float64) - ref[name])
        zero = A == 0.0
        assert (got[zero] == 0.0).all(), (tag, name, "an element nothing contributes to must be an exact zero")
        worst = float((e[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
        print(f"{tag}: {name}: max err / bound = {worst:.3f}, {int(zero.sum())} exact zeros of {got.size}")
        assert worst <= 1.0, (tag, name, worst)
    src = ref["src"]
    assert (G_src[np.setdiff1d(np.arange(G_src.shape[0]), src)] == 0.0).all(), (tag, "rows that are no query's source")
    assert (G_src[src[~np.isfinite(ref["lse"])]] == 0.0).all(), (tag, "a source without candidates has no gradient")


def _tag_of(tags, prefix):
    hit = [t for t in tags if t.startswith(prefix)]
    assert len(hit) == 1, (prefix, tags)
    return hit[0]


def _case(Q, sizes, F, seed, scale=0.5):
    """Embeddings, Q distinct sources spread over all graphs (every graph has a query when Q allows, the empty ones too),
    an upstream gradient with zeros and negative values, and a random known set."""
    g = np.random.default_rng(seed)
    n_dst, G = int(sum(sizes)), len(sizes)
    n_src = Q + 7
    zs = (g.standard_normal((n_src, F)) * scale).astype(np.float32)
    zd = (g.standard_normal((n_dst, F)) * scale).astype(np.float32)
    src = g.permutation(n_src)[:Q].astype(np.int64)
    src_seg = g.integers(0, G, n_src)
    src_seg[src[:G]] = np.arange(G)[:min(G, Q)]
    g_up = g.standard_normal(Q) * (g.random(Q) < 0.8)
    if Q == 1:
        g_up[0] = -1.5
    some = src[g.random(Q) < 2 / 3]
    known = np.stack([np.repeat(some, 3), g.integers(0, n_dst, 3 * some.size)]) if some.size else None
    return zs, zd, src, src_seg, g_up, known


# ---------------------------------------------------------------------------------------------------
# 1. the shape grid
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [SIZES, (129,)], ids=["five_graphs", "one_graph"])
@pytest.mark.parametrize("Q", [1, 129])
def test_forward_and_gradients_over_the_shape_grid(Q, sizes):
    """F = 1, 7, 8, 36, 128; without known edges and with a random known set at temperature 0.7; the queries sorted by
    graph and in random order.  Sources sit in every graph, the one without destinations included (lse = -inf, exact
    zero rows of G_src: ``_check``)."""
    ptr = dst_ptr_of(sizes)
    n_dst, tiles = int(ptr[-1]), -(-int(ptr[-1]) // 128)
    for F in (1, 7, 8, 36, 128):
        vec = 4 if F % 4 == 0 else 1
        zs, zd, src, src_seg, g_up, known = _case(Q, sizes, F, seed=1000 * F + Q + n_dst)
        seg = _segments(src_seg, sizes)
        by_graph = np.argsort(src_seg[src], kind="stable")
        for kn, T in ((None, 1.0), (known, 0.7)):
            ref = _ref(zs, zd, src, g_up, T, augment_known(src, src_seg, ptr, kn))
            if len(sizes) > 1 and Q > 1:
                assert np.isneginf(ref["lse"][src_seg[src] == 3]).all() and (src_seg[src] == 3).any()
            for order, perm in (("sorted", by_graph), ("shuffled", None)):
                s, gu = (src, g_up) if perm is None else (src[perm], g_up[perm])
                lse, G_src, G_dst, tags = _run(zs, zd, s, gu, T, kn, seg)
                assert _tag_of(tags, "k_lse_sweep") == f"k_lse_sweep<{vec},SEG> splits={tiles} sweep=1", tags
                assert _tag_of(tags, f"k_lse_bwd<{vec},SRC") == f"k_lse_bwd<{vec},SRC,SEG> splits={tiles} sweep=1 chunks=1"
                assert _tag_of(tags, f"k_lse_bwd<{vec},DST") == \
                    f"k_lse_bwd<{vec},DST,SEG> splits={-(-Q // 128)} sweep=1 chunks=1", tags
                _check((Q, sizes, F, kn is not None, order), ref, lse, G_src, G_dst, perm)


# ---------------------------------------------------------------------------------------------------
# 2. / 3. empty slices, graphs without queries, graphs without destinations
# ---------------------------------------------------------------------------------------------------
def test_empty_slices_still_write_their_partials():
    """40 queries, 420 destinations: the plan is 4 splits of one tile.  Every query sits in the graph that owns the
    destinations 130 .. 250, all of them in tile 1, so the covered range is one tile and three of the four slices are
    empty: the merge and the fold still read all four.  No query touches tiles 0, 2, 3: their rows of G_dst (never
    cleared by the caller) must be written as zeros."""
    Q, F = 40, 16
    sizes = (130, 121, 169)                                   # destinations 130 .. 250 are graph 1
    zs, zd, src, src_seg, g_up, known = _case(Q, sizes, F, seed=91)
    src_seg[:] = 1
    ptr = dst_ptr_of(sizes)
    assert int(ptr[-1]) == 420 and (int(ptr[1]), int(ptr[2]) - 1) == (130, 250)
    seg = _segments(src_seg, sizes)
    for kn in (None, known):
        ref = _ref(zs, zd, src, g_up, 1.0, augment_known(src, src_seg, ptr, kn))
        lse, G_src, G_dst, tags = _run(zs, zd, src, g_up, 1.0, kn, seg)
        assert _tag_of(tags, "k_lse_sweep") == "k_lse_sweep<4,SEG> splits=4 sweep=1", tags
        assert "k_lse_merge splits=4" in tags and "k_lse_fold<SRC> splits=4" in tags
        assert _tag_of(tags, "k_lse_bwd<4,SRC") == "k_lse_bwd<4,SRC,SEG> splits=4 sweep=1 chunks=1"
        assert np.isfinite(lse).all()
        _check(("empty slices", kn is not None), ref, lse, G_src, G_dst)
        outside = np.r_[0:130, 251:420]
        assert (G_dst[outside] == 0.0).all() and np.abs(G_dst[130:251]).max() > 0.0
    # the same queries in a graph that spans tiles 1 and 2 (130 .. 300): two slices of one tile, two empty
    sizes = (130, 171, 119)
    ptr = dst_ptr_of(sizes)
    seg = _segments(src_seg, sizes)
    ref = _ref(zs, zd, src, g_up, 1.0, augment_known(src, src_seg, ptr, known))
    lse, G_src, G_dst, tags = _run(zs, zd, src, g_up, 1.0, known, seg)
    _check("two of four slices", ref, lse, G_src, G_dst)
    assert (G_dst[np.r_[0:130, 301:420]] == 0.0).all()


def test_graphs_without_queries_and_graphs_without_destinations():
    """Three graphs: graph 0 has destinations (0 .. 199, tiles 0 and 1) and no query; graph 1 has queries and no
    destination (lse = -inf, no gradient); graph 2 has both (200 .. 419).  More than one query block (Q = 200), so a
    whole block of destination-less queries is swept by bwd_dst."""
    Q, F = 200, 12
    sizes = (200, 0, 220)
    zs, zd, src, src_seg, g_up, known = _case(Q, sizes, F, seed=92)
    src_seg[:] = 0                                   # the sources that are no query sit in graph 0
    src_seg[src[:130]] = 1                           # the first block and two more queries: no destination
    src_seg[src[130:]] = 2
    ptr = dst_ptr_of(sizes)
    seg = _segments(src_seg, sizes)
    for kn in (None, known):
        ref = _ref(zs, zd, src, g_up, 0.7, augment_known(src, src_seg, ptr, kn))
        lse, G_src, G_dst, tags = _run(zs, zd, src, g_up, 0.7, kn, seg)
        _check(("no queries / no destinations", kn is not None), ref, lse, G_src, G_dst)
        assert np.isneginf(lse[:130]).all() and np.isfinite(lse[130:]).all()
        assert (G_dst[:200] == 0.0).all() and (G_src[src[:130]] == 0.0).all()
    # nobody has a destination: every output is -inf / an exact zero
    src_seg[:] = 1
    lse, G_src, G_dst, _ = _run(zs, zd, src, g_up, 1.0, known, _segments(src_seg, sizes))
    assert np.isneginf(lse).all() and (G_src == 0.0).all() and (G_dst == 0.0).all()


# ---------------------------------------------------------------------------------------------------
# 4. / 7. many query blocks per bwd_dst slice; determinism
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _big_seg():
    """The multi-tile shape of tests/test_gpu_linklse.py (its embeddings, known set with the hub and the split-boundary
    entries, upstream gradient) cut into 6 graphs; the queries, in their given order, are sorted by graph."""
    from test_gpu_linklse import _big
    zs, zd, src, known, g_up = _big()
    Q = len(src)
    assert sum(BIG_COUNTS) == Q and (Q, zd.shape[0], zs.shape[1]) == BIG
    src_seg = np.zeros(zs.shape[0], np.int64)
    src_seg[src] = np.repeat(np.arange(len(BIG_SIZES)), BIG_COUNTS)
    perm = np.random.default_rng(5).permutation(Q)
    return zs, zd, src, known, g_up, src_seg, dst_ptr_of(BIG_SIZES), perm


@functools.lru_cache(maxsize=None)
def _big_ref(with_known: bool):
    zs, zd, src, known, g_up, src_seg, ptr, _ = _big_seg()
    return _ref(zs, zd, src, g_up, 1.0, augment_known(src, src_seg, ptr, known if with_known else None))


def test_the_big_shape_skips_blocks_at_the_start_middle_and_end_of_a_slice():
    """What the queries' layout is there for, restated on the host: with the queries sorted, some (tile, slice of 3
    query blocks) has a skipped block first, one has it in the middle, one has it last."""
    _, _, src, _, _, src_seg, ptr, _ = _big_seg()
    g = src_seg[src]
    lo, hi = ptr[g], ptr[g + 1]
    n_blocks = -(-len(src) // 128)
    live = np.zeros((5, n_blocks), bool)
    for b in range(n_blocks):
        has = hi[b * 128:(b + 1) * 128] > lo[b * 128:(b + 1) * 128]
        if has.any():
            b_lo, b_hi = lo[b * 128:(b + 1) * 128][has].min(), hi[b * 128:(b + 1) * 128][has].max()
            for t in range(5):
                live[t, b] = b_lo < (t + 1) * 128 and b_hi > t * 128
    pats = {tuple(live[t, s:s + 3]) for t in range(5) for s in range(0, n_blocks - 2, 3)}
    assert (True, False, True) in pats and (False, False, True) in pats and (True, False, False) in pats
    assert (False, False, False) in pats and (True, True, True) in pats
    assert live.sum() < 0.45 * live.size                      # sorted queries skip most (tile, block) pairs


@pytest.mark.parametrize("with_known", [False, True], ids=["plain", "known"])
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
def test_many_query_blocks_per_slice(order, with_known):
    zs, zd, src, known, g_up, src_seg, ptr, perm = _big_seg()
    ref = _big_ref(with_known)
    seg = _segments(src_seg, BIG_SIZES)
    p = None if order == "sorted" else perm
    s, gu = (src, g_up) if p is None else (src[p], g_up[p])
    lse, G_src, G_dst, tags = _run(zs, zd, s, gu, 1.0, known if with_known else None, seg)
    assert _tag_of(tags, "k_lse_sweep") == "k_lse_sweep<4,SEG> splits=2 sweep=3", tags
    assert _tag_of(tags, "k_lse_bwd<4,SRC") == "k_lse_bwd<4,SRC,SEG> splits=2 sweep=3 chunks=1"
    assert _tag_of(tags, "k_lse_bwd<4,DST") == "k_lse_bwd<4,DST,SEG> splits=86 sweep=3 chunks=1"
    assert "k_lse_fold<SRC> splits=2" in tags and "k_lse_fold<DST> splits=86" in tags
    _check(("big", order, with_known), ref, lse, G_src, G_dst, p)
    assert np.isneginf(lse).sum() >= BIG_COUNTS[4]            # the queries of the graph without destinations


def test_forward_and_gradients_are_bit_equal_over_two_calls():
    zs, zd, src, known, g_up, src_seg, _, _ = _big_seg()
    seg = _segments(src_seg, BIG_SIZES)
    a = _run(zs, zd, src, g_up, 1.0, known, seg)
    b = _run(zs, zd, src, g_up, 1.0, known, seg)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


# ---------------------------------------------------------------------------------------------------
# 5. one graph is the unsegmented call
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(129, 300, 36), BIG, (129, 300, 260)], ids=["f36", "big", "f260"])
def test_one_graph_is_the_unsegmented_call_bit_for_bit(shape):
    """Under A19's slice rule a block whose queries cover every tile cuts ceil(n_tiles / splits) = tiles_per_split tiles
    per split: the unsegmented plan.  F = 260: the 256-feature workgroup with two feature chunks."""
    from hgin.linkpred import link_lse
    if shape == BIG:
        zs, zd, src, known, g_up = _big_seg()[:5]
    else:
        Q, n_dst, F = shape
        zs, zd, src, _, g_up, known = _case(Q, (n_dst,), F, seed=55 + F)
    seg = _segments(np.zeros(zs.shape[0], np.int64), (zd.shape[0],))
    assert seg.n_graphs == 1
    out = []
    for kw in ({}, {"segments": seg}):
        zs_d, zd_d = _t(zs).requires_grad_(True), _t(zd).requires_grad_(True)
        lse = link_lse(zs_d, zd_d, _t(src), 0.8, _t(known), **kw)
        lse.backward(_t(g_up, torch.float32))
        out.append((lse.detach(), zs_d.grad, zd_d.grad))
    for name, a, b in zip(("lse", "G_src", "G_dst"), *out):
        assert torch.equal(a, b), (shape, name)
    assert bool(torch.isfinite(out[0][0]).any()) and bool(out[0][2].abs().sum() > 0)


# ---------------------------------------------------------------------------------------------------
# 6. foreign rows cannot leak
# ---------------------------------------------------------------------------------------------------
def test_rows_of_other_graphs_do_not_reach_a_graph():
    """Every z_dst row outside graph 1 (destinations 1 .. 126) times 1e4 (finite: a masked weight of 0 still multiplies
    them in the second product): graph 1's lse, its sources' rows of G_src and its rows of G_dst keep their bits."""
    Q, F = 129, 36
    zs, zd, src, src_seg, g_up, known = _case(Q, SIZES, F, seed=66)
    seg = _segments(src_seg, SIZES)
    loud = zd.copy()
    loud[0] *= 1e4
    loud[127:] *= 1e4
    mine = src_seg[src] == 1
    assert mine.sum() > 10 and (~mine).sum() > 10
    for kn in (None, known):
        a = _run(zs, zd, src, g_up, 0.7, kn, seg)
        b = _run(zs, loud, src, g_up, 0.7, kn, seg)
        assert np.isfinite(b[1]).all() and np.isfinite(b[2]).all()
        assert np.array_equal(a[0][mine].view(np.uint32), b[0][mine].view(np.uint32))
        assert np.array_equal(a[1][src[mine]].view(np.uint32), b[1][src[mine]].view(np.uint32))
        assert np.array_equal(a[2][1:127].view(np.uint32), b[2][1:127].view(np.uint32))
        other = ~mine & np.isfinite(a[0])                       # the other graphs' queries did change
        assert not np.array_equal(a[0][other], b[0][other])


# ---------------------------------------------------------------------------------------------------
# 8. the scalar load path
# ---------------------------------------------------------------------------------------------------
def test_an_odd_offset_column_window():
    Q, F = 129, 36
    zs_w, zd_w, src, src_seg, g_up, known = _case(Q, SIZES, F + 5, seed=31)
    zs_d, zd_d = _t(zs_w)[:, 3:3 + F], _t(zd_w)[:, 3:3 + F]
    assert not zs_d.is_contiguous() and zs_d.data_ptr() % 16 != 0
    seg = _segments(src_seg, SIZES)
    zs, zd = zs_w[:, 3:3 + F], zd_w[:, 3:3 + F]
    ref = _ref(zs, zd, src, g_up, 1.0, augment_known(src, src_seg, dst_ptr_of(SIZES), known))
    lse, G_src, G_dst, tags = _run(zs_d, zd_d, src, g_up, 1.0, known, seg)
    assert _tag_of(tags, "k_lse_sweep").startswith("k_lse_sweep<1,SEG> ")
    assert _tag_of(tags, "k_lse_bwd<1,SRC").startswith("k_lse_bwd<1,SRC,SEG> ")
    assert _tag_of(tags, "k_lse_bwd<1,DST").startswith("k_lse_bwd<1,DST,SEG> ")
    _check("strided", ref, lse, G_src, G_dst)


# ---------------------------------------------------------------------------------------------------
# 9. cross-checks
# ---------------------------------------------------------------------------------------------------
def test_cross_checks_with_the_unfused_baseline_and_topk():
    from hgin.linkpred import link_lse, link_lse_unfused, link_topk
    Q, F, T = 129, 36, 0.5
    zs, zd, src, src_seg, g_up, known = _case(Q, SIZES, F, seed=41)
    seg = _segments(src_seg, SIZES)
    aug = augment_known(src, src_seg, dst_ptr_of(SIZES), known)
    want, tol = ref_lse(zs, zd, src, T, aug), ref_lse_tol(zs, zd, src, T, aug)
    fin = np.isfinite(want)
    fused = link_lse(_t(zs), _t(zd), _t(src), T, _t(known), segments=seg).cpu().numpy()
    assert np.array_equal(np.isneginf(fused), ~fin) and (np.abs(fused[fin] - want[fin]) <= tol[fin]).all()
    for kw in ({}, {"chunk_rows": 50}):
        unfused = link_lse_unfused(_t(zs), _t(zd), _t(src), T, _t(known), segments=seg, **kw).cpu().numpy()
        assert np.array_equal(np.isneginf(unfused), ~fin)
        unfused_err = np.abs(unfused[fin] - want[fin])       # the baseline's own error against float64, as measured
        print(f"unfused {kw}: max error against float64 {unfused_err.max():.3g}")
        assert (np.abs(fused[fin].astype(np.float64) - unfused[fin]) <= tol[fin] + unfused_err).all()
    # a query has a finite lse exactly when top-1 retrieval over the same candidates returns a destination
    idx, top = link_topk(_t(zs), _t(zd), _t(src), 1, _t(known), segments=seg)
    assert np.array_equal(idx[:, 0].cpu().numpy() >= 0, fin) and (~fin).sum() > 0
    lse1 = link_lse(_t(zs), _t(zd), _t(src), 1.0, _t(known), segments=seg).cpu().numpy()
    assert (top[:, 0].cpu().numpy()[fin] <= lse1[fin]).all()   # the best candidate alone is one term of the sum


# ---------------------------------------------------------------------------------------------------
# 10. full_softmax_link_loss(segments=)
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _components():
    import hgin
    from hgin.data import CONFIGS, REL_PL, component_graph
    cfg = CONFIGS["cfg1"]
    g = component_graph(cfg, 3).to(DEV)
    return cfg, g, hgin.LinkSegments.of(g, REL_PL), REL_PL


def test_full_softmax_link_loss_over_each_positives_own_graph():
    """Random embeddings with the row counts, the positives and the segmentation of ``component_graph(cfg1, 3)``.
    known = None: the mean of lse(s_e) - t_e over the graph-local candidates; with ``known``: ``ref_full_softmax`` on
    known + the out-of-segment pairs.  The loss bound is the one tests/test_gpu_linklse.py derives term by term.  The
    gradients are checked against the same composition on ``link_lse_unfused(segments=)``: the fused side within
    (4 tol.max() + (n + F + 64) U) A, A = the sum of the absolute terms of an element's gradient
    (every positive weighs 1 / E, a softplus' slope is at most 1 and its error, a quarter of the error of its argument,
    fits the slack the factor 4 leaves over the 2 tol of exp(t - lse)), plus the baseline's own measured error against a
    float64 autograd of the restatement."""
    from hgin.linkpred import full_softmax_link_loss, link_lse_unfused
    _, graph, seg, rel = _components()
    pos_d = graph.edge_index[rel]
    pos = pos_d.cpu().numpy()
    n_src, n_dst, F, T = seg.n_src, seg.n_dst, 12, 0.6
    assert seg.n_graphs == 3 and n_dst == 300
    g = np.random.default_rng(10)
    zs = g.standard_normal((n_src, F)).astype(np.float32)
    zd = g.standard_normal((n_dst, F)).astype(np.float32)
    src_seg, ptr = seg.src_seg.cpu().numpy(), seg.dst_ptr.cpu().numpy().astype(np.int64)
    known = np.stack([g.integers(0, n_src, 400), g.integers(0, n_dst, 400)])
    it, E = inv_t_of(T), pos.shape[1]
    u, inv = np.unique(pos[0], return_inverse=True)
    own = (zs[pos[0]].astype(np.float64) * zd[pos[1]]).sum(1) * it
    b_own = 2.0 * F * U * (np.abs(zs[pos[0]]).astype(np.float64) * np.abs(zd[pos[1]])).sum(1) * it
    for kn in (None, known):
        aug = augment_known(u, src_seg, ptr, kn if kn is None else np.concatenate([kn, pos], 1))
        lse_u, tol_u = ref_lse(zs, zd, u, T, aug), ref_lse_tol(zs, zd, u, T, aug)
        if kn is None:
            assert np.isfinite(lse_u).all()
            want = float((lse_u[inv] - own).mean())
            term = np.abs(lse_u[inv] - own)
        else:
            want = ref_full_softmax(zs, zd, pos, T, augment_known(u, src_seg, ptr, kn))
            term = np.logaddexp(0.0, np.where(np.isfinite(lse_u[inv]), lse_u[inv], -np.inf) - own)
        lse_abs = np.where(np.isfinite(lse_u[inv]), np.abs(lse_u[inv]), 0.0)
        per = tol_u[inv] + b_own + 2 * U * np.abs(own) + U * (lse_abs + np.abs(own)) + 4 * U * term
        bound = float(per.mean()) + (np.log2(E) + 2) * U * float((lse_abs + np.abs(own)).mean())
        zs_d, zd_d = _t(zs).requires_grad_(True), _t(zd).requires_grad_(True)
        loss = full_softmax_link_loss(zs_d, zd_d, pos_d, T, _t(kn), segments=seg)
        got_loss = float(loss.detach())
        print(f"known={kn is not None}: loss {got_loss:.8g} ref {want:.8g} bound {bound:.3g}")
        assert abs(got_loss - want) <= bound
        loss.backward()

        # the same composition, unfused (float32 on the device) and in float64 on the host
        def compose(zs_t, zd_t, lse_of, pos_t, inv_t_):
            t_e = (zs_t[pos_t[0]] * zd_t[pos_t[1]]).sum(1) * inv_t_
            lse_e = lse_of(zs_t, zd_t)[torch.as_tensor(inv, device=zs_t.device)]
            return (lse_e - t_e).mean() if kn is None else torch.nn.functional.softplus(lse_e - t_e).mean()

        zs_u, zd_u = _t(zs).requires_grad_(True), _t(zd).requires_grad_(True)
        both = None if kn is None else _t(np.concatenate([kn, pos], 1))
        compose(zs_u, zd_u, lambda a, b: link_lse_unfused(a, b, _t(u), T, both, segments=seg), pos_d, it).backward()
        zs_r, zd_r = torch.tensor(zs, dtype=torch.float64, requires_grad=True), torch.tensor(zd, dtype=torch.float64,
                                                                                             requires_grad=True)
        cand = torch.as_tensor(lse_candidate_mask(u, n_src, n_dst, aug))

        def lse64(a, b):
            return torch.logsumexp(((a[torch.as_tensor(u)] @ b.t()) * it).masked_fill(~cand, float("-inf")), 1)

        compose(zs_r, zd_r, lse64, torch.as_tensor(pos), it).backward()
        P = ref_lse_probs(zs, zd, u, T, aug)[inv]                                   # [E, n_dst]
        A_src, A_dst = np.zeros(zs.shape), np.zeros(zd.shape)
        np.add.at(A_src, pos[0], (P @ np.abs(zd) + np.abs(zd[pos[1]])) * it / E)
        A_dst += it / E * (P.T @ np.abs(zs[pos[0]]).astype(np.float64))
        np.add.at(A_dst, pos[1], np.abs(zs[pos[0]]) * it / E)
        n_cand = int(lse_candidate_mask(u, n_src, n_dst, aug).sum(1).max())
        for name, got, unf, ref64, A, n in (("z_src", zs_d.grad, zs_u.grad, zs_r.grad, A_src, n_cand),
                                            ("z_dst", zd_d.grad, zd_u.grad, zd_r.grad, A_dst, E)):
            got, unf, ref64 = got.double().cpu().numpy(), unf.double().cpu().numpy(), ref64.numpy()
            assert np.isfinite(got).all() and np.isfinite(unf).all()
            fused_bound = (4.0 * tol_u.max() + (n + F + 64) * U) * A
            unf_err = np.abs(unf - ref64)
            worst = float((np.abs(got - unf) / (fused_bound + unf_err + 1e-300)).max())
            print(f"known={kn is not None}: d {name}: max |fused - unfused| / bound = {worst:.3f}")
            assert worst <= 1.0, (name, worst)
            assert (got[A == 0.0] == 0.0).all()


# ---------------------------------------------------------------------------------------------------
# 11. the predictor
# ---------------------------------------------------------------------------------------------------
def test_predictor_full_loss_with_segments():
    import hgin
    from hgin.linkpred import full_softmax_link_loss
    cfg, graph, seg, rel = _components()
    torch.manual_seed(1997)
    ic = {"link": cfg.f_link, "path": cfg.f_path, "node": cfg.f_node}
    model = hgin.HetroGIN(**cfg.model_kwargs(ic)).to(DEV).train()
    pos = graph.edge_index[rel]
    T = 0.5
    recorded, encode = [], model.encode

    def recording_encode(*args, **kw):
        recorded.append(encode(*args, **kw))
        return recorded[-1]

    for filt in (False, True):
        pred = hgin.LinkPredictor(model, rel, k=1, seed=1, temperature=T, filter_negatives=filt)
        model.encode = recording_encode
        try:
            loss = pred.full_loss(graph, segments=seg)
        finally:
            model.encode = encode
        z = {k: v.detach() for k, v in recorded[-1].items()}
        direct = full_softmax_link_loss(z[rel[0]], z[rel[2]], pos, T, known=pos if filt else None, segments=seg)
        assert loss.dim() == 0 and bool(torch.isfinite(loss)) and torch.equal(loss.detach(), direct)
        whole = pred.full_loss(graph)                       # every destination of the batch: another, larger denominator
        assert float(whole.detach()) > float(loss.detach())
    pred = hgin.LinkPredictor(model, rel, k=1, seed=1, temperature=T)
    opt = torch.optim.Adam(model.parameters(), lr=3e-3)
    first = last = None
    for _ in range(8):
        opt.zero_grad()
        loss = pred.full_loss(graph, segments=seg)
        loss.backward()
        opt.step()
        last = float(loss.detach())
        first = last if first is None else first
    assert np.isfinite(last) and last < first, (first, last)
    local = hgin.LinkPredictor(model, rel, k=1, seed=1, graph_local=True)
    with pytest.raises(ValueError, match="hard > 0 and graph_local = True are not supported"):
        local.full_loss(graph, segments=seg)
