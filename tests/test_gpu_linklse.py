"""Full-candidate softmax link loss (A23) on the MI355X against the float64 restatement of tests/test_linklse_host.py:
the forward within its derived bound over a grid of shapes, in the multi-tile / multi-split regime, on unaligned rows
and at large scores; known sets (everything known, a hub row over whole tiles, entries at a split boundary); both
gradients within their derived bounds through every path of the backward kernel; determinism; cross-checks against
``sampled_link_loss``, ``link_lse_unfused`` and ``link_topk``; ``full_softmax_link_loss`` with ``known``; and
``LinkPredictor.full_loss`` / ``batch_full_loss``.

Geometry (csrc/hgin_linklse.hip = the A15 sweep): 128 queries x 128 destinations per tile, splits by ``sweep_plan``
(for the destination gradient with the roles swapped), 128 output features per backward workgroup, 256 once F > 128."""
import functools

import numpy as np
import pytest
import torch

from test_linklse_host import (U, inv_t_of, lse_candidate_mask, ref_full_softmax, ref_lse, ref_lse_grads, ref_lse_tol)

DEV = "cuda"
pytestmark = pytest.mark.gpu


def _inputs(Q, n_dst, F, seed, n_src=None, scale=0.5):
    """float32 embeddings, Q distinct sources in random order out of n_src > Q rows."""
    g = np.random.default_rng(seed)
    n_src = Q + 7 if n_src is None else n_src
    zs = (g.standard_normal((n_src, F)) * scale).astype(np.float32)
    zd = (g.standard_normal((n_dst, F)) * scale).astype(np.float32)
    src = g.permutation(n_src)[:Q].astype(np.int64)
    return zs, zd, src, g


def _random_known(g, src, n_dst, degree):
    """About ``degree`` known destinations for two thirds of the sources (the others have none), repeats included."""
    some = src[g.random(src.size) < 2 / 3]
    if some.size == 0 or n_dst == 0:
        return None
    s = np.repeat(some, degree)
    return np.stack([s, g.integers(0, n_dst, s.size)])


def _t(a, dtype=None):
    return None if a is None else torch.as_tensor(a, dtype=dtype).to(DEV)


def _fwd(zs, zd, src, T=1.0, known=None):
    """(lse float32 numpy, launch tags) of ``link_lse`` on device copies (tensors already on the device pass as is)."""
    from hgin import _lib
    from hgin.linkpred import link_lse
    zs, zd = (z if isinstance(z, torch.Tensor) else _t(z) for z in (zs, zd))
    with _lib.trace_launches() as tr:
        lse = link_lse(zs, zd, _t(src), T, _t(known))
    assert lse.dtype == torch.float32 and lse.is_cuda and tuple(lse.shape) == (len(src),)
    return lse.cpu().numpy(), tr.kernels


def _grads(zs, zd, src, g_up, T=1.0, known=None):
    """(lse, G_src, G_dst as numpy, launch tags): forward, then backward with the upstream gradient ``g_up``."""
    from hgin import _lib
    from hgin.linkpred import link_lse
    zs_d, zd_d = _t(zs).requires_grad_(True), _t(zd).requires_grad_(True)
    with _lib.trace_launches() as tr:
        lse = link_lse(zs_d, zd_d, _t(src), T, _t(known))
        lse.backward(_t(g_up, torch.float32))
    return lse.detach().cpu().numpy(), zs_d.grad.cpu().numpy(), zd_d.grad.cpu().numpy(), tr.kernels


def _check_fwd(got, zs, zd, src, T, known, tag):
    want = ref_lse(zs, zd, src, T, known)
    tol = ref_lse_tol(zs, zd, src, T, known)
    empty = ~np.isfinite(want)
    assert np.array_equal(np.isneginf(got), empty), (tag, "a query without candidates must give -inf and only it")
    err = np.abs(got[~empty].astype(np.float64) - want[~empty])
    worst = float((err / tol[~empty]).max()) if err.size else 0.0
    print(f"{tag}: max |lse - ref| / tol = {worst:.3f} over {err.size} queries ({int(empty.sum())} empty)")
    assert worst <= 1.0, (tag, worst)
    return want, tol


def _check_grads(G_src, G_dst, zs, zd, src, g_up, T, known, tag):
    want_s, want_d, A_s, A_d = ref_lse_grads(zs, zd, src, g_up, T, known)
    tol = ref_lse_tol(zs, zd, src, T, known)
    n_cand = int(lse_candidate_mask(src, zs.shape[0], zd.shape[0], known).sum(1).max())
    F = zs.shape[1]
    for name, got, want, A, n in (("G_src", G_src, want_s, A_s, n_cand), ("G_dst", G_dst, want_d, A_d, len(src))):
        assert np.isfinite(got).all(), (tag, name)
        bound = (4.0 * tol.max() + (n + F + 64) * U) * A
        err = np.abs(got.astype(np.float64) - want)
        zero = A == 0.0
        assert (got[zero] == 0.0).all(), (tag, name, "an element nothing contributes to must be an exact zero")
        worst = float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
        print(f"{tag}: {name}: max err / bound = {worst:.3f}, {int(zero.sum())} exact zeros of {got.size}")
        assert worst <= 1.0, (tag, name, worst)
    not_src = np.setdiff1d(np.arange(zs.shape[0]), src)
    assert (G_src[not_src] == 0.0).all(), (tag, "rows of z_src that are no query's source")


def _tag_of(tags, prefix):
    hit = [t for t in tags if t.startswith(prefix)]
    assert len(hit) == 1, (prefix, tags)
    return hit[0]


# ---------------------------------------------------------------------------------------------------
# 1. the forward
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_dst", [1, 127, 129, 300])
@pytest.mark.parametrize("Q", [1, 129])
def test_forward_over_the_shape_grid(Q, n_dst):
    """F = 1, 7, 8, 36, 128 at every (Q, n_dst): one and two query blocks, one to three tiles, rows that end inside a
    tile; without known edges and with a random known set (temperature 0.7)."""
    for F in (1, 7, 8, 36, 128):
        zs, zd, src, g = _inputs(Q, n_dst, F, seed=100 * F + Q + n_dst)
        for known, T in ((None, 1.0), (_random_known(g, src, n_dst, 3), 0.7)):
            got, tags = _fwd(zs, zd, src, T, known)
            _tag_of(tags, f"k_lse_sweep<{4 if F % 4 == 0 else 1}> splits={min(-(-512 // -(-Q // 128)), -(-n_dst // 128))} ")
            _check_fwd(got, zs, zd, src, T, known, (Q, n_dst, F, known is not None))


BIG = (32768, 600, 8)      # 256 query blocks: 2 splits of 3 and 2 tiles; the destination side: 5 tiles, 86 splits of 3


@functools.lru_cache(maxsize=None)
def _big():
    """The multi-tile shape with its known set and references, computed once: about 3 known destinations per source,
    plus, for the first 64 queries, the destinations 383 and 384 on either side of the split boundary (tile 3), and a hub
    source that knows the destinations 100 .. 499."""
    Q, n_dst, F = BIG
    zs, zd, src, g = _inputs(Q, n_dst, F, seed=77, n_src=Q + 100)
    edge = np.stack([np.repeat(src[:64], 2), np.tile([383, 384], 64)])
    hub = np.stack([np.full(400, src[100]), np.arange(100, 500)])        # whole tiles inside one split's sweep
    known = np.concatenate([_random_known(g, src, n_dst, 3), edge, hub], 1)
    g_up = g.standard_normal(Q) * (g.random(Q) < 0.8)         # zeros and negative values
    return zs, zd, src, known, g_up


def test_forward_with_more_than_one_tile_per_split():
    zs, zd, src, known, _ = _big()
    for kn in (None, known):
        got, tags = _fwd(zs, zd, src, 1.0, kn)
        assert _tag_of(tags, "k_lse_sweep") == "k_lse_sweep<4> splits=2 sweep=3", tags
        assert _tag_of(tags, "k_lse_merge") == "k_lse_merge splits=2"
        _check_fwd(got, zs, zd, src, 1.0, kn, ("big", kn is not None))


def test_forward_on_unaligned_rows_and_at_large_scores():
    """A column window at an odd offset of wider tensors (the scalar load path), and scores of magnitude about 80 at
    temperature 0.1: t reaches several hundred, far past where exp overflows without the running maximum."""
    Q, n_dst, F = 129, 300, 36
    zs_w, zd_w, src, _ = _inputs(Q, n_dst, F + 5, seed=31)
    zs_d, zd_d = _t(zs_w)[:, 3:3 + F], _t(zd_w)[:, 3:3 + F]
    assert not zs_d.is_contiguous() and zs_d.data_ptr() % 16 != 0
    got, tags = _fwd(zs_d, zd_d, src)
    assert _tag_of(tags, "k_lse_sweep").startswith("k_lse_sweep<1> ")
    _check_fwd(got, zs_w[:, 3:3 + F], zd_w[:, 3:3 + F], src, 1.0, None, "strided")

    zs, zd, src, g = _inputs(Q, n_dst, 64, seed=32, scale=3.3)     # |score| ~ 3.3^2 * 8 = 87
    got, _ = _fwd(zs, zd, src, 0.1)
    assert np.isfinite(got).all() and float(np.abs(got).max()) > 400.0
    _check_fwd(got, zs, zd, src, 0.1, None, "large scores")


# ---------------------------------------------------------------------------------------------------
# 2. known sets
# ---------------------------------------------------------------------------------------------------
def test_known_sets_all_known_hub_boundary_and_none():
    """Source A knows every destination (lse = -inf, no gradient anywhere from it, no NaN); hub source B knows
    destinations 100 .. 399 (tiles 1 and 2 entirely, parts of tiles 0 and 3); source C knows 127, 128, 255, 256 (the
    first and last rows of tiles); the other sources know nothing.  420 destinations are 4 splits of one tile for one
    query block, so B's row crosses three split boundaries and a cursor opens in the middle of it."""
    Q, n_dst, F = 40, 420, 16
    zs, zd, src, g = _inputs(Q, n_dst, F, seed=9)
    a, b, c = (int(v) for v in src[[3, 17, 39]])
    known = np.concatenate([np.stack([np.full(n_dst, a), np.arange(n_dst)]),
                            np.stack([np.full(300, b), np.arange(100, 400)]),
                            np.stack([np.full(4, c), np.array([127, 128, 255, 256])])], 1)
    known = known[:, g.permutation(known.shape[1])]
    g_up = g.standard_normal(Q)
    g_up[5] = 0.0
    lse, G_src, G_dst, tags = _grads(zs, zd, src, g_up, 1.0, known)
    assert _tag_of(tags, "k_lse_sweep") == "k_lse_sweep<4> splits=4 sweep=1"
    _check_fwd(lse, zs, zd, src, 1.0, known, "known sets")
    assert np.isneginf(lse[3]) and np.isfinite(np.delete(lse, 3)).all()
    _check_grads(G_src, G_dst, zs, zd, src, g_up, 1.0, known, "known sets")
    assert (G_src[a] == 0.0).all() and (G_src[int(src[5])] == 0.0).all()
    # every source known to everything: all -inf, all gradients exactly zero
    everything = np.stack([np.repeat(src, n_dst), np.tile(np.arange(n_dst), Q)])
    lse, G_src, G_dst, _ = _grads(zs, zd, src, g_up, 1.0, everything)
    assert np.isneginf(lse).all() and (G_src == 0.0).all() and (G_dst == 0.0).all()


# ---------------------------------------------------------------------------------------------------
# 3. the backward
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_dst", [1, 127, 129, 300])
@pytest.mark.parametrize("Q", [1, 129])
def test_backward_over_the_shape_grid(Q, n_dst):
    """The forward's grid (every shape is small in float64): F = 1, 7, 8, 36, 128 at every (Q, n_dst), without known
    edges and with a random known set (temperature 0.7), upstream gradients with zeros and negative values.  F = 36 and
    128 run the 128-feature workgroup with more than one live column block per wave and with both feature halves
    (waves wn = 0 and 1).  The trace is asserted per shape: the query-stationary kernel is cut into one split per
    destination tile, the destination-stationary one into one split per query block, one tile swept each, one feature
    chunk; a fold wherever there is more than one split."""
    tiles, blocks = -(-n_dst // 128), -(-Q // 128)
    for F in (1, 7, 8, 36, 128):
        vec = 4 if F % 4 == 0 else 1
        zs, zd, src, g = _inputs(Q, n_dst, F, seed=900 * F + Q + n_dst)
        g_up = g.standard_normal(Q) * (g.random(Q) < 0.8)
        if Q == 1:
            g_up[0] = -1.5
        for known, T in ((None, 1.0), (_random_known(g, src, n_dst, 3), 0.7)):
            lse, G_src, G_dst, tags = _grads(zs, zd, src, g_up, T, known)
            assert _tag_of(tags, "k_lse_sweep") == f"k_lse_sweep<{vec}> splits={tiles} sweep=1", tags
            assert _tag_of(tags, "k_lse_bwd<%d,SRC>" % vec) == f"k_lse_bwd<{vec},SRC> splits={tiles} sweep=1 chunks=1", tags
            assert _tag_of(tags, "k_lse_bwd<%d,DST>" % vec) == f"k_lse_bwd<{vec},DST> splits={blocks} sweep=1 chunks=1", tags
            assert sorted(t for t in tags if t.startswith("k_lse_fold")) == sorted(
                ([f"k_lse_fold<SRC> splits={tiles}"] if tiles > 1 else [])
                + ([f"k_lse_fold<DST> splits={blocks}"] if blocks > 1 else [])), tags
            _check_fwd(lse, zs, zd, src, T, known, (Q, n_dst, F, known is not None))
            _check_grads(G_src, G_dst, zs, zd, src, g_up, T, known, (Q, n_dst, F, known is not None))


def test_backward_through_every_path():
    """Shapes and the paths they take (asserted from the trace):
      (129, 300, 7)   scalar loads; G_src: 2 query blocks x 3 splits of one tile, folded; G_dst: 3 tiles x 2 splits of
                      one query block, folded
      (100, 120, 8)   one workgroup each, one split: rows written straight to the outputs, no fold
      (129, 300, 130) the 256-feature workgroup (F > 128), its last three column blocks empty or 2 features wide
      (129, 300, 260) two output-feature chunks of 256, the second 4 features wide
      BIG             (32768, 600, 8) G_src: 2 splits sweeping 3 and 2 tiles; G_dst: 86 splits sweeping 3 query blocks;
                      both folded."""
    for Q, n_dst, F, vec, s_src, s_dst, chunks in ((129, 300, 7, 1, 3, 2, 1), (100, 120, 8, 4, 1, 1, 1),
                                                   (129, 300, 130, 1, 3, 2, 1), (129, 300, 260, 4, 3, 2, 2)):
        zs, zd, src, g = _inputs(Q, n_dst, F, seed=500 + F)
        known = _random_known(g, src, n_dst, 4)
        g_up = g.standard_normal(Q) * (g.random(Q) < 0.8)
        lse, G_src, G_dst, tags = _grads(zs, zd, src, g_up, 0.8, known)
        assert _tag_of(tags, "k_lse_bwd<%d,SRC>" % vec) == f"k_lse_bwd<{vec},SRC> splits={s_src} sweep=1 chunks={chunks}"
        assert _tag_of(tags, "k_lse_bwd<%d,DST>" % vec) == f"k_lse_bwd<{vec},DST> splits={s_dst} sweep=1 chunks={chunks}"
        assert sum(t.startswith("k_lse_fold") for t in tags) == (s_src > 1) + (s_dst > 1), tags
        _check_grads(G_src, G_dst, zs, zd, src, g_up, 0.8, known, (Q, n_dst, F))
    zs, zd, src, known, g_up = _big()
    lse, G_src, G_dst, tags = _grads(zs, zd, src, g_up, 1.0, known)
    assert _tag_of(tags, "k_lse_bwd<4,SRC>") == "k_lse_bwd<4,SRC> splits=2 sweep=3 chunks=1"
    assert _tag_of(tags, "k_lse_bwd<4,DST>") == "k_lse_bwd<4,DST> splits=86 sweep=3 chunks=1"
    assert "k_lse_fold<SRC> splits=2" in tags and "k_lse_fold<DST> splits=86" in tags
    _check_grads(G_src, G_dst, zs, zd, src, g_up, 1.0, known, "big")


def test_forward_and_gradients_are_bit_equal_over_two_calls():
    zs, zd, src, known, g_up = _big()
    a = _grads(zs, zd, src, g_up, 1.0, known)
    b = _grads(zs, zd, src, g_up, 1.0, known)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


# ---------------------------------------------------------------------------------------------------
# 4. cross-checks with the existing kernels
# ---------------------------------------------------------------------------------------------------
def test_cross_checks_with_sampled_loss_unfused_and_topk():
    from hgin.linkpred import full_softmax_link_loss, link_lse_unfused, link_topk, sampled_link_loss
    n_src, n_dst, F, E, T = 30, 40, 16, 50, 0.5
    g = np.random.default_rng(3)
    zs = (g.standard_normal((n_src, F)) * 0.5).astype(np.float32)
    zd = (g.standard_normal((n_dst, F)) * 0.5).astype(np.float32)
    pos = np.stack([g.integers(0, n_src, E), g.integers(0, n_dst, E)])
    zs_d, zd_d, pos_d = _t(zs), _t(zd), _t(pos)
    # every c != d as given negatives: InfoNCE over all of them is the full softmax
    neg = np.stack([np.delete(np.arange(n_dst), d) for d in pos[1]])
    full = float(full_softmax_link_loss(zs_d, zd_d, pos_d, T))
    sampled = float(sampled_link_loss(zs_d, zd_d, pos_d, 0, 1, 0, "softmax", T, neg_dst=_t(neg, torch.int32)))
    want = ref_full_softmax(zs, zd, pos, T)
    # either side: a mean of terms lse - t, each within its query's lse bound plus the rounding of its own t
    tol = ref_lse_tol(zs, zd, pos[0], T)
    t_own = np.abs((zs[pos[0]].astype(np.float64) * zd[pos[1]]).sum(1)) * inv_t_of(T)
    b_own = 2.0 * F * U * (np.abs(zs[pos[0]]).astype(np.float64) * np.abs(zd[pos[1]])).sum(1) * inv_t_of(T)
    side = float((tol + b_own + 2 * U * t_own).mean()) + 4 * U * abs(want)
    print(f"full {full:.8g} sampled {sampled:.8g} ref {want:.8g} bound per side {side:.3g}")
    assert abs(full - want) <= side and abs(sampled - want) <= side and abs(full - sampled) <= 2 * side

    zs, zd, src, g = _inputs(129, 300, 36, seed=41)
    known = _random_known(g, src, 300, 3)
    fused, _ = _fwd(zs, zd, src, T, known)
    unfused = link_lse_unfused(_t(zs), _t(zd), _t(src), T, _t(known)).cpu().numpy()
    want, tol = _check_fwd(fused, zs, zd, src, T, known, "fused vs unfused")
    fin = np.isfinite(want)
    assert np.array_equal(np.isneginf(unfused), ~fin)
    unfused_err = np.abs(unfused[fin] - want[fin])
    print(f"unfused: max error against float64 {unfused_err.max():.3g}")
    assert (np.abs(fused[fin].astype(np.float64) - unfused[fin]) <= tol[fin] + unfused_err).all()
    small = link_lse_unfused(_t(zs), _t(zd), _t(src), T, _t(known), chunk_rows=50).cpu().numpy()
    assert np.array_equal(np.isneginf(small), ~fin) and np.abs(small[fin] - want[fin]).max() <= 2 * unfused_err.max() + 1e-6

    _, top = link_topk(_t(zs), _t(zd), _t(src), 1, _t(known))
    top = top[:, 0].cpu().numpy()
    lse1, _ = _fwd(zs, zd, src, 1.0, known)
    assert (top[fin] <= lse1[fin]).all()            # the best candidate alone is one term of the sum (T = 1)
    assert (top[fin] * inv_t_of(T) <= fused[fin] * (1 + 2 * U) + 2 * U).all()
    assert np.array_equal(np.isneginf(top), ~fin)


def test_full_softmax_with_known_keeps_each_positive_and_drops_the_others():
    from hgin.linkpred import full_softmax_link_loss
    n_src, n_dst, F, T = 20, 150, 12, 0.6
    g = np.random.default_rng(8)
    zs = (g.standard_normal((n_src, F))).astype(np.float32)
    zd = (g.standard_normal((n_dst, F))).astype(np.float32)
    # source 4 has five positives, source 7 two (one of them listed twice), the rest one or none
    pos = np.array([[4, 4, 4, 4, 4, 7, 7, 7, 0, 1, 2, 3, 19], [0, 10, 128, 129, 149, 5, 6, 5, 1, 2, 3, 4, 77]])
    zd[pos[1, :5]] = zs[4] + 0.1 * zd[pos[1, :5]]     # a trained model: source 4's true edges are its dominant terms
    known = np.stack([g.integers(0, n_src, 60), g.integers(0, n_dst, 60)])
    for kn in (None, known, pos[:, :0]):
        zs_d, zd_d = _t(zs).requires_grad_(True), _t(zd).requires_grad_(True)
        loss = full_softmax_link_loss(zs_d, zd_d, _t(pos), T, _t(kn))
        want = ref_full_softmax(zs, zd, pos, T, kn)
        # per positive e the loss term is lse(s_e) - t_e (known = None) or softplus(lse_neg(s_e) - t_e):
        #   the log-sum-exp within its query's derived bound (over the candidates the kernel sums: without known
        #   edges, or without known u pos);
        #   t_e = fl32(score_e * inv_t): b_own for the fp32 dot product, u |t_e| for the product, u |t_e| more for the
        #   decoder's own rounding of the score;
        #   the difference x = lse - t_e rounds once more, u (|lse| + |t_e|), and softplus is 1-Lipschitz in x with a
        #   result good to a few ulp: 4 u |term|;
        #   the mean (or the two sums of the known = None form, which cancel down from sum |lse| + sum |t|) adds
        #   log2(E) + 2 roundings of partial sums no larger than sum_e (|lse_e| + |t_e|): that many u times their mean.
        union = None if kn is None else np.concatenate([kn, pos], 1)
        it, E = inv_t_of(T), pos.shape[1]
        tol = ref_lse_tol(zs, zd, pos[0], T, union)
        lse_e = ref_lse(zs, zd, pos[0], T, union)
        assert np.isfinite(lse_e).all() or kn is not None
        lse_abs = np.where(np.isfinite(lse_e), np.abs(lse_e), 0.0)
        own = (zs[pos[0]].astype(np.float64) * zd[pos[1]]).sum(1) * it
        b_own = 2.0 * F * U * (np.abs(zs[pos[0]]).astype(np.float64) * np.abs(zd[pos[1]])).sum(1) * it
        x = np.where(np.isfinite(lse_e), lse_e, -np.inf) - own
        term = np.abs(x) if kn is None else np.logaddexp(0.0, x)
        per = tol + b_own + 2 * U * np.abs(own) + U * (lse_abs + np.abs(own)) + 4 * U * term
        bound = float(per.mean()) + (np.log2(E) + 2) * U * float((lse_abs + np.abs(own)).mean())
        print(f"known={None if kn is None else kn.shape[1]}: loss {float(loss.detach()):.8g} ref {want:.8g} bound {bound:.3g}")
        assert abs(float(loss.detach()) - want) <= bound
        loss.backward()
        assert torch.isfinite(zs_d.grad).all() and torch.isfinite(zd_d.grad).all()
        # the loss is a mean of log-probabilities: its gradient moves no mass along the all-ones direction of t, and a
        # float64 finite difference of the restatement along a random direction agrees with the directional derivative
        d_s, d_d = g.standard_normal(zs.shape), g.standard_normal(zd.shape)
        h = 1e-6
        fd = (ref_full_softmax(zs + h * d_s, zd + h * d_d, pos, T, kn)
              - ref_full_softmax(zs - h * d_s, zd - h * d_d, pos, T, kn)) / (2 * h)
        got = float((zs_d.grad.double().cpu().numpy() * d_s).sum() + (zd_d.grad.double().cpu().numpy() * d_d).sum())
        assert abs(got - fd) <= 1e-4 * (1.0 + abs(fd)), (got, fd)
    without = ref_full_softmax(zs, zd, pos, T, None)
    # source 4's other positives left its denominators: each of its five terms loses about log 5
    assert ref_full_softmax(zs, zd, pos, T, pos[:, :0]) < without - 0.4


# ---------------------------------------------------------------------------------------------------
# 5. the predictor
# ---------------------------------------------------------------------------------------------------
def test_predictor_full_loss_and_batch_full_loss():
    """cfg1 at 0.3 with a hub link: finite losses, a gradient on every encoder parameter that has one under the sampled
    loss; with fanouts = [-1] * layers and a batch of every positive, ``batch_full_loss`` is ``full_softmax_link_loss``
    of the full graph's embeddings restricted to the batch's destination seeds."""
    import hgin
    from hgin.data import REL_PL
    from hgin.linkpred import full_softmax_link_loss
    from test_gpu_neighbor import _graphs, _model
    _, dev = _graphs()
    model, layers = _model()
    pos = dev.edge_index[REL_PL]
    T = 0.5
    sampler = hgin.NeighborSampler(dev, fanouts=[-1] * layers, seed=5)

    def grads_of(loss):
        model.zero_grad()
        loss.backward()
        have = {n: p.grad for n, p in model.named_parameters() if p.grad is not None}
        assert all(bool(torch.isfinite(v).all()) for v in have.values())
        assert any(bool(v.abs().sum() > 0) for v in have.values())
        return set(have)

    sampled = grads_of(hgin.LinkPredictor(model, REL_PL, k=3, seed=1, objective="softmax", temperature=T).loss(dev))
    for filt in (False, True):
        pred = hgin.LinkPredictor(model, REL_PL, k=1, seed=1, temperature=T, filter_negatives=filt)
        full = pred.full_loss(dev)
        assert full.dim() == 0 and bool(torch.isfinite(full)) and float(full) > 0
        assert grads_of(full) == sampled and sampled
        got = pred.batch_full_loss(sampler, pos, step=0)
        assert got.dim() == 0 and bool(torch.isfinite(got))
        assert grads_of(got) == sampled

        with torch.no_grad():
            z = model.encode(dev.x_dict(), dev.edge_index_dict())
            cand = torch.unique(pos[1])
            local = torch.stack([pos[0], torch.searchsorted(cand, pos[1])])
            want = full_softmax_link_loss(z["path"], z["link"][cand], local, T, known=local)
            zs, zd = z["path"].double(), z["link"][cand].double()
        # the sub-graph's seed embeddings are the full graph's within 1e-5 of the block's norm
        # (tests/test_gpu_neighbor.py); a loss term lse - t moves by at most twice the largest
        # |dt| <= inv_t (|dzs| |zd| + |zs| |dzd|)
        reach = 2 * 1e-5 * float(zs.norm() * zd.norm(dim=1).max() + zs.norm(dim=1).max() * zd.norm()) * inv_t_of(T)
        tol = ref_lse_tol(zs.cpu().numpy(), zd.cpu().numpy(), torch.unique(pos[0]).cpu().numpy(), T)
        bound = reach + 2 * (2 * float(tol.max()) + 8 * U * abs(float(want)))
        print(f"filter_negatives={filt}: batch {float(got):.8g} restricted full {float(want):.8g} bound {bound:.3g}")
        assert abs(float(got) - float(want)) <= bound
    pred = hgin.LinkPredictor(model, REL_PL, k=1, seed=1, temperature=T)
    a = float(pred.batch_full_loss(sampler, pos[:, :64].contiguous(), step=3, known=pos))
    b = float(pred.batch_full_loss(sampler, pos[:, :64].contiguous(), step=3, known=pos))
    assert a == b and np.isfinite(a)
