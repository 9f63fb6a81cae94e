"""The fused sampled link loss and the sampled ranks (A13 / A14) past the shapes of tests/test_gpu_linkpred.py.

That file keeps E = 211: the forward's persistent grid is at most 53 workgroups, a source owns about 42 items.  Here:

* more than ``kLinkMaxGrid`` = 4096 workgroups' worth of edges, so that ``k_link_fwd`` strides over its grid (LOSS
  and RANK variants; ONE / LOOP, float4 / scalar, wide and two-lane groups) and a later pass ends in idle groups;
  and a grid of more than 256 workgroups below the cap, for ``k_link_loss_sum``'s strided read on its own;
* hub rows: one source (one destination) owning all 4000 positives, the row checked by its own norm;
* saturated and degenerate scores (0, +-30, +-200 on integer-valued embeddings): every saved coefficient against
  float64.

References: the float64 ones of tests/test_linkpred_host.py built from the C oracle's negatives; bounds: the
project's 1e-5 |loss| and 1e-5 ||g|| + 1e-9.  Every scale test recomputes the launch arithmetic of ``link_shape``
(csrc/hgin_linkpred.hip) and asserts its regime next to the launch tag."""
import functools
import math

import numpy as np
import pytest
import torch

from test_gpu_linkpred import SEED, _check, _run_fused
from test_linkpred_host import ref_loss_and_grads, ref_ranks

DEV = "cuda"
pytestmark = pytest.mark.gpu

MAX_GRID = 4096          # kLinkMaxGrid
N_SRC, N_DST = 3000, 9000


def _cdiv(a, b):
    return -(-a // b)


def _fwd_plan(E, F, vec):
    """(launch tag without the epilogue, workgroups before the cap) as link_shape / launch_link_fwd choose them."""
    pieces = F // 4 if vec else F
    one = pieces <= 64
    g = 64
    if one:
        g = 1
        while g < pieces and g < 64:
            g <<= 1
    blocks = _cdiv(_cdiv(E, 64 // g), 4)
    return f"k_link_fwd<{4 if vec else 1},{g},{'ONE' if one else 'LOOP'}", blocks


def _inputs(E, n_src, n_dst, F, seed, integer=False):
    """Sources from the first nine tenths of the rows (the rest has no pair), destinations from the first four fifths
    (the rest is reached by drawn negatives only)."""
    g = torch.Generator().manual_seed(seed)
    pos = torch.stack([torch.randint(0, n_src - n_src // 10, (E,), generator=g),
                       torch.randint(0, n_dst - n_dst // 5, (E,), generator=g)])
    if integer:
        zs = torch.randint(-2, 3, (n_src, F), generator=g).float()
        zd = torch.randint(-2, 3, (n_dst, F), generator=g).float()
    else:
        zs = torch.randn(n_src, F, generator=g) * 0.5
        zd = torch.randn(n_dst, F, generator=g) * 0.5
    return pos, zs, zd


# name: (E, F, k, offset, column window, n_src, n_dst, tag)
SCALE = {
    "capped_one": (32919, 256, 1, 6, False, N_SRC, N_DST, "k_link_fwd<4,64,ONE,LOSS>"),
    "capped_loop": (32919, 260, 1, 2**32 + 1, False, N_SRC, N_DST, "k_link_fwd<4,64,LOOP,LOSS>"),
    "capped_scalar_window": (33000, 70, 2, 6, True, N_SRC, N_DST, "k_link_fwd<1,64,LOOP,LOSS>"),
    "capped_two_lane_groups": (600001, 8, 1, 6, False, N_SRC, N_DST, "k_link_fwd<4,2,ONE,LOSS>"),
    # 375 workgroups: below the cap, above the 256 threads of k_link_loss_sum
    "partials_past_256": (1500, 256, 3, 6, False, 300, 500, "k_link_fwd<4,64,ONE,LOSS>"),
}
CAPPED = [n for n in SCALE if n.startswith("capped")]


def _fused_on_views(vs, vd, leaves, posd, k, off):
    """One fused forward + backward; the gradients are those of ``leaves`` (the embeddings or the buffers they are
    windows of)."""
    from hgin import _lib
    from hgin.linkpred import sampled_link_loss
    for t in leaves:
        t.grad = None
    with _lib.trace_launches() as tr:
        loss = sampled_link_loss(vs, vd, posd, k, SEED, off)
        neg = loss.grad_fn.saved_tensors[1]
        loss.backward()
    return loss.detach(), leaves[0].grad, leaves[1].grad, neg, tr.kernels


@functools.lru_cache(maxsize=None)
def _case(name):
    from oracle import c_oracle
    E, F, k, off, window, n_src, n_dst, tag = SCALE[name]
    pos, zs, zd = _inputs(E, n_src, n_dst, F, seed=E + F)
    posd = pos.to(DEV)
    if window:   # column windows of wider buffers: odd row strides, starts not 16-byte aligned
        g = torch.Generator().manual_seed(5)
        bs, bd = torch.randn(n_src, 2 * F + 1, generator=g), torch.randn(n_dst, F + 3, generator=g)
        bs[:, 1:F + 1], bd[:, 3:] = zs, zd
        bs, bd = bs.to(DEV).requires_grad_(True), bd.to(DEV).requires_grad_(True)
        vs, vd = bs[:, 1:F + 1], bd[:, 3:]
        assert not vs.is_contiguous() and vs.stride(0) % 2 == 1 and vd.stride(0) % 2 == 1
        leaves = (bs, bd)
        cut = lambda gs, gd: (gs[:, 1:F + 1], gd[:, 3:])  # noqa: E731
    else:
        vs, vd = zs.to(DEV).requires_grad_(True), zd.to(DEV).requires_grad_(True)
        leaves = (vs, vd)
        cut = lambda gs, gd: (gs, gd)  # noqa: E731
    loss, gs, gd, neg, tags = _fused_on_views(vs, vd, leaves, posd, k, off)
    loss2, gs2, gd2, neg2, _ = _fused_on_views(vs, vd, leaves, posd, k, off)
    want_neg = c_oracle.neg_sample(SEED, off, E * k, n_dst)
    ref = ref_loss_and_grads(zs, zd, pos, want_neg, k)
    g_src, g_dst = cut(gs, gd)
    return dict(pos=pos, loss=loss, g_src=g_src, g_dst=g_dst, neg=neg, full=(gs, gd), tags=tags, want_neg=want_neg,
                ref=ref, second=(loss2, gs2, gd2, neg2))


def _assert_regime(name, tags):
    E, F, k, off, window, n_src, n_dst, tag = SCALE[name]
    head, blocks = _fwd_plan(E, F, vec=not window)
    assert tag == head + ",LOSS>" and tag in tags and "k_link_loss_sum" in tags, (tag, head, tags)
    if name in CAPPED:
        assert blocks > MAX_GRID, (name, blocks)          # a wave takes more than one pass of the grid
    else:
        assert 256 < blocks <= MAX_GRID, (name, blocks)   # uncapped, and more partials than the final sum's threads
    return blocks


@pytest.mark.parametrize("name", list(SCALE))
def test_scale_negatives_are_the_oracle_samplers(name):
    c = _case(name)
    blocks = _assert_regime(name, c["tags"])
    E, F, k = SCALE[name][:3]
    if name == "capped_two_lane_groups":
        # 32 edges per wave: the last wave of the second pass holds one valid edge and 31 idle groups
        waves, per_pass = _cdiv(E, 32), MAX_GRID * 4
        assert blocks == 4688 and per_pass < waves <= 2 * per_pass and E - (waves - 1) * 32 == 1
    neg = c["neg"].cpu()
    assert neg.dtype == torch.int64 and tuple(neg.shape) == (2, E * k)
    assert np.array_equal(neg[1].numpy(), c["want_neg"].astype(np.int64))
    assert torch.equal(neg[0], c["pos"][0].repeat_interleave(k))


@pytest.mark.parametrize("name", list(SCALE))
def test_scale_loss_and_gradients_vs_float64_reference(name):
    c = _case(name)
    _assert_regime(name, c["tags"])
    assert c["loss"].dim() == 0 and c["loss"].dtype == torch.float32
    _check(c["loss"], c["g_src"], c["g_dst"], c["ref"], f"{name}: fused vs float64")


@pytest.mark.parametrize("name", list(SCALE))
def test_scale_bitwise_determinism_and_exact_zero_rows(name):
    c = _case(name)
    _assert_regime(name, c["tags"])
    E, F, k, off, window, n_src, n_dst, _ = SCALE[name]
    loss2, gs2, gd2, neg2 = c["second"]
    assert torch.equal(loss2, c["loss"]) and torch.equal(neg2, c["neg"])
    assert torch.equal(gs2, c["full"][0]) and torch.equal(gd2, c["full"][1])
    no_pos = torch.ones(n_src, dtype=torch.bool)
    no_pos[c["pos"][0]] = False
    assert int(no_pos.sum()) >= n_src // 10
    rows = c["g_src"].cpu()[no_pos]
    assert bool((rows == 0).all()) and not bool(torch.signbit(rows).any())
    untouched = torch.ones(n_dst, dtype=torch.bool)
    untouched[c["pos"][1]] = False
    untouched[torch.as_tensor(c["want_neg"].astype(np.int64))] = False
    if name in ("capped_one", "capped_loop"):
        assert int(untouched.sum()) >= 10   # destinations that are no positive's and are never drawn
    rows = c["g_dst"].cpu()[untouched]
    assert bool((rows == 0).all()) and not bool(torch.signbit(rows).any())
    if window:   # the gradient reaches the windows and nothing else
        gs, gd = c["full"]
        assert bool((gs[:, 0] == 0).all()) and bool((gs[:, F + 1:] == 0).all()) and bool((gd[:, :3] == 0).all())


@pytest.mark.parametrize("E,F,k,tag", [(32919, 256, 3, "k_link_fwd<4,64,ONE,RANK>"),
                                       (600001, 8, 1, "k_link_fwd<4,2,ONE,RANK>")])
def test_scale_ranks_exact_on_integer_embeddings(E, F, k, tag):
    """Embeddings in {-2..2}: every score is an exact fp32 integer in any order, so the counts of the RANK epilogue
    are exact in every pass of the grid."""
    from hgin import _lib
    from hgin.linkpred import link_ranks
    from oracle import c_oracle
    off = 6
    pos, zs, zd = _inputs(E, N_SRC, N_DST, F, seed=E + F + 1, integer=True)
    head, blocks = _fwd_plan(E, F, vec=True)
    assert tag == head + ",RANK>" and blocks > MAX_GRID
    nd = c_oracle.neg_sample(SEED, off, E * k, N_DST).astype(np.int64)
    zsn, zdn = zs.numpy().astype(np.int32), zd.numpy().astype(np.int32)
    src, dst = pos[0].numpy(), pos[1].numpy()
    s_pos = np.einsum("ef,ef->e", zsn[src], zdn[dst])
    s_neg = np.einsum("ef,ef->e", zsn[np.repeat(src, k)], zdn[nd])
    want_gt, want_eq = ref_ranks(s_pos, s_neg, k)
    assert int(want_eq.sum()) > 0 and int(want_gt.sum()) > 0
    with _lib.trace_launches() as tr:
        gt, eq = link_ranks(zs.to(DEV), zd.to(DEV), pos.to(DEV), k, SEED, off)
    assert [t for t in tr.kernels if t.startswith("k_link")] == [tag]
    gt, eq = gt.cpu().numpy(), eq.cpu().numpy()
    for name, a, b in (("n_greater", gt, want_gt), ("n_equal", eq, want_eq)):
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, (name, bad.size, bad[:5].tolist(), a[bad[:5]].tolist(), b[bad[:5]].tolist())


# ---------------------------------------------------------------------------------------------------
# hub rows in the backward
# ---------------------------------------------------------------------------------------------------
def _row_ratio(got_row, ref_row):
    d = float((got_row.detach().cpu().double() - ref_row.double()).norm())
    n = float(ref_row.double().norm())
    return d, n


@pytest.mark.parametrize("side", ["source", "destination"])
def test_hub_row_gradient_by_its_own_norm(side):
    """All 4000 positives leave source 0 (enter destination 0): that row is a weighted sum of 24000 (4000 and the
    draws that hit it) largely cancelling items.  It is held to the project's bound by its own norm,
    ||d|| <= 1e-5 ||row|| + 1e-9: in the whole-matrix norm of ``_check`` a single small row can hide.  Not compared
    with ``link_loss``, whose decoder backward is pinned bit for bit to a plain sequential fp32 sum.
    Measured on an MI355X with a plain fp32 running sum on the source side: 2.18e-5 (the bound is missed); with the
    compensated sum both sides use now: see DESIGN.md §0.1."""
    from oracle import c_oracle
    n_src, n_dst, F, k, E, off = 37, 53, 128, 5, 4000, 6
    g = torch.Generator().manual_seed(4000 + (side == "source"))
    if side == "source":
        pos = torch.stack([torch.zeros(E, dtype=torch.long), torch.randint(0, n_dst - n_dst // 5, (E,), generator=g)])
    else:
        pos = torch.stack([torch.randint(0, 30, (E,), generator=g), torch.zeros(E, dtype=torch.long)])
    zs, zd = torch.randn(n_src, F, generator=g) * 0.5, torch.randn(n_dst, F, generator=g) * 0.5
    loss, g_src, g_dst, _ = _run_fused(zs.to(DEV), zd.to(DEV), pos.to(DEV), k, off)
    ref = ref_loss_and_grads(zs, zd, pos, c_oracle.neg_sample(SEED, off, E * k, n_dst), k)
    got_row, ref_row = (g_src[0], ref[1][0]) if side == "source" else (g_dst[0], ref[2][0])
    d, n = _row_ratio(got_row, ref_row)
    print(f"hub {side} row: ||d|| / ||row|| {d / n:.3g} (||row|| {n:.3g})")
    _check(loss, g_src, g_dst, ref, f"hub {side}: fused vs float64")
    assert d <= 1e-5 * n + 1e-9, (side, d / n)
    rest = g_src.cpu()[1:] if side == "source" else g_src.cpu()[30:]
    assert bool((rest == 0).all()) and not bool(torch.signbit(rest).any())   # rows without a positive: exactly +0


# ---------------------------------------------------------------------------------------------------
# saturated and degenerate scores
# ---------------------------------------------------------------------------------------------------
def test_saturated_and_zero_scores_coefficient_by_coefficient():
    """Integer-valued embeddings whose scores are exactly 0 (zero source rows), +-30 and +-200 (fp32 exp(-200)
    underflows to 0).  Every saved coefficient (``[E positives | E k negatives]``) against float64 within 1e-6
    relative + 1e-12; an entry that is exactly zero must be one whose float64 sigmoid is below the smallest normal
    fp32, and carries the sign of the float64 value; loss and gradients within the file's bounds."""
    from hgin.linkpred import sampled_link_loss
    from oracle import c_oracle
    E, n_dst, k, F, off, n_src = 64, 8, 3, 8, 6, 12
    g = torch.Generator().manual_seed(64)
    pos = torch.stack([torch.randint(0, n_src, (E,), generator=g), torch.randint(0, n_dst, (E,), generator=g)])
    zs, zd = torch.zeros(n_src, F), torch.zeros(n_dst, F)
    zs[4:8, 0], zs[8:12, 1] = 5.0, 10.0               # rows 0..3 zero: s = 0; 4..7: s = +-30; 8..11: s = +-200
    zd[0::2, 0], zd[0::2, 1], zd[1::2, 0], zd[1::2, 1] = 6.0, 20.0, -6.0, -20.0
    zd[:, 2:] = torch.randint(-2, 3, (n_dst, F - 2), generator=g).float()   # meets zeros of z_src only
    nd = c_oracle.neg_sample(SEED, off, E * k, n_dst).astype(np.int64)
    zs64, zd64 = zs.double().numpy(), zd.double().numpy()
    src, dst = pos[0].numpy(), pos[1].numpy()
    s = np.concatenate([(zs64[src] * zd64[dst]).sum(1), (zs64[np.repeat(src, k)] * zd64[nd]).sum(1)])
    is_pos = np.arange(E * (1 + k)) < E
    for want in (0.0, 30.0, -30.0, 200.0, -200.0):     # every score occurs on a positive and on a negative
        assert int(((s == want) & is_pos).sum()) >= 1 and int(((s == want) & ~is_pos).sum()) >= 1, want
    assert set(np.unique(s).tolist()) == {0.0, 30.0, -30.0, 200.0, -200.0}
    w = np.where(is_pos, 0.5 / E, 0.5 / (E * k))
    sig = np.where(is_pos, -1.0 / (1.0 + np.exp(s)), 1.0 / (1.0 + np.exp(-s)))   # sigmoid(s) - label, no cancellation
    want_coef = w * sig
    softplus = lambda x: np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))  # noqa: E731
    want_loss = float((w * softplus(np.where(is_pos, -s, s))).sum())

    a, b = zs.to(DEV).requires_grad_(True), zd.to(DEV).requires_grad_(True)
    loss = sampled_link_loss(a, b, pos.to(DEV), k, SEED, off)
    coef = loss.grad_fn.saved_tensors[0].detach().cpu()
    loss.backward()
    assert coef.dtype == torch.float32 and tuple(coef.shape) == (E * (1 + k),)
    got = coef.double().numpy()
    err = np.abs(got - want_coef)
    print(f"saturated scores: |dloss|/|loss| {abs(float(loss) - want_loss) / want_loss:.3g}  "
          f"max coefficient error / (1e-6 |c| + 1e-12) {float((err / (1e-6 * np.abs(want_coef) + 1e-12)).max()):.3g}")
    bad = np.nonzero(err > 1e-6 * np.abs(want_coef) + 1e-12)[0]
    assert bad.size == 0, (bad[:5].tolist(), s[bad[:5]].tolist(), got[bad[:5]].tolist(), want_coef[bad[:5]].tolist())
    assert np.array_equal(np.signbit(coef.numpy()), want_coef < 0), "a coefficient (or a zero) of the wrong sign"
    zero = got == 0
    smallest_normal = float(np.finfo(np.float32).tiny)
    assert bool((np.abs(want_coef[zero]) / w[zero] < smallest_normal).all())
    # exp(-|s|) underflows exactly where the sigmoid leaves the label's side: +200 positives, -200 negatives
    assert np.array_equal(zero, np.where(is_pos, s == 200.0, s == -200.0))
    half = s == 0.0                                   # s = 0: the coefficient is -+ w / 2 to the last bit
    assert np.array_equal(coef.numpy()[half], (np.where(is_pos, -0.5, 0.5) * w.astype(np.float32))[half])
    full = np.where(is_pos, s == -200.0, s == 200.0)  # the saturated side: -w / +w
    assert np.array_equal(coef.numpy()[full], (np.where(is_pos, -1.0, 1.0) * w.astype(np.float32))[full])
    assert abs(float(loss) - want_loss) <= 1e-5 * abs(want_loss), (float(loss), want_loss)
    assert math.isfinite(float(loss))
    # The gradients, in float64 from the float64 coefficients: g_src[s] = sum c z_dst[d], g_dst[d] = sum c z_src[s].
    # (Not through autograd of ref_loss: max(x, 0) + log1p(exp(-|x|)) has a kink at the exact zeros scored here,
    # where autograd picks a one-sided derivative instead of sigmoid(0) = 1 / 2.)
    all_src, all_dst = np.concatenate([src, np.repeat(src, k)]), np.concatenate([dst, nd])
    want_gs, want_gd = np.zeros((n_src, F)), np.zeros((n_dst, F))
    np.add.at(want_gs, all_src, want_coef[:, None] * zd64[all_dst])
    np.add.at(want_gd, all_dst, want_coef[:, None] * zs64[all_src])
    assert abs(float(ref_loss_and_grads(zs, zd, pos, nd, k)[0]) - want_loss) <= 1e-12 * want_loss
    _check(loss.detach(), a.grad, b.grad, (torch.tensor(want_loss, dtype=torch.float64), torch.from_numpy(want_gs),
                                           torch.from_numpy(want_gd)), "saturated scores: fused vs float64")
