"""The softmax, BPR and self-adversarial objectives of the fused link loss on the GPU (include/hgin.h A17).

Negatives: bit for bit the C oracle's sampler and the ``"bce"`` run's.  Loss and gradients: against this suite's
float64 CPU reference (tests/test_linkobj_host.py) built from the oracle's negatives, and against the unfused
``link_loss(..., objective=...)`` on the GPU, within tests/test_gpu_linkpred.py::_check's bounds (reused, not
re-chosen): |d loss| <= 1e-5 |loss|, ||d g|| <= 1e-5 ||g_ref|| + 1e-9.  Determinism: bitwise.

fp32 restatement.  ``test_fp32_restatement_stays_inside_the_band`` evaluates the reference expression itself in
float32 on the CPU (pair by pair, torch's own summation order) at every shape of the grid and at the large-score
shapes, and holds it to the same band, so the band is known to be reachable in single precision.  Observed over the
grid (E = 211, embeddings randn * 0.5), worst case per objective of |d loss| / |loss|, ||d g_src|| / ||g||,
||d g_dst|| / ||g||: softmax 8.8e-8, 3.1e-7, 4.7e-7; bpr 1.2e-7, 2.2e-7, 5.3e-7; selfadv 1.5e-7, 5.4e-7, 1.3e-6: a
margin of 7x or more under 1e-5.  At the large-score shapes (F = 256, embeddings x 8, scores in the hundreds; torch's
summation order, hence the figure, varies with the host's thread count): loss 1.1e-7 at worst, gradients up to 1.8e-6
(softmax), 7.2e-6 (softmax at temperature 0.25, where a pair's probability carries the fp32 error of an argument near
1000), 1.1e-6 (bpr), 3.6e-6 (selfadv): still inside.  The kernels themselves, on an MI355X: 3.4e-7 at worst over the
grid, 1.5e-6 at the large-score shapes (softmax at temperature 0.25).

One exception, measured and not widened silently.  For softmax and bpr at n_dst = 1 all k + 1 pairs of a positive are
the same two rows, its coefficients sum to zero, and the true gradient is identically zero (||g_ref|| ~ 1e-16 in
float64), so 1e-5 ||g_ref|| + 1e-9 leaves 1e-9 absolute for a sum of E (k + 1) individually rounded products of size
0.5 / E * |z|.  The fp32 restatement misses that: over the grid's n_dst = 1 cases its gradients are up to 1.5e-6
(softmax; F = 8, k = 5, temperature 0.25) and 9.1e-7 (bpr; F = 260, k = 3) from zero.  Following the issue, those
cases hold the gradients to 4 x that measured distance as an absolute bound (``ZERO_GRADIENT_FLOOR``; a dropped or
doubled pair would show as about 2e-3 sqrt(F)); their loss, and everything at every other shape, stays in the band.
(The kernels' own gradients at those cases measured at most 5.6e-8 from zero: their compensated sums and the exactly
cancelling stored coefficients do better than the restatement.)

Sums of coefficients.  The kernels form a positive's coefficient for softmax and bpr as minus the sum of its
negatives' stored coefficients (at most k - 1 rounded additions of partial sums no larger than 1 / (tau E), resp.
k / (E k) = 1 / E), so in float64 the stored floats of one positive sum to zero within (k - 1) / 2 ulps of that scale;
the test holds them to the issue's (k + 1) ulps of 1 / (tau E) (bpr: tau = 1).

Model level: five ``link_train_step``s against the CPU replica (oracle convs + the float64 objective + the oracle's
negatives + torch's Adam), with the bounds of the existing bce test."""
import functools
import math

import numpy as np
import pytest
import torch

from test_gpu_linkpred import E, N_SRC, REL_PL, SEED, _check, _gin_pair, _inputs, _oracle_encode
from test_linkobj_host import ref_obj_loss, ref_obj_loss_and_grads

DEV = "cuda"
pytestmark = pytest.mark.gpu

FS = (2, 4, 6, 8, 128, 70, 260)   # G = 2 / G = 1 writer forms, scalar G = 8, float4 in registers, the looped forms
KS = (1, 3, 4, 5, 9)              # one short batch, one full batch, a second batch of one / two pairs, three batches
N_DSTS = (1, 5, 53)
OFFS = (0, 2**32 + 1)
PARAMS = {"softmax": (1.0, 0.25), "bpr": (0.0,), "selfadv": (0.0, 1.0, 4.0)}


def _grid():
    """Every F form with two k each (so every k at least once, in fact at least twice) per objective, n_dst / offset /
    parameter cycling at different periods, then every parameter value at a second batch of two pairs and at three
    batches on the widest register form: 54 cases."""
    cases = []
    for obj, params in PARAMS.items():
        j = 0
        for i, F in enumerate(FS):
            for k in (KS[i % 5], KS[(i + 2) % 5]):
                cases.append((obj, params[(j // 2) % len(params)], N_DSTS[j % 3], k, OFFS[(j // 3) % 2], F))
                j += 1
        for param in params:
            for k, n_dst, off in ((5, 53, 2**32 + 1), (9, 5, 0)):
                case = (obj, param, n_dst, k, off, 128)
                if case not in cases:
                    cases.append(case)
    return cases


CASES = _grid()
# the persistent loop's second trip (more than kLinkMaxGrid * 4 waves of two positives at G = 32) and a single positive
BIG = [(obj, PARAMS[obj][-1], 53, 5, 6, 128, 70_001) for obj in PARAMS]
# (with one positive the loss is that positive's term alone, and the relative bound on it needs a term fp32 can
# resolve: at the default parameters these are 0.059 / 0.012 / 0.55, while at temperature 0.25 this positive's is
# log1p(5.9e-7), which the fp32 restatement, and link_loss with it, returns as 0)
ONE = [("softmax", 1.0, 53, 5, 6, 128, 1), ("bpr", 0.0, 53, 5, 6, 128, 1), ("selfadv", 1.0, 53, 5, 6, 128, 1)]
LARGE = [("softmax", 1.0), ("softmax", 0.25), ("bpr", 0.0), ("selfadv", 1.0), ("selfadv", 4.0)]


def test_the_grid_covers_every_form_and_every_k_per_objective():
    assert 50 <= len(CASES) <= 60 and len(set(CASES)) == len(CASES)
    for obj, params in PARAMS.items():
        mine = [c for c in CASES if c[0] == obj]
        assert {c[5] for c in mine} == set(FS) and {c[3] for c in mine} == set(KS)
        assert {c[1] for c in mine} == set(params) and {c[2] for c in mine} == set(N_DSTS)
        assert {c[4] for c in mine} == set(OFFS)


def _inputs_e(n_dst, F, n_edges, scale=1.0):
    """``_inputs`` of tests/test_gpu_linkpred.py at another number of positives (same tables, same ranges)."""
    if n_edges == E and scale == 1.0:
        return _inputs(n_dst, F)
    g = torch.Generator().manual_seed(1000 * n_dst + F + n_edges)
    pos = torch.stack([torch.randint(0, 30, (n_edges,), generator=g),
                       torch.randint(0, n_dst - n_dst // 5, (n_edges,), generator=g)])
    zs = torch.randn(N_SRC, F, generator=g) * 0.5 * scale
    zd = torch.randn(n_dst, F, generator=g) * 0.5 * scale
    return pos, zs, zd


def _run(zs, zd, pos, k, off, objective, param):
    """(loss, g_src, g_dst, negatives, coefficients) of one fused forward + backward on the device."""
    from hgin.linkpred import _SampledLinkLossFn, sampled_link_loss
    a, b = zs.detach().clone().requires_grad_(True), zd.detach().clone().requires_grad_(True)
    kw = {"softmax": dict(temperature=param), "selfadv": dict(alpha=param)}.get(objective, {})
    loss = sampled_link_loss(a, b, pos, k, SEED, off, objective=objective, **kw)
    assert isinstance(loss.grad_fn, _SampledLinkLossFn._backward_cls)
    coef, neg, sa, sb = loss.grad_fn.saved_tensors   # nothing else is saved, for any objective
    assert tuple(coef.shape) == (pos.size(1) * (1 + k),) and sa.data_ptr() == a.data_ptr() and sb.data_ptr() == b.data_ptr()
    loss.backward()
    return loss.detach(), a.grad, b.grad, neg, coef


@functools.lru_cache(maxsize=None)
def _case(objective, param, n_dst, k, off, F, n_edges=E, scale=1.0):
    from oracle import c_oracle
    pos, zs, zd = _inputs_e(n_dst, F, n_edges, scale)
    posd, zsd, zdd = pos.to(DEV), zs.to(DEV), zd.to(DEV)
    loss, g_src, g_dst, neg, coef = _run(zsd, zdd, posd, k, off, objective, param)
    want_neg = c_oracle.neg_sample(SEED, off, n_edges * k, n_dst)
    ref = ref_obj_loss_and_grads(zs, zd, pos, want_neg, k, objective, param)
    return dict(pos=pos, posd=posd, zs=zs, zd=zd, zsd=zsd, zdd=zdd, loss=loss, g_src=g_src, g_dst=g_dst, neg=neg,
                coef=coef, want_neg=want_neg, ref=ref)


# softmax and bpr at n_dst = 1: ||g_ref|| = 0, see the module docstring; 4 x the fp32 restatement's measured distance
ZERO_GRADIENT_FLOOR = {"softmax": 4 * 1.5e-6, "bpr": 4 * 9.1e-7}


def _check_band(loss, g_src, g_dst, ref, what, objective, n_dst):
    """``_check`` of tests/test_gpu_linkpred.py; where the true gradient is identically zero (module docstring) the
    loss is held to the same 1e-5 and the gradients to the measured absolute floor."""
    if n_dst != 1 or objective not in ZERO_GRADIENT_FLOOR:
        return _check(loss, g_src, g_dst, ref, what)
    rl, rs, rd = ref
    floor = ZERO_GRADIENT_FLOOR[objective]
    assert float(rs.double().norm()) <= floor and float(rd.double().norm()) <= floor   # zero, to the reference's rounding
    dl = abs(float(loss) - float(rl))
    ds, dd = float(g_src.detach().cpu().double().norm()), float(g_dst.detach().cpu().double().norm())   # from zero
    print(f"{what}: |dloss|/|loss| {dl / abs(float(rl)):.3g}  ||g_src|| {ds:.3g}  ||g_dst|| {dd:.3g} (true gradient 0)")
    assert dl <= 1e-5 * abs(float(rl)), (what, dl, float(rl))
    assert ds <= floor and dd <= floor, (what, ds, dd)


def _link_loss(c, k, off, objective, param):
    from hgin.linkpred import link_loss
    a, b = c["zsd"].clone().requires_grad_(True), c["zdd"].clone().requires_grad_(True)
    base = link_loss(a, b, c["posd"], k, SEED, off, objective=objective, temperature=param or 1.0, alpha=param)
    base.backward()
    return base.detach().cpu(), a.grad.cpu(), b.grad.cpu()


def _bce_negatives(c, k, off):
    from hgin.linkpred import sampled_link_loss
    with torch.enable_grad():
        loss = sampled_link_loss(c["zsd"].clone().requires_grad_(True), c["zdd"], c["posd"], k, SEED, off,
                                 objective="bce")
    return loss.grad_fn.saved_tensors[1]


def _check_negatives(c, k, off, n_edges):
    neg = c["neg"].cpu()
    assert neg.dtype == torch.int64 and tuple(neg.shape) == (2, n_edges * k)
    assert np.array_equal(neg[1].numpy(), c["want_neg"].astype(np.int64))
    assert torch.equal(neg[0], c["pos"][0].repeat_interleave(k))
    assert torch.equal(_bce_negatives(c, k, off), c["neg"])


def _check_zero_rows(c, n_dst):
    no_pos = torch.ones(N_SRC, dtype=torch.bool)
    no_pos[c["pos"][0]] = False
    assert int(no_pos.sum()) >= 7
    rows = c["g_src"].cpu()[no_pos]
    assert rows.numel() and bool((rows == 0).all()) and not bool(torch.signbit(rows).any())
    untouched = torch.ones(n_dst, dtype=torch.bool)
    untouched[c["pos"][1]] = False
    untouched[torch.as_tensor(c["want_neg"].astype(np.int64))] = False
    rows = c["g_dst"].cpu()[untouched]
    assert bool((rows == 0).all()) and not bool(torch.signbit(rows).any())


@pytest.mark.parametrize("objective,param,n_dst,k,off,F", CASES)
def test_negatives_are_the_oracle_samplers_and_the_bce_runs(objective, param, n_dst, k, off, F):
    _check_negatives(_case(objective, param, n_dst, k, off, F), k, off, E)


@pytest.mark.parametrize("objective,param,n_dst,k,off,F", CASES)
def test_loss_and_gradients_vs_float64_reference_and_link_loss(objective, param, n_dst, k, off, F):
    c = _case(objective, param, n_dst, k, off, F)
    assert c["loss"].dim() == 0 and c["loss"].dtype == torch.float32
    _check_band(c["loss"], c["g_src"], c["g_dst"], c["ref"], f"fused {objective} vs float64", objective, n_dst)
    _check_band(c["loss"], c["g_src"], c["g_dst"], _link_loss(c, k, off, objective, param),
                f"fused {objective} vs link_loss", objective, n_dst)


@pytest.mark.parametrize("objective,param,n_dst,k,off,F", CASES)
def test_fp32_restatement_stays_inside_the_band(objective, param, n_dst, k, off, F):
    """No device: the reference expression in float32 on the CPU against itself in float64 (module docstring)."""
    from oracle import c_oracle
    pos, zs, zd = _inputs(n_dst, F)
    nd = c_oracle.neg_sample(SEED, off, E * k, n_dst)
    l32, s32, d32 = ref_obj_loss_and_grads(zs, zd, pos, nd, k, objective, param, dtype=torch.float32)
    _check_band(l32, s32, d32, ref_obj_loss_and_grads(zs, zd, pos, nd, k, objective, param),
                f"fp32 {objective} vs float64", objective, n_dst)


@pytest.mark.parametrize("objective,param,n_dst,k,off,F", CASES)
def test_bitwise_determinism_and_exact_zero_rows(objective, param, n_dst, k, off, F):
    c = _case(objective, param, n_dst, k, off, F)
    loss, g_src, g_dst, neg, coef = _run(c["zsd"], c["zdd"], c["posd"], k, off, objective, param)
    assert torch.equal(loss, c["loss"]) and torch.equal(g_src, c["g_src"]) and torch.equal(g_dst, c["g_dst"])
    assert torch.equal(neg, c["neg"]) and torch.equal(coef, c["coef"])
    _check_zero_rows(c, n_dst)


@pytest.mark.parametrize("objective,param,n_dst,k,off,F,n_edges", BIG + ONE)
def test_second_trip_of_the_persistent_loop_and_a_single_positive(objective, param, n_dst, k, off, F, n_edges):
    """E = 70 001 at G = 32: 35 001 waves of two positives over 4096 * 4 resident ones, so every wave takes a second
    or third trip and the last wave has an idle group; E = 1: one group works, every other one idles."""
    c = _case(objective, param, n_dst, k, off, F, n_edges)
    _check_negatives(c, k, off, n_edges)
    _check(c["loss"], c["g_src"], c["g_dst"], c["ref"], f"E = {n_edges} {objective} vs float64")
    _check(c["loss"], c["g_src"], c["g_dst"], _link_loss(c, k, off, objective, param),
           f"E = {n_edges} {objective} vs link_loss")
    loss, g_src, g_dst, neg, coef = _run(c["zsd"], c["zdd"], c["posd"], k, off, objective, param)
    assert torch.equal(loss, c["loss"]) and torch.equal(g_src, c["g_src"]) and torch.equal(g_dst, c["g_dst"])
    assert torch.equal(coef, c["coef"])


@pytest.mark.parametrize("objective,param", LARGE)
def test_large_scores_stay_finite_and_inside_the_band(objective, param):
    """Embeddings x 8 at F = 256: scores of a few hundred (softmax arguments past a thousand at temperature 0.25),
    where exp(s) or exp(s / tau) overflows fp32 unless the maximum is subtracted first."""
    from oracle import c_oracle
    n_dst, k, off, F = 53, 5, 6, 256
    c = _case(objective, param, n_dst, k, off, F, E, 8.0)
    s = (c["zs"].double() @ c["zd"].double().t()).abs().max()
    assert float(s) > 300.0
    for t in (c["loss"], c["g_src"], c["g_dst"], c["coef"]):
        assert bool(torch.isfinite(t).all())
    _check(c["loss"], c["g_src"], c["g_dst"], c["ref"], f"large scores {objective} vs float64")
    _check(c["loss"], c["g_src"], c["g_dst"], _link_loss(c, k, off, objective, param),
           f"large scores {objective} vs link_loss")
    nd = c_oracle.neg_sample(SEED, off, E * k, n_dst)
    l32, s32, d32 = ref_obj_loss_and_grads(c["zs"], c["zd"], c["pos"], nd, k, objective, param, dtype=torch.float32)
    _check(l32, s32, d32, c["ref"], f"large scores fp32 {objective} vs float64")


@pytest.mark.parametrize("k,F", [(1, 8), (3, 128), (4, 2), (5, 70), (9, 6)])
def test_closed_forms_at_one_destination(k, F):
    """n_dst = 1: every score of a positive is one number, bit for bit: softmax = log(k + 1) at any temperature,
    bpr = log 2, and selfadv at alpha = 0 is bce, all to 1e-6."""
    from hgin.linkpred import sampled_link_loss
    pos, zs, zd = _inputs(1, F)
    posd, zsd, zdd = pos.to(DEV), zs.to(DEV), zd.to(DEV)
    for tau in (1.0, 0.25):
        got = float(sampled_link_loss(zsd, zdd, posd, k, SEED, 6, objective="softmax", temperature=tau))
        assert abs(got - math.log(k + 1)) <= 1e-6, (tau, got)
    got = float(sampled_link_loss(zsd, zdd, posd, k, SEED, 6, objective="bpr"))
    assert abs(got - math.log(2.0)) <= 1e-6, got
    got = float(sampled_link_loss(zsd, zdd, posd, k, SEED, 6, objective="selfadv", alpha=0.0))
    want = float(sampled_link_loss(zsd, zdd, posd, k, SEED, 6))
    assert abs(got - want) <= 1e-6, (got, want)


@pytest.mark.parametrize("n_dst,k,off,F", [(53, 1, 0, 8), (5, 4, 2**32 + 1, 128), (53, 5, 6, 70), (53, 9, 0, 4)])
def test_selfadv_at_alpha_zero_is_bce(n_dst, k, off, F):
    c = _case("selfadv", 0.0, n_dst, k, off, F)
    bce = _run(c["zsd"], c["zdd"], c["posd"], k, off, "bce", 0.0)
    _check(c["loss"], c["g_src"], c["g_dst"], (bce[0].cpu(), bce[1].cpu(), bce[2].cpu()), "selfadv(alpha = 0) vs bce")


@pytest.mark.parametrize("objective,param,n_dst,k,off,F",
                         [c for c in CASES if c[0] in ("softmax", "bpr")] + [("softmax", 0.25, 53, 5, 6, 256)])
def test_a_positives_coefficients_sum_to_zero(objective, param, n_dst, k, off, F):
    c = _case(objective, param, n_dst, k, off, F)
    coef = c["coef"].cpu().double()
    total = coef[:E] + coef[E:].reshape(E, k).sum(1)
    tau = param if objective == "softmax" else 1.0
    band = (k + 1) * float(np.spacing(np.float32(1.0 / (tau * E))))
    worst = float(total.abs().max())
    print(f"{objective}: worst |sum of a positive's coefficients| {worst:.3g}, band {band:.3g}")
    assert worst <= band
    assert bool((coef[:E] <= 0).all()) and bool((coef[E:] >= 0).all())


@pytest.mark.parametrize("n_dst,k,off,F", [(53, 3, 6, 128), (5, 5, 2**32 + 1, 70), (53, 4, 0, 2)])
def test_the_default_path_is_untouched(n_dst, k, off, F):
    """objective="bce" and no argument at all: one path, bitwise, and still hgin_link_loss_fwd_f32's kernel."""
    from hgin import _lib
    from hgin.linkpred import sampled_link_loss
    pos, zs, zd = _inputs(n_dst, F)
    posd = pos.to(DEV)
    a, b = zs.to(DEV).requires_grad_(True), zd.to(DEV).requires_grad_(True)
    sampled_link_loss(a, b, posd, k, SEED, off).backward()
    explicit = _run(zs.to(DEV), zd.to(DEV), posd, k, off, "bce", 0.0)
    with _lib.trace_launches() as tr:
        default = sampled_link_loss(a, b, posd, k, SEED, off)
    assert [t.rsplit(",", 1)[1] for t in tr.kernels if t.startswith("k_link_fwd")] == ["LOSS>"]
    assert torch.equal(default.detach(), explicit[0])
    assert torch.equal(a.grad, explicit[1]) and torch.equal(b.grad, explicit[2])


def test_launch_tags():
    from hgin import _lib
    for objective, tag in (("softmax", "SOFTMAX"), ("bpr", "BPR"), ("selfadv", "SELFADV")):
        c = _case(objective, PARAMS[objective][-1], 53, 5, 2**32 + 1, 128)
        with _lib.trace_launches() as tr:
            _run(c["zsd"], c["zdd"], c["posd"], 5, 2**32 + 1, objective, PARAMS[objective][-1])
        assert f"k_link_fwd<4,32,ONE,{tag}>" in tr.kernels and "k_link_loss_sum" in tr.kernels
        assert "k_link_bwd_src<4,32>" in tr.kernels and "k_link_bwd_dst<4,32>" in tr.kernels


@pytest.mark.parametrize("objective,param,F,k", [("softmax", 0.25, 70, 5), ("bpr", 0.0, 8, 3), ("selfadv", 4.0, 128, 4)])
def test_non_contiguous_odd_stride_views(objective, param, F, k):
    """Embeddings that are column windows of wider buffers (row stride odd, start not 16-byte aligned): the scalar
    path; the gradient reaches the window and nothing else."""
    from hgin.linkpred import sampled_link_loss
    from oracle import c_oracle
    n_dst, off = 53, 6
    pos, zs, zd = _inputs(n_dst, F)
    g = torch.Generator().manual_seed(5)
    bs = torch.randn(N_SRC, 2 * F + 1, generator=g)
    bd = torch.randn(n_dst, F + 3, generator=g)
    bs[:, 1:F + 1], bd[:, 3:] = zs, zd
    bs, bd = bs.to(DEV).requires_grad_(True), bd.to(DEV).requires_grad_(True)
    vs, vd = bs[:, 1:F + 1], bd[:, 3:]
    assert not vs.is_contiguous() and vs.stride(0) % 2 == 1 and vd.stride(0) % 2 == 1
    loss = sampled_link_loss(vs, vd, pos.to(DEV), k, SEED, off, objective=objective, temperature=param or 1.0,
                             alpha=param)
    loss.backward()
    ref = ref_obj_loss_and_grads(zs, zd, pos, c_oracle.neg_sample(SEED, off, E * k, n_dst), k, objective, param)
    _check(loss.detach(), bs.grad[:, 1:F + 1], bd.grad[:, 3:], ref, f"strided views {objective} vs float64")
    assert bool((bs.grad[:, 0] == 0).all()) and bool((bs.grad[:, F + 1:] == 0).all())
    assert bool((bd.grad[:, :3] == 0).all())


@pytest.mark.parametrize("objective,param", [("softmax", 0.5), ("selfadv", 1.0)])
def test_five_link_train_steps_follow_the_cpu_replica(objective, param):
    import hgin
    from oracle import c_oracle
    cfg, g, ref, model = _gin_pair()
    gd = g.to(DEV)
    k, seed = 3, 7
    pos = g.edge_index[REL_PL]
    n_e = int(pos.size(1))
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    pred = hgin.LinkPredictor(model, REL_PL, k, seed, objective=objective, temperature=param, alpha=param)
    got = [hgin.link_train_step(model, opt, gd, pred, step=s) for s in range(5)]
    assert all(v.is_cuda and v.dim() == 0 and not v.requires_grad for v in got)
    got = [float(v) for v in got]

    ropt = torch.optim.Adam(ref.parameters(), lr=1e-3)
    want = []
    for s in range(5):
        ropt.zero_grad()
        z = _oracle_encode(ref, g.x_dict(), g.edge_index_dict())
        nd = c_oracle.neg_sample(seed, s * n_e * k, n_e * k, cfg.n_link)
        loss = ref_obj_loss(z["path"].double(), z["link"].double(), pos, nd, k, objective, param)
        loss.backward()
        ropt.step()
        want.append(float(loss.detach()))
    print(f"{objective} link loss trajectory gpu", got, "cpu", want)
    for s, (a, b) in enumerate(zip(got, want)):
        assert abs(a - b) <= 1e-4 * abs(b), (s, a, b)
    assert got[4] < got[0]
