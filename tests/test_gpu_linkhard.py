"""Caller-supplied and mined negatives of the fused link loss on the GPU (include/hgin.h A18).

Pairs: the written negatives are [the C oracle's draws at counters offset + e k + j | the given destinations], bit for
bit.  Substitution: a given destination carries the bits of a drawn one, so (k, G), (0, [draws | G]) and, for G = the
draws themselves, the pre-A18 ``sampled_link_loss(k = K)`` agree bitwise in loss, coefficients, pairs and both
gradients, for every objective, and ``link_ranks`` likewise: that pins the new instantiations to the validated ones.
Loss and gradients: against this suite's float64 CPU reference on the combined negative array and against the unfused
``link_loss(..., neg_dst=)`` on the GPU, within tests/test_gpu_linkpred.py::_check's bounds (reused, not re-chosen):
|d loss| <= 1e-5 |loss|, ||d g|| <= 1e-5 ||g_ref|| + 1e-9.  n_dst = 1 is left out: there the true softmax / bpr gradient
is identically zero and the existing absolute floor was measured for k pairs, not k + m.  Ranks: exact on integer
embeddings.  ``hard_negatives``: against ``ref_topk`` on integer embeddings (exact scores, ties by index), padded slots
exactly where the CPU says and holding the sampler's draws.  Model level: four ``link_train_step``s with mining every
second step, the kept set and every loss reproduced bitwise from the recorded embeddings."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_linkobj import _inputs_e
from test_gpu_linkpred import E, N_SRC, REL_PL, SEED, _check, _gin_pair, _inputs
from test_linkobj_host import ref_obj_loss_and_grads
from test_linkpred_host import ref_metrics, ref_ranks
from test_linktopk_host import ref_topk

DEV = "cuda"
pytestmark = pytest.mark.gpu

# no draws (one / two batches); the boundary inside the first batch; draws filling the first batch with the boundary on
# its edge; draws and given pairs sharing the first batch, the rest in a second; draws spilling into a second batch
# shared with given pairs; three batches
KM = ((0, 1), (0, 5), (1, 5), (3, 1), (3, 4), (4, 3), (2, 9))
FS = (2, 6, 8, 128, 260)          # the single-writer forms (G = 2, G = 8 scalar), float4 in registers, looped
N_DSTS = (5, 53)
OFFS = (0, 2**32 + 1)
OBJECTIVES = ("bce", "softmax", "bpr", "selfadv")
PARAMS = {"bce": (0.0, 0.0), "softmax": (1.0, 0.25), "bpr": (0.0, 0.0), "selfadv": (1.0, 4.0)}


def _grid():
    """Every (k, m) with every objective; F, n_dst, offset, parameter and the set's dtype cycle at other periods, so
    every F meets at least five different (k, m): 28 cases."""
    cases = []
    for i, obj in enumerate(OBJECTIVES):
        for j, (k, m) in enumerate(KM):
            cases.append((obj, PARAMS[obj][j % 2], N_DSTS[(i + j) % 2], k, m, OFFS[(j // 2 + i) % 2], FS[(i + j) % 5]))
    return cases


CASES = _grid()
RANK_CASES = [(N_DSTS[j % 2], k, m, OFFS[(j // 2) % 2], (6, 8, 64, 128, 260)[j % 5]) for j, (k, m) in enumerate(KM)]


def test_the_grid_covers_what_it_says():
    assert len(CASES) == 28 and len(set(CASES)) == 28
    for obj in OBJECTIVES:
        assert {(c[3], c[4]) for c in CASES if c[0] == obj} == set(KM)
    for F in FS:
        assert len({(c[3], c[4]) for c in CASES if c[6] == F}) >= 2
    assert {c[2] for c in CASES} == set(N_DSTS) and {c[5] for c in CASES} == set(OFFS)
    assert {(c[1], c[2]) for c in RANK_CASES} == set(KM)


def _given(pos, n_dst, m, seed=0):
    """int64 [E, m]: random destinations in range; every seventh positive meets its own destination in slot 0."""
    g = torch.Generator().manual_seed(77 + 1000 * n_dst + m + seed)
    G = torch.randint(0, n_dst, (pos.size(1), m), generator=g)
    G[::7, 0] = pos[1, ::7]
    return G


def _kw(objective, param):
    extra = {"softmax": dict(temperature=param), "selfadv": dict(alpha=param)}.get(objective, {})
    return dict(objective=objective, **extra)


def _run(zs, zd, pos, k, off, objective, param, neg_dst):
    """(loss, g_src, g_dst, negatives, coefficients) of one fused forward + backward on the device."""
    from hgin.linkpred import _SampledLinkLossFn, sampled_link_loss
    a, b = zs.detach().clone().requires_grad_(True), zd.detach().clone().requires_grad_(True)
    kw = _kw(objective, param)
    if neg_dst is not None:
        kw["neg_dst"] = neg_dst
    loss = sampled_link_loss(a, b, pos, k, SEED, off, **kw)
    assert isinstance(loss.grad_fn, _SampledLinkLossFn._backward_cls)
    K = k + (0 if neg_dst is None else int(neg_dst.size(1)))
    saved = loss.grad_fn.saved_tensors
    assert len(saved) == 4                                  # exactly coef, neg, z_src, z_dst
    coef, neg, sa, sb = saved
    assert tuple(coef.shape) == (pos.size(1) * (1 + K),) and tuple(neg.shape) == (2, pos.size(1) * K)
    assert sa.data_ptr() == a.data_ptr() and sb.data_ptr() == b.data_ptr()
    loss.backward()
    return loss.detach(), a.grad, b.grad, neg, coef


def _same(x, y):
    return all(torch.equal(a, b) for a, b in zip(x, y))


@functools.lru_cache(maxsize=None)
def _case(objective, param, n_dst, k, m, off, F, n_edges=E):
    from oracle import c_oracle
    pos, zs, zd = _inputs_e(n_dst, F, n_edges)
    G = _given(pos, n_dst, m)
    posd, zsd, zdd = pos.to(DEV), zs.to(DEV), zd.to(DEV)
    # the set goes in as int64 or as int32 (the latter is handed to the kernel as it is)
    Gd = G.to(DEV) if (k + m) % 2 else G.to(DEV, torch.int32)
    out = _run(zsd, zdd, posd, k, off, objective, param, Gd)
    U = torch.as_tensor(c_oracle.neg_sample(SEED, off, n_edges * k, n_dst).astype(np.int64)).reshape(n_edges, k)
    combined = torch.cat([U, G], 1)
    ref = ref_obj_loss_and_grads(zs, zd, pos, combined.reshape(-1).numpy(), k + m, objective, param)
    return dict(pos=pos, posd=posd, zs=zs, zd=zd, zsd=zsd, zdd=zdd, G=G, Gd=Gd, U=U, combined=combined, out=out,
                ref=ref)


@pytest.mark.parametrize("objective,param,n_dst,k,m,off,F", CASES)
def test_pairs_are_the_oracles_draws_then_the_given_ones(objective, param, n_dst, k, m, off, F):
    from hgin.linkpred import negative_edges
    c = _case(objective, param, n_dst, k, m, off, F)
    neg = c["out"][3].cpu()
    assert neg.dtype == torch.int64 and tuple(neg.shape) == (2, E * (k + m))
    assert torch.equal(neg[1].reshape(E, k + m), c["combined"])
    assert torch.equal(neg[0], c["pos"][0].repeat_interleave(k + m))
    assert int((c["G"][:, 0] == c["pos"][1]).sum()) >= E // 7      # some given pairs are the positive's own destination
    assert torch.equal(negative_edges(c["posd"], n_dst, k, SEED, off, neg_dst=c["Gd"]).cpu(), neg)


@pytest.mark.parametrize("objective,param,n_dst,k,m,off,F", CASES)
def test_substitution_is_bitwise_and_runs_repeat(objective, param, n_dst, k, m, off, F):
    from oracle import c_oracle
    c = _case(objective, param, n_dst, k, m, off, F)
    args = (c["zsd"], c["zdd"], c["posd"])
    # again: run-to-run
    assert _same(_run(*args, k, off, objective, param, c["Gd"]), c["out"])
    # the draws handed in as given pairs
    assert _same(_run(*args, 0, off, objective, param, c["combined"].to(DEV)), c["out"])
    # and K given pairs that are the draws of k = K: the path without a set, as it was before the sets existed
    K = k + m
    D = torch.as_tensor(c_oracle.neg_sample(SEED, off, E * K, n_dst).astype(np.int32)).reshape(E, K).to(DEV)
    assert _same(_run(*args, 0, off, objective, param, D), _run(*args, K, off, objective, param, None))


@pytest.mark.parametrize("objective,param,n_dst,k,m,off,F", CASES)
def test_loss_and_gradients_vs_float64_reference_and_link_loss(objective, param, n_dst, k, m, off, F):
    from hgin.linkpred import link_loss
    c = _case(objective, param, n_dst, k, m, off, F)
    loss, g_src, g_dst = c["out"][:3]
    assert loss.dim() == 0 and loss.dtype == torch.float32
    _check(loss, g_src, g_dst, c["ref"], f"given {objective} ({k}, {m}) vs float64")
    a, b = c["zsd"].clone().requires_grad_(True), c["zdd"].clone().requires_grad_(True)
    base = link_loss(a, b, c["posd"], k, SEED, off, objective=objective, temperature=param or 1.0, alpha=param,
                     neg_dst=c["Gd"])
    base.backward()
    _check(loss, g_src, g_dst, (base.detach().cpu(), a.grad.cpu(), b.grad.cpu()),
           f"given {objective} ({k}, {m}) vs link_loss")


@pytest.mark.parametrize("n_dst,k,m,off,F", RANK_CASES)
def test_ranks_exact_on_integer_embeddings_and_metrics(n_dst, k, m, off, F):
    from hgin.linkpred import link_metrics, link_ranks
    from oracle import c_oracle
    pos, zs, zd = _inputs(n_dst, F, integer=True)
    G = _given(pos, n_dst, m)
    K = k + m
    U = c_oracle.neg_sample(SEED, off, E * k, n_dst).astype(np.int64).reshape(E, k)
    nd = np.concatenate([U, G.numpy()], 1).reshape(-1)
    zsn, zdn = zs.numpy().astype(np.int64), zd.numpy().astype(np.int64)
    s_pos = (zsn[pos[0].numpy()] * zdn[pos[1].numpy()]).sum(1)
    s_neg = (zsn[pos[0].repeat_interleave(K).numpy()] * zdn[nd]).sum(1)
    want_gt, want_eq = ref_ranks(s_pos, s_neg, K)
    assert int(want_eq.sum()) >= E // 7
    zsd, zdd, posd, Gd = zs.to(DEV), zd.to(DEV), pos.to(DEV), G.to(DEV)
    gt, eq = link_ranks(zsd, zdd, posd, k, SEED, off, neg_dst=Gd)
    assert gt.dtype == torch.int32 and eq.dtype == torch.int32
    assert np.array_equal(gt.cpu().numpy(), want_gt) and np.array_equal(eq.cpu().numpy(), want_eq)
    # substitution: all K as given pairs, and K given pairs that are the draws of the path without a set
    gt2, eq2 = link_ranks(zsd, zdd, posd, 0, SEED, off, neg_dst=torch.as_tensor(nd.reshape(E, K)).to(DEV))
    assert torch.equal(gt2, gt) and torch.equal(eq2, eq)
    D = torch.as_tensor(c_oracle.neg_sample(SEED, off, E * K, n_dst).astype(np.int32)).reshape(E, K).to(DEV)
    assert _same(link_ranks(zsd, zdd, posd, 0, SEED, off, neg_dst=D), link_ranks(zsd, zdd, posd, K, SEED, off))
    got = link_metrics(zsd, zdd, posd, k, SEED, off, neg_dst=Gd)
    want = ref_metrics(want_gt, want_eq, K)
    assert sorted(got) == sorted(want)
    for name, v in want.items():
        assert got[name].is_cuda and got[name].dim() == 0
        assert abs(float(got[name]) - v) <= 1e-6, (name, float(got[name]), v)


@pytest.mark.parametrize("objective,param,F,k,m", [("softmax", 0.25, 70, 3, 4), ("bpr", 0.0, 8, 2, 9),
                                                   ("selfadv", 4.0, 128, 0, 5), ("bce", 0.0, 6, 4, 3)])
def test_non_contiguous_odd_stride_views(objective, param, F, k, m):
    """Embeddings that are column windows of wider buffers (row stride odd, start not 16-byte aligned): the scalar
    path; the gradient reaches the window and nothing else.  The set is a strided view too (made contiguous inside)."""
    from hgin.linkpred import sampled_link_loss
    from oracle import c_oracle
    n_dst, off = 53, 6
    pos, zs, zd = _inputs(n_dst, F)
    G = _given(pos, n_dst, m)
    g = torch.Generator().manual_seed(5)
    bs = torch.randn(N_SRC, 2 * F + 1, generator=g)
    bd = torch.randn(n_dst, F + 3, generator=g)
    bs[:, 1:F + 1], bd[:, 3:] = zs, zd
    bs, bd = bs.to(DEV).requires_grad_(True), bd.to(DEV).requires_grad_(True)
    vs, vd = bs[:, 1:F + 1], bd[:, 3:]
    assert not vs.is_contiguous() and vs.stride(0) % 2 == 1 and vd.stride(0) % 2 == 1
    wide = torch.zeros(E, m + 2, dtype=torch.int32, device=DEV)
    wide[:, 1:m + 1] = G.to(DEV)
    Gv = wide[:, 1:m + 1]
    assert not Gv.is_contiguous()
    loss = sampled_link_loss(vs, vd, pos.to(DEV), k, SEED, off, neg_dst=Gv, **_kw(objective, param))
    loss.backward()
    U = torch.as_tensor(c_oracle.neg_sample(SEED, off, E * k, n_dst).astype(np.int64)).reshape(E, k)
    ref = ref_obj_loss_and_grads(zs, zd, pos, torch.cat([U, G], 1).reshape(-1).numpy(), k + m, objective, param)
    _check(loss.detach(), bs.grad[:, 1:F + 1], bd.grad[:, 3:], ref, f"strided views {objective} vs float64")
    assert bool((bs.grad[:, 0] == 0).all()) and bool((bs.grad[:, F + 1:] == 0).all())
    assert bool((bd.grad[:, :3] == 0).all())


@pytest.mark.parametrize("objective,param,n_edges", [("bce", 0.0, 70_001), ("softmax", 1.0, 70_001), ("bce", 0.0, 1),
                                                     ("softmax", 1.0, 1), ("bpr", 0.0, 1), ("selfadv", 1.0, 1)])
def test_second_trip_of_the_persistent_loop_and_a_single_positive(objective, param, n_edges):
    """E = 70 001 at G = 32: every wave takes a second or third trip and the last wave has an idle group (which redoes
    the last edge, given reads included); E = 1: one group works, every other one idles."""
    from oracle import c_oracle
    n_dst, k, m, off, F = 53, 3, 4, 6, 128
    c = _case(objective, param, n_dst, k, m, off, F, n_edges)
    neg = c["out"][3].cpu()
    assert torch.equal(neg[1].reshape(n_edges, k + m), c["combined"])
    assert torch.equal(neg[0], c["pos"][0].repeat_interleave(k + m))
    _check(*c["out"][:3], c["ref"], f"E = {n_edges} given {objective} vs float64")
    args = (c["zsd"], c["zdd"], c["posd"])
    assert _same(_run(*args, k, off, objective, param, c["Gd"]), c["out"])
    K = k + m
    D = torch.as_tensor(c_oracle.neg_sample(SEED, off, n_edges * K, n_dst).astype(np.int32)).reshape(n_edges, K).to(DEV)
    assert _same(_run(*args, 0, off, objective, param, c["combined"].to(DEV)), c["out"])
    assert _same(_run(*args, 0, off, objective, param, D), _run(*args, K, off, objective, param, None))


def test_launch_tags():
    from hgin import _lib
    from hgin.linkpred import link_ranks
    for objective, tag in (("bce", "LOSS"), ("softmax", "SOFTMAX"), ("bpr", "BPR"), ("selfadv", "SELFADV")):
        c = _case(objective, 1.0 if objective in ("softmax", "selfadv") else 0.0, 53, 3, 4, 6, 128)
        args = (c["zsd"], c["zdd"], c["posd"])
        with _lib.trace_launches() as tr:
            _run(*args, 3, 6, objective, 1.0, c["Gd"])
        assert f"k_link_fwd<4,32,ONE,{tag},GIVEN>" in tr.kernels and "k_link_loss_sum" in tr.kernels
        assert "k_link_bwd_src<4,32>" in tr.kernels and "k_link_bwd_dst<4,32>" in tr.kernels
        assert f"k_link_fwd<4,32,ONE,{tag}>" not in tr.kernels
        with _lib.trace_launches() as tr:
            _run(*args, 7, 6, objective, 1.0, None)
        assert f"k_link_fwd<4,32,ONE,{tag}>" in tr.kernels and not any("GIVEN" in t for t in tr.kernels)
    c = _case("bce", 0.0, 53, 3, 4, 6, 128)
    with _lib.trace_launches() as tr:
        link_ranks(c["zsd"], c["zdd"], c["posd"], 3, SEED, 6, neg_dst=c["Gd"])
        link_ranks(c["zsd"], c["zdd"], c["posd"], 3, SEED, 6)
    assert [t for t in tr.kernels if t.startswith("k_link")] == ["k_link_fwd<4,32,ONE,RANK,GIVEN>",
                                                                 "k_link_fwd<4,32,ONE,RANK>"]
    pos, zs, zd = _inputs(53, 260)
    with _lib.trace_launches() as tr:
        _run(zs.to(DEV), zd.to(DEV), pos.to(DEV), 0, 6, "bce", 0.0, _given(pos, 53, 2).to(DEV))
    assert "k_link_fwd<4,64,LOOP,LOSS,GIVEN>" in tr.kernels


def test_the_set_is_range_checked_once_and_bad_sets_raise_before_any_launch():
    from hgin import _lib
    from hgin.linkpred import link_ranks, sampled_link_loss
    c = _case("bce", 0.0, 53, 3, 4, 6, 128)
    zs, zd, pos = c["zsd"], c["zdd"], c["posd"]
    for bad_value in (53, -1, 2**31 + 5):
        for dtype in (torch.int64, torch.int32):
            if dtype == torch.int32 and bad_value >= 2**31:
                continue
            G = c["G"].to(DEV, dtype).clone()
            G[100, 2] = bad_value
            with _lib.trace_launches() as tr:
                with pytest.raises(IndexError, match="neg_dst index out of range"):
                    sampled_link_loss(zs, zd, pos, 3, SEED, neg_dst=G)
                with pytest.raises(IndexError, match="neg_dst index out of range"):
                    link_ranks(zs, zd, pos, 3, SEED, neg_dst=G)
            assert tr.kernels == []
            assert not hasattr(G, "_hgin_neg_dst")
    with pytest.raises(ValueError, match="E \\* \\(k \\+ m\\)"):
        sampled_link_loss(zs, zd, pos, 2**31 // E, SEED, neg_dst=c["Gd"])
    with pytest.raises(ValueError, match="k >= 1"):
        sampled_link_loss(zs, zd, pos, 0, SEED)
    # once per tensor version: the checked set is cached on the tensor and handed back without another look
    for G in (c["G"].to(DEV), c["G"].to(DEV, torch.int32)):
        assert not hasattr(G, "_hgin_neg_dst")
        first = sampled_link_loss(zs, zd, pos, 3, SEED, neg_dst=G)
        ver, cache = G._hgin_neg_dst
        assert ver == G._version and list(cache) == [53]
        assert cache[53].dtype == torch.int32 and cache[53].is_contiguous()
        assert (cache[53] is G) == (G.dtype == torch.int32)           # an int32 contiguous set is passed as it is
        kept = cache[53]
        assert torch.equal(sampled_link_loss(zs, zd, pos, 3, SEED, neg_dst=G), first)
        assert G._hgin_neg_dst[1][53] is kept
        G[0, 0] = 52                                                   # a new version is checked again
        sampled_link_loss(zs, zd, pos, 3, SEED, neg_dst=G)
        assert G._hgin_neg_dst[0] == G._version
        if G.dtype == torch.int64:
            assert G._hgin_neg_dst[1][53] is not kept
        G[0, 0] = 53
        with pytest.raises(IndexError):
            sampled_link_loss(zs, zd, pos, 3, SEED, neg_dst=G)


# ---------------------------------------------------------------------------------------------------
# hard_negatives
# ---------------------------------------------------------------------------------------------------
def _mining_inputs(F, m):
    """Integer embeddings; ``known`` = the positives, plus one source that knows all but m - 2 destinations and one
    that knows every destination (both own positives); the other sources know their few positives only."""
    n_dst = 53
    pos, zs, zd = _inputs(n_dst, F, integer=True)
    a, b = int(pos[0, 0]), int(pos[0][pos[0] != pos[0, 0]][0])
    all_dst = torch.arange(n_dst)
    keep = torch.ones(n_dst, dtype=torch.bool)
    own = set(pos[1][pos[0] == a].tolist())
    free = [d for d in range(n_dst) if d not in own][:m - 2]       # the m - 2 destinations source a does not know
    keep[free] = False
    known = torch.cat([pos, torch.stack([torch.full((int(keep.sum()),), a), all_dst[keep]]),
                       torch.stack([torch.full((n_dst,), b), all_dst])], 1)
    return n_dst, pos, zs, zd, known, a, b, len(free)


@pytest.mark.parametrize("F,m", [(8, 6), (128, 3), (70, 128)])
def test_hard_negatives_are_the_filtered_top_m_with_sampled_padding(F, m):
    import hgin
    from hgin.linkpred import link_topk
    from oracle import c_oracle
    n_dst, pos, zs, zd, known, a, b, n_free = _mining_inputs(F, m)
    assert n_free == m - 2 or m > n_dst
    seed, off = 4242, 2**32 + 3
    zsd, zdd, posd, knownd = zs.to(DEV).requires_grad_(True), zd.to(DEV), pos.to(DEV), known.to(DEV)
    got = hgin.hard_negatives(zsd, zdd, posd, m, knownd, seed, off)
    assert got.dtype == torch.int32 and tuple(got.shape) == (E, m) and not got.requires_grad and got.is_contiguous()
    assert hasattr(got, "_hgin_neg_dst")                            # in range by construction: never re-checked
    got = got.cpu().numpy().astype(np.int64)
    want, _ = ref_topk(zs.numpy(), zd.numpy(), pos[0].numpy(), m, known.numpy())
    direct, _ = link_topk(zsd.detach(), zdd, posd[0].contiguous(), m, knownd)
    assert np.array_equal(direct.cpu().numpy().astype(np.int64), want)
    pad = want < 0
    assert np.array_equal(got[~pad], want[~pad])
    # the padded slots are exactly those past a source's candidates, counted on the CPU
    deg = np.zeros(N_SRC, dtype=np.int64)
    for s, _d in {(int(s), int(d)) for s, d in known.t().tolist()}:
        deg[s] += 1
    assert deg[a] == n_dst - n_free and deg[b] == n_dst
    n_cand = n_dst - deg[pos[0].numpy()]
    want_pad = np.arange(m)[None, :] >= n_cand[:, None]
    assert np.array_equal(pad, want_pad)
    assert int(pad[pos[0].numpy() == b].sum()) == m * int((pos[0] == b).sum())       # that source: every slot
    if n_free == m - 2:
        assert int(pad[pos[0].numpy() == a].sum()) == 2 * int((pos[0] == a).sum())   # this one: its last two
    draws = c_oracle.neg_sample(seed, off, E * m, n_dst).astype(np.int64).reshape(E, m)
    assert np.array_equal(got[pad], draws[pad])
    is_known = np.zeros((N_SRC, n_dst), dtype=bool)
    is_known[known[0].numpy(), known[1].numpy()] = True
    src = np.repeat(pos[0].numpy()[:, None], m, 1)
    assert not is_known[src[~pad], got[~pad]].any()
    assert (got >= 0).all() and (got < n_dst).all()
    # default known = pos itself, default seed / offset
    got2 = hgin.hard_negatives(zsd, zdd, posd, m).cpu().numpy().astype(np.int64)
    want2, _ = ref_topk(zs.numpy(), zd.numpy(), pos[0].numpy(), m, pos.numpy())
    pad2 = want2 < 0
    assert np.array_equal(got2[~pad2], want2[~pad2])
    assert np.array_equal(got2[pad2], c_oracle.neg_sample(0, 0, E * m, n_dst).astype(np.int64).reshape(E, m)[pad2])


def test_mined_set_feeds_the_loss_without_another_range_check():
    import hgin
    n_dst, pos, zs, zd, known, _, _, _ = _mining_inputs(8, 6)
    zsd, zdd, posd = (zs * 0.25).to(DEV), (zd * 0.25).to(DEV), pos.to(DEV)
    mined = hgin.hard_negatives(zsd, zdd, posd, 6, known.to(DEV))
    kept = mined._hgin_neg_dst[1][n_dst]
    assert kept is mined
    out = _run(zsd, zdd, posd, 2, 6, "softmax", 1.0, mined)
    assert mined._hgin_neg_dst[1][n_dst] is kept
    assert torch.equal(out[3][1].reshape(E, 8)[:, 2:], mined.long())
    ref = ref_obj_loss_and_grads(zs * 0.25, zd * 0.25, pos, out[3][1].cpu().numpy(), 8, "softmax", 1.0)
    _check(*out[:3], ref, "mined softmax vs float64")


# ---------------------------------------------------------------------------------------------------
# model level (cfg1 synthetic graph)
# ---------------------------------------------------------------------------------------------------
def test_four_link_train_steps_mine_every_second_step():
    import hgin
    from hgin.linkpred import link_metrics, sampled_link_loss
    cfg, g, _, model = _gin_pair()
    gd = g.to(DEV)
    k, m, seed = 1, 2, 7
    pos = gd.edge_index[REL_PL]
    n_e = int(pos.size(1))
    recorded = []
    encode = model.encode

    def recording_encode(*args, **kw):
        z = encode(*args, **kw)
        recorded.append(z)
        return z

    model.encode = recording_encode
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    pred = hgin.LinkPredictor(model, REL_PL, k, seed, objective="softmax", hard=m, mine_every=2)
    assert pred.neg_dst is None
    previous = None
    for step in range(4):
        before = [p.detach().clone() for p in model.parameters()]
        loss = hgin.link_train_step(model, opt, gd, pred, step=step)
        assert len(recorded) == step + 1                      # mining costs no second encode
        z = recorded[step]
        zs, zd = z["path"].detach(), z["link"].detach()
        if step % 2 == 0:
            want = hgin.hard_negatives(zs, zd, pos, m, pos, seed + 1, step * n_e * m)
            assert pred.neg_dst is not previous and torch.equal(pred.neg_dst, want)
        else:
            assert pred.neg_dst is previous
        previous = pred.neg_dst
        assert pred.neg_dst.dtype == torch.int32 and tuple(pred.neg_dst.shape) == (n_e, m)
        again = sampled_link_loss(zs, zd, pos, k, seed, step * n_e, objective="softmax", neg_dst=pred.neg_dst)
        assert torch.equal(again, loss) and bool(torch.isfinite(loss))
        changed = [not torch.equal(p.detach(), q) for p, q in zip(model.parameters(), before) if p.grad is not None]
        assert sum(changed) >= 8
    # mine() on demand: an eval-mode encode without gradients, the mode restored; metrics with an evaluation set
    assert model.training
    mined = pred.mine(gd)
    assert model.training and mined is pred.neg_dst and mined is not previous and len(recorded) == 5
    assert not recorded[4]["path"].requires_grad
    zs, zd = recorded[4]["path"], recorded[4]["link"]
    assert torch.equal(mined, hgin.hard_negatives(zs, zd, pos, m, pos, seed + 1, 0))
    got = pred.metrics(gd, neg_dst=mined)
    want = link_metrics(recorded[5]["path"], recorded[5]["link"], pos, k, seed, neg_dst=mined)
    assert sorted(got) == sorted(want) and all(torch.equal(got[n], want[n]) for n in want)
