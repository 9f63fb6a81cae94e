"""Full-candidate softmax link loss (A23), host side (no GPU): this file's float64 restatement (the one
tests/test_gpu_linklse.py checks the kernels against) gives a hand-computed case, the public surface exists, host
tensors, other dtypes, repeated sources and bad temperatures are refused, the four entry points reject bad arguments
before touching the device, ``SampledSubgraph.local_edges`` agrees with a dict-based restatement on CPU tensors, and the
bench tool plans its shapes and FLOP counts on the CPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

from test_linkrank_host import ZD, ZS

U = 2.0 ** -24


# ---------------------------------------------------------------------------------------------------
# float64 restatement (shared with tests/test_gpu_linklse.py)
# ---------------------------------------------------------------------------------------------------
def inv_t_of(temperature: float) -> float:
    """fl32(1 / temperature), the factor the kernels multiply a score by."""
    return float(np.float32(1.0 / float(temperature)))


def lse_candidate_mask(src, n_src: int, n_dst: int, known) -> np.ndarray:
    """bool [Q, n_dst]: c is a candidate of query q when (src[q], c) is not in ``known``."""
    is_known = np.zeros((n_src, n_dst), dtype=bool)
    if known is not None:
        known = np.asarray(known)
        is_known[known[0], known[1]] = True
    return ~is_known[np.asarray(src)]


def _masked_lse(t: np.ndarray, mask: np.ndarray) -> np.ndarray:
    tm = np.where(mask, t, -np.inf)
    mx = tm.max(1)
    safe = np.where(np.isfinite(mx), mx, 0.0)
    with np.errstate(divide="ignore"):
        return np.where(np.isfinite(mx), safe + np.log(np.exp(tm - safe[:, None]).sum(1)), -np.inf)


def ref_lse(zs, zd, src, temperature=1.0, known=None) -> np.ndarray:
    """float64 [Q]: log sum over the candidates of exp(score * fl32(1 / T)); -inf for a query without candidates."""
    zs, zd, src = np.asarray(zs, np.float64), np.asarray(zd, np.float64), np.asarray(src)
    t = (zs[src] @ zd.T) * inv_t_of(temperature)
    return _masked_lse(t, lse_candidate_mask(src, zs.shape[0], zd.shape[0], known))


def ref_lse_probs(zs, zd, src, temperature=1.0, known=None) -> np.ndarray:
    """float64 [Q, n_dst]: P = exp(t - lse) on the candidates, 0 elsewhere and in the rows whose lse is -inf."""
    zs, zd, src = np.asarray(zs, np.float64), np.asarray(zd, np.float64), np.asarray(src)
    t = (zs[src] @ zd.T) * inv_t_of(temperature)
    mask = lse_candidate_mask(src, zs.shape[0], zd.shape[0], known)
    lse = _masked_lse(t, mask)
    fin = np.isfinite(lse)
    return np.where(mask & fin[:, None], np.exp(np.where(mask, t, -np.inf) - np.where(fin, lse, 0.0)[:, None]), 0.0)


def ref_lse_grads(zs, zd, src, g, temperature=1.0, known=None):
    """(G_src [n_src, F], G_dst [n_dst, F], A_src, A_dst) in float64: the gradients of sum_q g[q] lse[q] and the
    magnitudes A the error bounds scale with (the same sums over absolute values)."""
    zs, zd, src, g = np.asarray(zs, np.float64), np.asarray(zd, np.float64), np.asarray(src), np.asarray(g, np.float64)
    it = inv_t_of(temperature)
    P = ref_lse_probs(zs, zd, src, temperature, known)
    G_src, A_src = np.zeros_like(zs), np.zeros_like(zs)
    G_src[src] = g[:, None] * it * (P @ zd)
    A_src[src] = np.abs(g)[:, None] * it * (P @ np.abs(zd))
    G_dst = it * (P * g[:, None]).T @ zs[src]
    A_dst = it * (P * np.abs(g)[:, None]).T @ np.abs(zs[src])
    return G_src, G_dst, A_src, A_dst


def ref_lse_tol(zs, zd, src, temperature=1.0, known=None) -> np.ndarray:
    """The forward's derived bound, float64 [Q]: with u = 2^-24 and b[q, c] = 2 F u sum_f |zs zd| (``ref_full_bands``),
    tol[q] = inv_t max_c (b + u |score|) + (n_cand + 64) u + u |lse|; lse is 1-Lipschitz in the scores, the second term
    covers the fp32 sum and a few ulp of exp / log.  A query without candidates gets 0 (its -inf is exact)."""
    zs, zd, src = np.asarray(zs, np.float64), np.asarray(zd, np.float64), np.asarray(src)
    F = zs.shape[1]
    it = inv_t_of(temperature)
    score = zs[src] @ zd.T
    b = 2.0 * F * U * (np.abs(zs[src]) @ np.abs(zd).T)
    mask = lse_candidate_mask(src, zs.shape[0], zd.shape[0], known)
    lse = ref_lse(zs, zd, src, temperature, known)
    n_cand = mask.sum(1)
    first = it * np.where(mask, b + U * np.abs(score), 0.0).max(1)
    return np.where(np.isfinite(lse), first + (n_cand + 64) * U + U * np.abs(np.where(np.isfinite(lse), lse, 0.0)), 0.0)


def ref_full_softmax(zs, zd, pos, temperature=1.0, known=None) -> float:
    """float64 scalar: mean over the positives (s, d) of log sum_{c in C(s, d)} exp(t[s, c]) - t[s, d]; C = every
    destination without ``known``; with it, d itself plus the destinations that are neither known nor positive
    neighbours of s."""
    zs, zd, pos = np.asarray(zs, np.float64), np.asarray(zd, np.float64), np.asarray(pos)
    t = (zs[pos[0]] @ zd.T) * inv_t_of(temperature)
    E = pos.shape[1]
    if known is None:
        mask = np.ones_like(t, dtype=bool)
    else:
        mask = lse_candidate_mask(pos[0], zs.shape[0], zd.shape[0], np.concatenate([np.asarray(known), pos], 1))
        mask[np.arange(E), pos[1]] = True
    return float((_masked_lse(t, mask) - t[np.arange(E), pos[1]]).mean())


# ---------------------------------------------------------------------------------------------------
# the hand-computed case of tests/test_linkrank_host.py: 3 sources, 4 destinations, F = 2
#   scores   d0  d1  d2  d3
#   s0        2   2   0  -1
#   s1        1   1   3  -2
#   s2       -2  -2   0   1
# known: (0, 3), and source 1 to every destination
KNOWN_LSE = [[0, 1, 1, 1, 1], [3, 0, 1, 2, 3]]


def test_reference_on_the_hand_computed_case():
    e = math.e
    lse = ref_lse(ZS, ZD, [0, 1, 2])
    want = [math.log(2 * e ** 2 + 1 + 1 / e), math.log(2 * e + e ** 3 + e ** -2), math.log(2 * e ** -2 + 1 + e)]
    assert np.allclose(lse, want, rtol=0, atol=1e-14)
    lse = ref_lse(ZS, ZD, [0, 1, 2], 1.0, KNOWN_LSE)
    assert lse[1] == -np.inf
    assert np.allclose(lse[[0, 2]], [math.log(2 * e ** 2 + 1), want[2]], rtol=0, atol=1e-14)
    lse = ref_lse(ZS, ZD, [2, 0], 0.5, KNOWN_LSE)        # another order of queries, t = 2 score
    assert np.allclose(lse, [math.log(2 * e ** -4 + 1 + e ** 2), math.log(2 * e ** 4 + 1)], rtol=0, atol=1e-14)
    P = ref_lse_probs(ZS, ZD, [0, 1, 2], 1.0, KNOWN_LSE)
    assert P[1].tolist() == [0.0] * 4 and P[0, 3] == 0.0 and abs(P[0].sum() - 1) < 1e-15 and abs(P[2].sum() - 1) < 1e-15
    g = np.array([2.0, 5.0, -1.0])
    G_src, G_dst, A_src, A_dst = ref_lse_grads(ZS, ZD, [0, 1, 2], g, 1.0, KNOWN_LSE)
    z0 = 2 * e ** 2 + 1
    assert np.allclose(G_src[0], 2.0 * (2 * e ** 2 * np.array([2.0, 1.0]) + np.array([0.0, 3.0])) / z0, atol=1e-14)
    assert G_src[1].tolist() == [0.0, 0.0]                       # no candidate: no gradient, whatever g is
    z2 = np.exp(want[2])
    assert np.allclose(G_dst[3], -1.0 * (e / z2) * np.array(ZS[2]), atol=1e-14)    # d3: only source 2 sees it
    assert np.allclose(G_dst[2], 2.0 / z0 * np.array(ZS[0]) - 1.0 / z2 * np.array(ZS[2]), atol=1e-14)
    assert (A_src >= np.abs(G_src) - 1e-15).all() and (A_dst >= np.abs(G_dst) - 1e-15).all()
    tol = ref_lse_tol(ZS, ZD, [0, 1, 2], 1.0, KNOWN_LSE)
    assert tol[1] == 0.0 and 0 < tol[0] < 1e-4 and 0 < tol[2] < 1e-4
    # full softmax: two positives of source 0; with known each keeps itself and drops the other
    pos = [[0, 0, 2], [0, 2, 3]]
    want_plain = ((ref_lse(ZS, ZD, [0])[0] - 2) + (ref_lse(ZS, ZD, [0])[0] - 0) + (want[2] - 1)) / 3
    assert abs(ref_full_softmax(ZS, ZD, pos) - want_plain) < 1e-14
    # known (0, 3): (0 -> 0) sees d0, d1; (0 -> 2) sees d1, d2; (2 -> 3) sees everything
    want_known = ((math.log(2 * e ** 2) - 2) + (math.log(e ** 2 + 1) - 0) + (want[2] - 1)) / 3
    assert abs(ref_full_softmax(ZS, ZD, pos, 1.0, [[0], [3]]) - want_known) < 1e-14


def test_public_surface():
    import hgin
    from hgin import _lib, linkpred
    for name in ("link_lse", "link_lse_unfused", "full_softmax_link_loss"):
        assert name in hgin.__all__ and getattr(hgin, name) is getattr(linkpred, name)
    assert callable(hgin.LinkPredictor.full_loss) and callable(hgin.LinkPredictor.batch_full_loss)
    assert callable(hgin.SampledSubgraph.local_edges)
    assert hgin.LINK_OBJECTIVES == ("bce", "softmax", "bpr", "selfadv")
    lib = _lib.lib()
    assert lib.hgin_abi_version() == _lib.ABI_VERSION == 16
    for name in ("hgin_link_lse_workspace_size", "hgin_link_lse_fwd_f32", "hgin_link_lse_bwd_src_f32",
                 "hgin_link_lse_bwd_dst_f32"):
        assert name in _lib.exported_symbols() and hasattr(lib, name), name


def test_bad_inputs_are_refused_before_any_launch():
    from hgin import linkpred
    z = torch.zeros(3, 4)
    src = torch.tensor([0, 2])
    known = torch.zeros(2, 2, dtype=torch.long)
    for fn in (linkpred.link_lse, linkpred.link_lse_unfused):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(z, z, src)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(z, z, src, 1.0, known)
        with pytest.raises(TypeError, match=r"z_src must be float32 \(the fused link kernels are fp32 only\)"):
            fn(z.bfloat16(), z, src)
        with pytest.raises(TypeError, match=r"z_dst must be float32 \(the fused link kernels are fp32 only\)"):
            fn(z, z.bfloat16(), src)
        with pytest.raises(ValueError, match=r"src must be an int64 \[Q\] tensor"):
            fn(z, z, src.int())
        with pytest.raises(ValueError, match=r"src must be an int64 \[Q\] tensor"):
            fn(z, z, known)
        with pytest.raises(ValueError, match="distinct"):
            fn(z, z, torch.tensor([1, 0, 1]))
        with pytest.raises(IndexError, match="out of range"):
            fn(z, z, torch.tensor([1, 3]))
        for t in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(ValueError, match="temperature must be finite and > 0"):
                fn(z, z, src, t)
        with pytest.raises(TypeError, match="known must be an int64 edge index"):
            fn(z, z, src, 1.0, known.int())
    pos = torch.tensor([[0, 1], [1, 2]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        linkpred.full_softmax_link_loss(z, z, pos)
    with pytest.raises(TypeError, match="fp32 only"):
        linkpred.full_softmax_link_loss(z.bfloat16(), z, pos)
    with pytest.raises(ValueError, match="temperature must be finite and > 0"):
        linkpred.full_softmax_link_loss(z, z, pos, 0.0)


def test_full_losses_refuse_graph_local_and_hard():
    from hgin import linkpred

    class Model:
        def encode(self, x, e):
            raise AssertionError("refused before any encode")

    rel = ("a", "to", "b")
    for kw in ({"hard": 2}, {"graph_local": True}):
        lp = linkpred.LinkPredictor(Model(), rel, 1, 0, **kw)
        with pytest.raises(ValueError, match="hard > 0 and graph_local = True are not supported"):
            lp.full_loss(None)
        with pytest.raises(ValueError, match="hard > 0 and graph_local = True are not supported"):
            lp.batch_full_loss(None, torch.zeros(2, 1, dtype=torch.long))
    lp = linkpred.LinkPredictor(Model(), rel, 1, 0)
    with pytest.raises(TypeError, match="sampler must be a NeighborSampler"):
        lp.batch_full_loss(None, torch.zeros(2, 1, dtype=torch.long))


_Q = ctypes.c_void_p(16)   # a non-NULL pointer that must never be dereferenced
_F = ctypes.c_float


def _fwd(lib, src=_Q, Q=4, n_src=5, n_dst=300, zs=_Q, lds=8, zd=_Q, ldd=8, F=8, inv_t=1.0, rowptr=None, col=None,
         lse=_Q, ws=_Q, ws_bytes=1 << 20):
    return lib.hgin_link_lse_fwd_f32(src, Q, n_src, n_dst, zs, lds, zd, ldd, F, _F(inv_t), rowptr, col, lse, ws, ws_bytes,
                                     None)


def _bwd(fn, src=_Q, Q=4, n_src=5, n_dst=300, zs=_Q, lds=8, zd=_Q, ldd=8, F=8, inv_t=1.0, rowptr=None, col=None,
         lse=_Q, g=_Q, out=_Q, ldo=8, ws=_Q, ws_bytes=1 << 20):
    return fn(src, Q, n_src, n_dst, zs, lds, zd, ldd, F, _F(inv_t), rowptr, col, lse, g, out, ldo, ws, ws_bytes, None)


def test_argument_errors_do_not_touch_the_device():
    from hgin import _lib
    lib = _lib.lib()
    err = lib.hgin_last_error
    calls = [lambda **kw: _fwd(lib, **kw), lambda **kw: _bwd(lib.hgin_link_lse_bwd_src_f32, **kw),
             lambda **kw: _bwd(lib.hgin_link_lse_bwd_dst_f32, **kw)]
    for call in calls:
        assert call(Q=0) == -1 and b"n_query = 0" in err()
        assert call(Q=1 << 31) == -1 and b"n_query = " in err()
        assert call(n_src=0) == -1 and b"n_src" in err()
        assert call(n_dst=0) == -1 and b"n_dst" in err()
        assert call(n_dst=1 << 31) == -1 and b"n_dst" in err()
        assert call(F=0) == -1 and b"F " in err()
        assert call(F=-3) == -1 and b"F " in err()
        assert call(F=1 << 24, lds=1 << 24, ldd=1 << 24) == -1 and b"F " in err()
        assert call(src=None) == -1 and b"src NULL" in err()
        assert call(zs=None) == -1 and b"z_src NULL" in err()
        assert call(zd=None) == -1 and b"z_dst NULL" in err()
        assert call(lds=7) == -1 and b"leading dimension" in err()
        assert call(ldd=7) == -1 and b"leading dimension" in err()
        assert call(inv_t=0.0) == -1 and b"inv_t" in err()
        assert call(inv_t=float("inf")) == -1 and b"inv_t" in err()
        assert call(inv_t=float("nan")) == -1 and b"inv_t" in err()
        assert call(rowptr=_Q, col=None) == -1 and b"known_rowptr without known_col" in err()
        assert call(lse=None) == -1 and b"lse NULL" in err()
        # 512 splits x 128 queries, or 64 splits x 1024 destinations, x 2^23 features: 2^39 floats of partials, which
        # no launch could fold
        wide = {"F": 1 << 23, "lds": 1 << 23, "ldd": 1 << 23}
        if call is not calls[0]:
            wide["ldo"] = 1 << 23
        assert call(Q=128, n_src=128, n_dst=1 << 20, **wide) == -1 and b"split partials of g_src" in err()
        assert call(Q=1 << 20, n_src=1 << 20, n_dst=1 << 10, **wide) == -1 and b"split partials of g_dst" in err()
        # Q = 4 against 300 destinations: 3 splits in the forward and in bwd_src; Q = 300 against 4: 3 splits in bwd_dst
        shape = {"Q": 300, "n_src": 300, "n_dst": 4} if call is calls[2] else {}
        assert call(ws_bytes=8, **shape) == -3 and b"workspace" in err()
        assert call(ws=None, **shape) == -3 and b"workspace" in err()
    for call, name in ((calls[1], b"g_src NULL"), (calls[2], b"g_dst NULL")):
        assert call(g=None) == -1 and b"g NULL" in err()
        assert call(out=None) == -1 and name in err()
        assert call(ldo=7) == -1 and b"leading dimension" in err()

    sz = ctypes.c_size_t(0)
    size = lib.hgin_link_lse_workspace_size
    # 4 queries against 300 destinations: 3 splits; the forward needs 8 bytes per (split, query), bwd_src 4 F
    assert size(4, 300, 8, ctypes.byref(sz)) == 0 and sz.value >= 3 * 4 * 4 * 8
    # 32768 queries are 256 blocks: 2 splits of the forward (the destinations' side, 5 tiles, is cut further)
    assert size(32768, 600, 8, ctypes.byref(sz)) == 0 and sz.value >= 2 * 32768 * 8 * 4
    assert size(4, 300, 8, None) == -1 and b"bytes" in err()
    assert size(0, 300, 8, ctypes.byref(sz)) == -1 and b"n_query = 0" in err()
    assert size(4, 0, 8, ctypes.byref(sz)) == -1 and b"n_dst" in err()
    assert size(4, 300, 0, ctypes.byref(sz)) == -1 and b"F " in err()
    assert size(4, 300, 1 << 24, ctypes.byref(sz)) == -1 and b"F " in err()
    assert size(128, 1 << 20, 1 << 23, ctypes.byref(sz)) == -1 and b"split partials of g_src" in err()
    assert size(64, 1 << 20, 1 << 23, ctypes.byref(sz)) == 0 and sz.value == 512 * 64 * (1 << 23) * 4   # 2^40 bytes


def test_local_edges_against_a_dict_restatement():
    from hgin.neighbor import SampledSubgraph
    g = np.random.default_rng(5)
    seeds_a = np.sort(g.choice(50, 9, replace=False))
    seeds_b = np.sort(g.choice(40, 7, replace=False))
    n_id = {"a": torch.as_tensor(np.concatenate([seeds_a, [99, 3 if 3 not in seeds_a else 98]])),
            "b": torch.as_tensor(np.concatenate([seeds_b, [77]]))}
    sub = SampledSubgraph(graph=None, n_id=n_id, e_id={}, n_seed={"a": 9, "b": 7})
    edges = np.stack([g.integers(0, 50, 400), g.integers(0, 40, 400)])
    edges[:, :5] = [[seeds_a[0], seeds_a[8], seeds_a[3], 99, seeds_a[1]], [seeds_b[6], seeds_b[0], seeds_b[2], seeds_b[1], 77]]
    la, lb = {int(v): i for i, v in enumerate(seeds_a)}, {int(v): i for i, v in enumerate(seeds_b)}
    want = [(la[int(s)], lb[int(d)]) for s, d in edges.T if int(s) in la and int(d) in lb]
    got = sub.local_edges("a", "b", torch.as_tensor(edges))
    assert got.dtype == torch.int64 and got.shape == (2, len(want)) and len(want) >= 3
    assert [tuple(p) for p in got.t().tolist()] == want            # 99 and 77 are rows of the batch but no seeds
    assert sub.local_edges("a", "b", torch.zeros(2, 0, dtype=torch.long)).shape == (2, 0)
    same = sub.local_edges("a", "a", torch.as_tensor(np.stack([seeds_a, seeds_a[::-1].copy()])))
    assert same.tolist() == [list(range(9)), list(range(8, -1, -1))]
    empty = SampledSubgraph(graph=None, n_id=n_id, e_id={}, n_seed={"a": 9, "b": 0})
    assert empty.local_edges("a", "b", torch.as_tensor(edges)).shape == (2, 0)
    with pytest.raises(ValueError, match="unknown node type"):
        sub.local_edges("a", "c", torch.as_tensor(edges))
    with pytest.raises(TypeError, match="int64"):
        sub.local_edges("a", "b", torch.as_tensor(edges).int())
    with pytest.raises(ValueError, match=r"\[2, M\]"):
        sub.local_edges("a", "b", torch.zeros(3, 4, dtype=torch.long))


def test_bench_tool_plans_shapes_and_flops_on_the_cpu(capsys):
    import importlib.util
    import os

    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("bench_linklse", os.path.join(ROOT, "tools", "bench_linklse.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    shapes = tool.plan()
    assert [(s["name"], s["known_degree"]) for s in shapes] == [
        ("inbatch_f128", 0), ("inbatch_f128", 6), ("inbatch_f256", 0), ("inbatch_f256", 6), ("cfg2", 0), ("cfg2", 6),
        ("cfg3", 0), ("cfg3", 6)]
    s = shapes[0]
    assert (s["Q"], s["n_src"], s["n_dst"], s["F"]) == (4096, 4096, 4096, 128)
    sweep = 2 * 4096 * 4096 * 128
    assert s["flop"] == {"k_lse_sweep": sweep, "k_lse_bwd_src": 2 * sweep, "k_lse_bwd_dst": 2 * sweep,
                         "total": 5 * sweep}
    s = shapes[6]
    assert (s["Q"], s["n_dst"], s["F"]) == (4096, 3_000_000, 256) and shapes[4]["n_dst"] == 300_000
    sweep = 2 * 4096 * 3_000_000 * 256
    assert s["flop"]["k_lse_sweep"] == sweep and s["flop"]["k_lse_bwd_dst"] == 2 * sweep     # one chunk of 256 features
    assert tool.kernel_flop(10, 20, 260)["k_lse_bwd_src"] == 3 * 2 * 10 * 20 * 260           # two chunks past 256
    assert s["baseline_chunk_rows"] == (1 << 30) // (4 * 3_000_000)
    assert s["score_bytes_not_materialised"] == 4 * 4096 * 3_000_000
    assert tool.plan(0.01, 64)[4]["n_dst"] == 3000 and tool.plan(0.01, 64)[0]["n_dst"] == 64
    # the reduction of a kernel trace: medians per A23 kernel over the FLOPs of the one traced shape
    import json
    import tempfile
    head = '"Kind","Kernel_Name","Start_Timestamp","End_Timestamp"\n'
    sig = "(long const*, long)"
    rows = [("void hgin::(anonymous namespace)::k_lse_sweep<true>" + sig, 0, 50_000),
            ("void hgin::(anonymous namespace)::k_lse_sweep<true>" + sig, 100_000, 170_000),
            ("void hgin::(anonymous namespace)::k_lse_sweep<true>" + sig, 200_000, 260_000),
            ("void hgin::(anonymous namespace)::k_lse_bwd<true, false, 2>" + sig, 300_000, 400_000),
            ("void hgin::(anonymous namespace)::k_lse_bwd<true, true, 2>" + sig, 400_000, 600_000),
            ("void at::native::vectorized_elementwise_kernel<4, true, false>" + sig, 0, 1)]
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "t_kernel_trace.csv")
        with open(path, "w") as f:
            f.write(head + "".join(f'"KERNEL_DISPATCH","{n}",{a},{b}\n' for n, a, b in rows))
        rates = tool.kernel_rates(path, shapes[0])
        assert {k: (v["launches"], v["median_us"]) for k, v in rates.items()} == {
            "k_lse_sweep": (3, 60.0), "k_lse_bwd_src": (1, 100.0), "k_lse_bwd_dst": (1, 200.0)}
        sweep = 2 * 4096 * 4096 * 128
        assert abs(rates["k_lse_bwd_dst"]["tflops"] - 2 * sweep / 200e-6 / 1e12) < 1e-9
        assert abs(rates["k_lse_sweep"]["fraction_of_f32_mfma_peak"] - sweep / 60e-6 / 157e12) < 1e-12
        out = os.path.join(d, "rates.json")
        assert tool.main(["--only", "inbatch_f128", "--rates-from", path, "--out", out]) == 0
        assert json.load(open(out))["kernels"]["k_lse_bwd_src"]["median_us"] == 100.0
        capsys.readouterr()
    if not torch.cuda.is_available():
        rc = tool.main(["--scale", "0.01", "--queries", "64"])
        err = capsys.readouterr().err
        assert rc == 2 and "no HIP device" in err and '"Q": 64' in err
