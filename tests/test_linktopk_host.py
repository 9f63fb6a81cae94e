"""Top-K link retrieval (A16), host side (no GPU): this file's float64 reference (the one tests/test_gpu_linktopk.py
checks the kernels against) gives a hand-computed case, the public surface exists, host tensors and other dtypes are
refused, the two entry points reject bad arguments before touching the device, and the bench tool plans its shapes on
the CPU."""
import ctypes

import numpy as np
import pytest
import torch

from test_linkrank_host import KNOWN, ZD, ZS


# ---------------------------------------------------------------------------------------------------
# float64 reference (shared with tests/test_gpu_linktopk.py)
# ---------------------------------------------------------------------------------------------------
def topk_candidate_mask(src: np.ndarray, n_src: int, n_dst: int, known) -> np.ndarray:
    """bool [Q, n_dst]: c is a candidate of query q when (src[q], c) is not in ``known``."""
    is_known = np.zeros((n_src, n_dst), dtype=bool)
    if known is not None:
        known = np.asarray(known)
        is_known[known[0], known[1]] = True
    return ~is_known[np.asarray(src)]


def ref_topk(zs, zd, src, k, known):
    """(idx int64 [Q, k], score float64 [Q, k]): per query the min(k, candidates) best destinations by float64 score,
    ties in ascending index (a stable argsort of -score over ascending indices), padded with -1 / -inf."""
    zs, zd, src = np.asarray(zs, np.float64), np.asarray(zd, np.float64), np.asarray(src)
    Q, n_dst = src.shape[0], zd.shape[0]
    score = zs[src] @ zd.T
    mask = topk_candidate_mask(src, zs.shape[0], n_dst, known)
    order = np.argsort(np.where(mask, -score, np.inf), axis=1, kind="stable")[:, :k]   # non-candidates sort last
    rows = np.arange(Q)[:, None]
    is_cand = mask[rows, order]
    idx = np.full((Q, k), -1, dtype=np.int64)
    val = np.full((Q, k), -np.inf)
    idx[:, :order.shape[1]] = np.where(is_cand, order, -1)
    val[:, :order.shape[1]] = np.where(is_cand, score[rows, order], -np.inf)
    return idx, val


# the hand-computed case of tests/test_linkrank_host.py: 3 sources, 4 destinations, F = 2
#   scores   d0  d1  d2  d3        (destination rows 0 and 1 are identical)
#   s0        2   2   0  -1
#   s1        1   1   3  -2
#   s2       -2  -2   0   1
# known: (0, 3) twice, source 1 to every destination, (2, 2)
def test_reference_on_the_hand_computed_case():
    ninf = -np.inf
    idx, val = ref_topk(ZS, ZD, [0, 1, 2], 2, None)
    assert idx.tolist() == [[0, 1], [2, 0], [3, 2]]          # the tie of d0 and d1 comes out in index order
    assert val.tolist() == [[2.0, 2.0], [3.0, 1.0], [1.0, 0.0]]
    idx, val = ref_topk(ZS, ZD, [0, 1, 2], 2, KNOWN)
    assert idx.tolist() == [[0, 1], [-1, -1], [3, 0]]        # source 1 is known to everything; source 2 loses d2
    assert val.tolist() == [[2.0, 2.0], [ninf, ninf], [1.0, -2.0]]
    idx, val = ref_topk(ZS, ZD, [2, 0, 0, 1], 6, KNOWN)      # k > n_dst, a repeated source
    assert idx.tolist() == [[3, 0, 1, -1, -1, -1], [0, 1, 2, -1, -1, -1], [0, 1, 2, -1, -1, -1], [-1] * 6]
    assert val[0].tolist() == [1.0, -2.0, -2.0, ninf, ninf, ninf] and val[1].tolist() == [2.0, 2.0, 0.0] + [ninf] * 3
    idx, _ = ref_topk(ZS, ZD, [1], 6, None)
    assert idx.tolist() == [[2, 0, 1, 3, -1, -1]]


def test_public_surface():
    import hgin
    from hgin import linkpred
    assert "link_topk" in hgin.__all__ and hgin.link_topk is linkpred.link_topk
    assert callable(hgin.LinkPredictor.predict)
    for name in ("link_full_ranks", "link_full_metrics", "link_ranks", "link_metrics", "sampled_link_loss"):
        assert name in hgin.__all__ and getattr(hgin, name) is getattr(linkpred, name)
    assert callable(hgin.LinkPredictor.full_metrics) and callable(hgin.LinkPredictor.metrics)


def test_host_tensors_and_other_dtypes_are_refused():
    from hgin import linkpred
    z = torch.zeros(3, 4)
    src = torch.zeros(2, dtype=torch.long)
    known = torch.zeros(2, 2, dtype=torch.long)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        linkpred.link_topk(z, z, src, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        linkpred.link_topk(z, z, src, 2, known)
    with pytest.raises(TypeError, match=r"z_src must be float32 \(the fused link kernels are fp32 only\)"):
        linkpred.link_topk(z.bfloat16(), z, src, 2)
    with pytest.raises(TypeError, match=r"z_dst must be float32 \(the fused link kernels are fp32 only\)"):
        linkpred.link_topk(z, z.bfloat16(), src, 2)
    with pytest.raises(ValueError, match=r"src must be an int64 \[Q\] tensor"):
        linkpred.link_topk(z, z, known, 2)
    with pytest.raises(ValueError, match=r"src must be an int64 \[Q\] tensor"):
        linkpred.link_topk(z, z, src.int(), 2)


_Q = ctypes.c_void_p(16)   # a non-NULL pointer that must never be dereferenced


def _topk(lib, src=_Q, Q=4, n_src=5, n_dst=3, zs=_Q, lds=8, zd=_Q, ldd=8, F=8, rowptr=None, col=None, k=2, idx=_Q,
          score=_Q, ws=_Q, ws_bytes=1 << 20):
    return lib.hgin_link_topk_f32(src, Q, n_src, n_dst, zs, lds, zd, ldd, F, rowptr, col, k, idx, score, ws, ws_bytes,
                                  None)


def test_argument_errors_do_not_touch_the_device():
    from hgin import _lib
    lib = _lib.lib()
    err = lib.hgin_last_error
    assert lib.hgin_abi_version() == _lib.ABI_VERSION >= 11
    assert _topk(lib, Q=0) == -1 and b"n_query = 0" in err()
    assert _topk(lib, Q=1 << 31) == -1 and b"n_query = " in err()
    assert _topk(lib, n_src=0) == -1 and b"n_src" in err()
    assert _topk(lib, n_src=1 << 31) == -1 and b"n_src" in err()
    assert _topk(lib, n_dst=0) == -1 and b"n_dst" in err()
    assert _topk(lib, n_dst=1 << 31) == -1 and b"n_dst" in err()
    assert _topk(lib, F=0) == -1 and b"F " in err()
    assert _topk(lib, F=1 << 24, lds=1 << 24, ldd=1 << 24) == -1 and b"F " in err()
    assert _topk(lib, k=0) == -1 and b"k = 0" in err()
    assert _topk(lib, k=129) == -1 and b"k = 129" in err()
    assert _topk(lib, src=None) == -1 and b"src NULL" in err()
    assert _topk(lib, zs=None) == -1 and b"z_src NULL" in err()
    assert _topk(lib, zd=None) == -1 and b"z_dst NULL" in err()
    assert _topk(lib, lds=7) == -1 and b"leading dimension" in err()
    assert _topk(lib, ldd=7) == -1 and b"leading dimension" in err()
    assert _topk(lib, rowptr=_Q, col=None) == -1 and b"known_rowptr without known_col" in err()
    assert _topk(lib, idx=None) == -1 and b"top_idx NULL" in err()
    assert _topk(lib, score=None) == -1 and b"top_score NULL" in err()
    assert _topk(lib, ws_bytes=8) == -3 and b"workspace" in err()
    assert _topk(lib, ws=None) == -3 and b"workspace" in err()
    assert _topk(lib, k=128, n_dst=3, ws_bytes=8) == -3   # k may exceed n_dst: the next check is the workspace

    sz = ctypes.c_size_t(0)
    size = lib.hgin_link_topk_workspace_size
    # at least one split: 4 lists of k (score, index) entries and 4 counts per query
    assert size(1000, 300, 64, 10, ctypes.byref(sz)) == 0 and sz.value >= 1000 * 4 * (8 * 10 + 4)
    one = sz.value
    assert size(1000, 300, 64, 100, ctypes.byref(sz)) == 0 and 9 * one < sz.value < 11 * one   # linear in k
    assert size(1000, 300, 64, 10, None) == -1 and b"bytes" in err()
    assert size(0, 300, 64, 10, ctypes.byref(sz)) == -1 and b"n_query = 0" in err()
    assert size(1 << 31, 300, 64, 10, ctypes.byref(sz)) == -1 and b"n_query = " in err()
    assert size(1000, 0, 64, 10, ctypes.byref(sz)) == -1 and b"n_dst" in err()
    assert size(1000, 1 << 31, 64, 10, ctypes.byref(sz)) == -1 and b"n_dst" in err()
    assert size(1000, 300, 0, 10, ctypes.byref(sz)) == -1 and b"F " in err()
    assert size(1000, 300, 1 << 24, 10, ctypes.byref(sz)) == -1 and b"F " in err()
    assert size(1000, 300, 64, 0, ctypes.byref(sz)) == -1 and b"k = 0" in err()
    assert size(1000, 300, 64, 129, ctypes.byref(sz)) == -1 and b"k = 129" in err()


def test_bench_tool_plans_shapes_on_the_cpu_and_fails_without_a_gpu(capsys):
    import importlib.util
    import os

    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("bench_linktopk", os.path.join(ROOT, "tools", "bench_linktopk.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    shapes = tool.plan(["cfg2", "cfg3"], 65536, 1.0)
    assert [s["config"] for s in shapes] == ["cfg2", "cfg3"]
    s = shapes[1]
    assert (s["n_src"], s["n_dst"], s["E"], s["F"], s["Q"]) == (6_000_000, 3_000_000, 30_000_000, 256, 65536)
    assert s["flop"] == 2 * 65536 * 3_000_000 * 256 and s["ks"] == [10, 100]
    assert s["baseline_chunk_rows"] == (1 << 30) // (4 * 3_000_000)   # about 1 GB of fp32 scores per chunk
    assert shapes[0]["F"] == 128 and shapes[0]["n_dst"] == 300_000 and shapes[0]["Q"] == 65536
    assert tool.plan(["cfg1"], 65536, 1.0, ks=(5,))[0]["ks"] == [5]
    if not torch.cuda.is_available():
        rc = tool.main(["--configs", "cfg1", "--scale", "0.1", "--queries", "64"])
        err = capsys.readouterr().err
        assert rc == 2 and "no HIP device" in err and '"Q": 64' in err
