"""Full-candidate filtered link ranking (A15), host side (no GPU): this file's float64 reference (the one
tests/test_gpu_linkrank.py checks the kernels against) gives a hand-computed case, the metrics run on CPU counts, the
public surface exists, host tensors are refused, the two entry points reject bad arguments before touching the device,
and the bench tool plans its shapes on the CPU."""
import ctypes

import numpy as np
import torch


# ---------------------------------------------------------------------------------------------------
# float64 references (shared with tests/test_gpu_linkrank.py)
# ---------------------------------------------------------------------------------------------------
def candidate_mask(pos: np.ndarray, n_src: int, n_dst: int, known) -> np.ndarray:
    """bool [E, n_dst]: c is a candidate of query q = (s, d) when c != d and (s, c) is not in ``known``."""
    pos = np.asarray(pos)
    E = pos.shape[1]
    is_known = np.zeros((n_src, n_dst), dtype=bool)
    if known is not None:
        known = np.asarray(known)
        is_known[known[0], known[1]] = True
    mask = ~is_known[pos[0]]
    mask[np.arange(E), pos[1]] = False
    return mask


def ref_full_ranks(zs, zd, pos, known):
    """(n_greater, n_equal, n_cand), int64 [E], from float64 scores of every (query, destination)."""
    zs, zd, pos = np.asarray(zs, np.float64), np.asarray(zd, np.float64), np.asarray(pos)
    score = zs[pos[0]] @ zd.T
    thr = score[np.arange(pos.shape[1]), pos[1]][:, None]
    mask = candidate_mask(pos, zs.shape[0], zd.shape[0], known)
    return ((score > thr) & mask).sum(1), ((score == thr) & mask).sum(1), mask.sum(1)


def ref_full_ranks_chunked(zs, zd, pos, known, rows=2048):
    """``ref_full_ranks`` evaluated ``rows`` queries at a time and concatenated: the same counts (a query's counts
    depend on no other query) without the [E, n_dst] float64 score matrix of a large E."""
    pos = np.asarray(pos)
    parts = [ref_full_ranks(zs, zd, pos[:, i:i + rows], known) for i in range(0, pos.shape[1], rows)]
    return tuple(np.concatenate([p[j] for p in parts]) for j in range(3))


def ref_full_bands(zs, zd, pos, known):
    """Bounds that hold for every fp32 (or split) accumulation order: with b[q, c] = 2 F 2^-24 sum_f |zs[s, f]
    zd[c, f]|, returns (gt_lo, gt_hi, ge_lo, ge_hi, n_cand): n_greater lies in [gt_lo, gt_hi] = [#score > thr + b,
    #score > thr - b] and n_greater + n_equal in [ge_lo, ge_hi] = [#score > thr + b, #score >= thr - b]."""
    zs, zd, pos = np.asarray(zs, np.float64), np.asarray(zd, np.float64), np.asarray(pos)
    F = zs.shape[1]
    score = zs[pos[0]] @ zd.T
    b = 2.0 * F * 2.0 ** -24 * (np.abs(zs[pos[0]]) @ np.abs(zd).T)
    thr = score[np.arange(pos.shape[1]), pos[1]][:, None]
    mask = candidate_mask(pos, zs.shape[0], zd.shape[0], known)
    above, maybe = ((score > thr + b) & mask).sum(1), ((score > thr - b) & mask).sum(1)
    return above, maybe, above, ((score >= thr - b) & mask).sum(1), mask.sum(1)


def ref_full_metrics(n_greater, n_equal, n_cand) -> dict:
    gt, eq, nc = (np.asarray(v, np.float64) for v in (n_greater, n_equal, n_cand))
    above = gt + 0.5 * eq
    rank = 1.0 + above
    has = nc > 0
    out = {"auc": float((1.0 - above[has] / nc[has]).mean()), "mrr": float((1.0 / rank).mean())}
    for K in (1, 3, 10):
        out[f"hits@{K}"] = float((rank <= K).mean())
    return out


# ---------------------------------------------------------------------------------------------------
# the hand-computed case: 3 sources, 4 destinations, F = 2
#   scores   d0  d1  d2  d3        (destination rows 0 and 1 are identical)
#   s0        2   2   0  -1
#   s1        1   1   3  -2
#   s2       -2  -2   0   1
# queries (0 -> 0) thr 2, (1 -> 3) thr -2, (2 -> 0) thr -2, (1 -> 2) thr 3
# known: (0, 3) twice, source 1 to every destination, (2, 2)
ZS = [[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0]]
ZD = [[2.0, 1.0], [2.0, 1.0], [0.0, 3.0], [-1.0, -2.0]]
POS = [[0, 1, 2, 1], [0, 3, 0, 2]]
KNOWN = [[0, 0, 1, 1, 1, 1, 2], [3, 3, 0, 1, 2, 3, 2]]


def test_reference_on_the_hand_computed_case():
    gt, eq, nc = ref_full_ranks(ZS, ZD, POS, None)
    assert gt.tolist() == [0, 3, 2, 0] and eq.tolist() == [1, 0, 1, 0] and nc.tolist() == [3, 3, 3, 3]
    gt, eq, nc = ref_full_ranks(ZS, ZD, POS, KNOWN)
    # q0 loses d3 (listed twice, removed once); source 1 has no candidate left; q2 loses d2
    assert gt.tolist() == [0, 0, 1, 0] and eq.tolist() == [1, 0, 1, 0] and nc.tolist() == [2, 0, 2, 0]
    lo, hi, ge_lo, ge_hi, nc2 = ref_full_bands(ZS, ZD, POS, KNOWN)
    assert lo.tolist() == [0, 0, 1, 0] and hi.tolist() == [1, 0, 2, 0]   # the exact ties sit inside the band
    assert ge_lo.tolist() == lo.tolist() and ge_hi.tolist() == [1, 0, 2, 0] and nc2.tolist() == nc.tolist()
    m = ref_full_metrics(gt, eq, nc)   # ranks 1.5, 1, 2.5, 1; auc over q0 and q2 only: 0.75 and 0.25
    assert abs(m["mrr"] - (2 / 3 + 1 + 0.4 + 1) / 4) < 1e-15 and m["auc"] == 0.5
    assert m["hits@1"] == 0.5 and m["hits@3"] == 1.0 and m["hits@10"] == 1.0


def test_chunked_reference_equals_the_reference():
    """Chunks that do and do not divide E, a chunk of one query, one chunk for everything; with and without the
    filter (repeated known edges, a source connected to everything), on integers so that ties occur."""
    g = np.random.default_rng(17)
    E, n_src, n_dst, F = 203, 9, 37, 5
    zs = g.integers(-2, 3, (n_src, F)).astype(np.float32)
    zd = g.integers(-2, 3, (n_dst, F)).astype(np.float32)
    pos = np.stack([g.integers(0, n_src, E), g.integers(0, n_dst, E)])
    known = np.concatenate([pos[:, :120], pos[:, :40], np.stack([np.full(n_dst, 4), np.arange(n_dst)]),
                            np.stack([g.integers(0, n_src, 60), g.integers(0, n_dst, 60)])], 1)
    for kn in (None, known):
        want = ref_full_ranks(zs, zd, pos, kn)
        assert int(want[1].sum()) > 0 and int(want[0].sum()) > 0
        if kn is not None:
            assert int((want[2] == 0).sum()) > 0 and int(want[2].max()) < n_dst - 1
        for rows in (1, 7, 50, 203, 1000):
            got = ref_full_ranks_chunked(zs, zd, pos, kn, rows=rows)
            assert len(got) == 3
            for a, b in zip(got, want):
                assert a.shape == (E,) and a.dtype == b.dtype and np.array_equal(a, b), rows
    got = ref_full_ranks_chunked(ZS, ZD, POS, KNOWN, rows=3)
    assert [v.tolist() for v in got] == [[0, 0, 1, 0], [1, 0, 1, 0], [2, 0, 2, 0]]


def test_full_metrics_from_ranks_on_cpu_counts():
    from hgin.linkpred import full_metrics_from_ranks
    gt = torch.tensor([0, 4, 9, 0], dtype=torch.int32)
    eq = torch.tensor([0, 0, 2, 0], dtype=torch.int32)
    nc = torch.tensor([10, 8, 20, 0], dtype=torch.int32)   # the last query has no candidate: out of the auc
    m = full_metrics_from_ranks(gt, eq, nc)
    assert sorted(m) == ["auc", "hits@1", "hits@10", "hits@3", "mrr"]
    assert all(v.dtype == torch.float64 and v.dim() == 0 for v in m.values())
    assert abs(float(m["auc"]) - ((1.0 - 0.0) + (1.0 - 4 / 8) + (1.0 - 10 / 20)) / 3) < 1e-15
    assert abs(float(m["mrr"]) - (1 + 1 / 5 + 1 / 11 + 1) / 4) < 1e-15
    assert float(m["hits@1"]) == 0.5 and float(m["hits@3"]) == 0.5 and float(m["hits@10"]) == 0.75
    want = ref_full_metrics(gt.numpy(), eq.numpy(), nc.numpy())
    assert all(abs(float(m[k]) - want[k]) < 1e-15 for k in want)
    gt, eq, nc = (torch.as_tensor(v) for v in ref_full_ranks(ZS, ZD, POS, KNOWN))
    m, want = full_metrics_from_ranks(gt, eq, nc), ref_full_metrics(gt, eq, nc)
    assert all(abs(float(m[k]) - want[k]) < 1e-15 for k in want)


def test_public_surface():
    import hgin
    from hgin import linkpred
    for name in ("link_full_ranks", "link_full_metrics"):
        assert name in hgin.__all__ and getattr(hgin, name) is getattr(linkpred, name)
    assert callable(linkpred.full_metrics_from_ranks)
    assert callable(hgin.LinkPredictor.full_metrics)
    for name in ("link_ranks", "link_metrics"):   # the sampled pair stays
        assert name in hgin.__all__
    assert callable(hgin.LinkPredictor.metrics)


def test_host_tensors_and_other_dtypes_are_refused():
    import pytest

    from hgin import linkpred
    z = torch.zeros(3, 4)
    pos = torch.zeros(2, 2, dtype=torch.long)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        linkpred.link_full_ranks(z, z, pos)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        linkpred.link_full_ranks(z, z, pos, pos)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        linkpred.link_full_metrics(z, z, pos)


_Q = ctypes.c_void_p(16)   # a non-NULL pointer that must never be dereferenced


def _full(lib, pos=_Q, E=4, n_src=5, n_dst=3, zs=_Q, lds=8, zd=_Q, ldd=8, F=8, rowptr=None, col=None, gt=_Q, eq=_Q,
          nc=_Q, ws=_Q, ws_bytes=1 << 20):
    return lib.hgin_link_full_rank_f32(pos, E, n_src, n_dst, zs, lds, zd, ldd, F, rowptr, col, gt, eq, nc, ws,
                                       ws_bytes, None)


def test_argument_errors_do_not_touch_the_device():
    from hgin import _lib
    lib = _lib.lib()
    err = lib.hgin_last_error
    assert lib.hgin_abi_version() == _lib.ABI_VERSION >= 10
    assert _full(lib, E=0) == -1 and b"E = 0" in err()
    assert _full(lib, E=1 << 31) == -1 and b"E = " in err()
    assert _full(lib, n_src=0) == -1 and b"n_src" in err()
    assert _full(lib, n_src=1 << 31) == -1 and b"n_src" in err()
    assert _full(lib, n_dst=0) == -1 and b"n_dst" in err()
    assert _full(lib, n_dst=1 << 31) == -1 and b"n_dst" in err()
    assert _full(lib, F=0) == -1 and b"F " in err()
    assert _full(lib, F=1 << 24, lds=1 << 24, ldd=1 << 24) == -1 and b"F " in err()
    assert _full(lib, pos=None) == -1 and b"pos NULL" in err()
    assert _full(lib, zs=None) == -1 and b"z_src NULL" in err()
    assert _full(lib, zd=None) == -1 and b"z_dst NULL" in err()
    assert _full(lib, lds=7) == -1 and b"leading dimension" in err()
    assert _full(lib, ldd=7) == -1 and b"leading dimension" in err()
    assert _full(lib, rowptr=_Q, col=None) == -1 and b"known_rowptr without known_col" in err()
    assert _full(lib, gt=None) == -1 and b"n_greater NULL" in err()
    assert _full(lib, eq=None) == -1 and b"n_equal NULL" in err()
    assert _full(lib, nc=None) == -1 and b"n_cand NULL" in err()
    assert _full(lib, ws_bytes=8) == -3 and b"workspace" in err()
    assert _full(lib, ws=None) == -3 and b"workspace" in err()

    sz = ctypes.c_size_t(0)
    size = lib.hgin_link_full_rank_workspace_size
    assert size(1000, 300, 64, ctypes.byref(sz)) == 0 and sz.value >= 4000
    assert size(1000, 300, 64, None) == -1 and b"bytes" in err()
    assert size(0, 300, 64, ctypes.byref(sz)) == -1 and b"E = 0" in err()
    assert size(1 << 31, 300, 64, ctypes.byref(sz)) == -1 and b"E = " in err()
    assert size(1000, 0, 64, ctypes.byref(sz)) == -1 and b"n_dst" in err()
    assert size(1000, 1 << 31, 64, ctypes.byref(sz)) == -1 and b"n_dst" in err()
    assert size(1000, 300, 0, ctypes.byref(sz)) == -1 and b"F " in err()
    assert size(1000, 300, 1 << 24, ctypes.byref(sz)) == -1 and b"F " in err()


def test_bench_tool_plans_shapes_on_the_cpu_and_fails_without_a_gpu(capsys):
    import importlib.util
    import os

    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("bench_linkrank", os.path.join(ROOT, "tools", "bench_linkrank.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    shapes = tool.plan(["cfg2", "cfg3"], 65536, 1.0)
    assert [s["config"] for s in shapes] == ["cfg2", "cfg3"]
    s = shapes[1]
    assert (s["n_src"], s["n_dst"], s["E"], s["F"], s["Q"]) == (6_000_000, 3_000_000, 30_000_000, 256, 65536)
    assert s["flop"] == 2 * 65536 * 3_000_000 * 256
    assert s["baseline_chunk_rows"] == (1 << 30) // (4 * 3_000_000)   # about 1 GB of fp32 scores per chunk
    assert shapes[0]["F"] == 128 and shapes[0]["n_dst"] == 300_000 and shapes[0]["Q"] == 65536
    assert tool.plan(["cfg1"], 65536, 1.0)[0]["Q"] == 2000   # never more queries than the relation has positives
    if not torch.cuda.is_available():
        rc = tool.main(["--configs", "cfg1", "--scale", "0.1", "--queries", "64"])
        err = capsys.readouterr().err
        assert rc == 2 and "no HIP device" in err and '"Q": 64' in err
