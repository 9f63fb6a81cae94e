"""Graph-local candidates for the full softmax link loss (A24), host side (no GPU): the four entry points exist, refuse
bad arguments before touching the device and ask for at least the unsegmented workspace; the Python surface refuses a
``segments`` that is no ``LinkSegments``, one with other row counts and a positive that leaves its graph; and the
float64 restatement the GPU tests use (tests/test_linklse_host.py's ``ref_lse`` / ``ref_lse_grads`` with ``known``
augmented by every (source, out-of-segment destination) pair, ``augment_known``) equals a segmented reference written
directly as a loop over the graphs."""
import ctypes

import numpy as np
import pytest
import torch

from test_linklse_host import ref_lse, ref_lse_grads, ref_lse_tol

_Q = ctypes.c_void_p(16)   # a non-NULL pointer that must never be dereferenced
_F = ctypes.c_float


# ---------------------------------------------------------------------------------------------------
# float64 restatement (shared with tests/test_gpu_linklse_seg.py)
# ---------------------------------------------------------------------------------------------------
def dst_ptr_of(sizes) -> np.ndarray:
    """int64 [G + 1]: the destination blocks of graphs with ``sizes`` destinations each."""
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64))])


def augment_known(src, src_seg, dst_ptr, known=None) -> np.ndarray:
    """int64 [2, M]: ``known`` plus, for every source of ``src``, every destination outside its graph's block
    [dst_ptr[g], dst_ptr[g + 1]).  A23's candidates under this known set are A24's candidates."""
    src, src_seg, dst_ptr = np.asarray(src), np.asarray(src_seg), np.asarray(dst_ptr)
    n_dst = int(dst_ptr[-1])
    cols = np.arange(n_dst)
    parts = [np.zeros((2, 0), np.int64)] if known is None else [np.asarray(known, np.int64).reshape(2, -1)]
    for s in src:
        g = int(src_seg[s])
        out = cols[(cols < dst_ptr[g]) | (cols >= dst_ptr[g + 1])]
        parts.append(np.stack([np.full(out.size, s, np.int64), out]))
    return np.concatenate(parts, 1)


def ref_seg_direct(zs, zd, src, g_up, src_seg, dst_ptr, temperature=1.0, known=None):
    """(lse [Q], G_src [n_src, F], G_dst [n_dst, F]) in float64, graph by graph: the queries of graph g against the
    destination rows of graph g alone, with the known edges that stay inside it."""
    zs, zd = np.asarray(zs, np.float64), np.asarray(zd, np.float64)
    src, g_up, src_seg, dst_ptr = np.asarray(src), np.asarray(g_up, np.float64), np.asarray(src_seg), np.asarray(dst_ptr)
    lse = np.full(src.size, -np.inf)
    G_src, G_dst = np.zeros_like(zs), np.zeros_like(zd)
    for g in range(dst_ptr.size - 1):
        lo, hi = int(dst_ptr[g]), int(dst_ptr[g + 1])
        mine = np.flatnonzero(src_seg[src] == g)
        if mine.size == 0 or hi == lo:
            continue
        kn = None
        if known is not None:
            known = np.asarray(known)
            keep = (known[1] >= lo) & (known[1] < hi)
            kn = np.stack([known[0, keep], known[1, keep] - lo])
        lse[mine] = ref_lse(zs, zd[lo:hi], src[mine], temperature, kn)
        gs, gd, _, _ = ref_lse_grads(zs, zd[lo:hi], src[mine], g_up[mine], temperature, kn)
        G_src += gs
        G_dst[lo:hi] += gd
    return lse, G_src, G_dst


def test_augmented_known_is_the_segmented_reference():
    g = np.random.default_rng(24)
    sizes = (1, 126, 1, 0, 172)
    ptr = dst_ptr_of(sizes)
    n_src, n_dst, F, Q = 60, int(ptr[-1]), 5, 41
    zs, zd = g.standard_normal((n_src, F)), g.standard_normal((n_dst, F))
    src_seg = g.integers(0, len(sizes), n_src)
    src_seg[:5] = np.arange(5)                  # every graph has a source, the empty graph 3 too
    src = np.concatenate([np.arange(5), 5 + g.permutation(n_src - 5)[:Q - 5]])
    g_up = g.standard_normal(Q)
    some = g.integers(0, n_src, 200)
    known = np.stack([some, g.integers(0, n_dst, 200)])
    one = int(np.flatnonzero(src_seg == 1)[0])    # a source that knows its whole graph (and a few rows outside it)
    known = np.concatenate([known, np.stack([np.full(130, one), np.arange(0, 130)])], 1)
    for kn, T in ((None, 1.0), (known, 0.7)):
        want_lse, want_s, want_d = ref_seg_direct(zs, zd, src, g_up, src_seg, ptr, T, kn)
        aug = augment_known(src, src_seg, ptr, kn)
        got_lse = ref_lse(zs, zd, src, T, aug)
        got_s, got_d, A_s, A_d = ref_lse_grads(zs, zd, src, g_up, T, aug)
        assert np.array_equal(np.isneginf(want_lse), np.isneginf(got_lse))
        fin = np.isfinite(want_lse)
        assert np.isneginf(want_lse[src_seg[src] == 3]).all() and fin.sum() > Q // 2
        if kn is not None:
            assert np.isneginf(want_lse[src == one]).all()
        assert np.abs(got_lse[fin] - want_lse[fin]).max() <= 1e-12
        assert np.abs(got_s - want_s).max() <= 1e-12 and np.abs(got_d - want_d).max() <= 1e-12
        # what nothing contributes to: sources without a candidate, destinations of a graph without a query
        assert (got_s[src[~fin]] == 0.0).all() and (A_s[src[~fin]] == 0.0).all()
        tol = ref_lse_tol(zs, zd, src, T, aug)
        assert (tol[~fin] == 0.0).all() and (tol[fin] > 0.0).all()
    # one graph: nothing is added
    assert augment_known(src, np.zeros(n_src, np.int64), dst_ptr_of([n_dst]), known).shape == known.shape


# ---------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------
def test_public_surface():
    import inspect

    import hgin
    from hgin import _lib, linkpred
    lib = _lib.lib()
    assert lib.hgin_abi_version() == _lib.ABI_VERSION == 16
    i64, p, sz, f32 = ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_float
    a23_fwd = [p, i64, i64, i64, p, i64, p, i64, i64, f32, p, p, p, p, sz]
    a23_bwd = [p, i64, i64, i64, p, i64, p, i64, i64, f32, p, p, p, p, p, i64, p, sz]
    seg = [p, p, i64, p]                           # src_seg, dst_ptr, n_graphs before stream
    want = {"hgin_link_lse_seg_workspace_size": [i64, i64, i64, ctypes.POINTER(sz)],
            "hgin_link_lse_fwd_seg_f32": a23_fwd + seg,
            "hgin_link_lse_bwd_src_seg_f32": a23_bwd + seg,
            "hgin_link_lse_bwd_dst_seg_f32": a23_bwd + seg}
    for name, args in want.items():
        assert name in _lib.exported_symbols() and hasattr(lib, name), name
        assert _lib._SIGS[name] == (args, ctypes.c_int), name
    # the unsegmented signatures are the segmented ones without the segmentation
    assert _lib._SIGS["hgin_link_lse_fwd_f32"][0] == a23_fwd + [p]
    assert _lib._SIGS["hgin_link_lse_bwd_dst_f32"][0] == a23_bwd + [p]
    for fn in (linkpred.link_lse, linkpred.link_lse_unfused, linkpred.full_softmax_link_loss,
               hgin.LinkPredictor.full_loss):
        par = inspect.signature(fn).parameters
        assert "segments" in par and par["segments"].default is None, fn
    assert list(inspect.signature(linkpred.link_lse).parameters) == ["z_src", "z_dst", "src", "temperature", "known",
                                                                     "segments"]


def _fwd(lib, src=_Q, Q=4, n_src=5, n_dst=300, zs=_Q, lds=8, zd=_Q, ldd=8, F=8, inv_t=1.0, rowptr=None, col=None,
         lse=_Q, ws=_Q, ws_bytes=1 << 20, src_seg=_Q, dst_ptr=_Q, n_graphs=3):
    return lib.hgin_link_lse_fwd_seg_f32(src, Q, n_src, n_dst, zs, lds, zd, ldd, F, _F(inv_t), rowptr, col, lse, ws,
                                         ws_bytes, src_seg, dst_ptr, n_graphs, None)


def _bwd(fn, src=_Q, Q=4, n_src=5, n_dst=300, zs=_Q, lds=8, zd=_Q, ldd=8, F=8, inv_t=1.0, rowptr=None, col=None,
         lse=_Q, g=_Q, out=_Q, ldo=8, ws=_Q, ws_bytes=1 << 20, src_seg=_Q, dst_ptr=_Q, n_graphs=3):
    return fn(src, Q, n_src, n_dst, zs, lds, zd, ldd, F, _F(inv_t), rowptr, col, lse, g, out, ldo, ws, ws_bytes, src_seg,
              dst_ptr, n_graphs, None)


def test_argument_errors_do_not_touch_the_device():
    """Every pointer is 16: a launch, or any host read of an operand, would fault."""
    from hgin import _lib
    lib = _lib.lib()
    err = lib.hgin_last_error
    calls = [lambda **kw: _fwd(lib, **kw), lambda **kw: _bwd(lib.hgin_link_lse_bwd_src_seg_f32, **kw),
             lambda **kw: _bwd(lib.hgin_link_lse_bwd_dst_seg_f32, **kw)]
    names = [b"hgin_link_lse_fwd_seg_f32", b"hgin_link_lse_bwd_src_seg_f32", b"hgin_link_lse_bwd_dst_seg_f32"]
    for call, name in zip(calls, names):
        # A24's own refusals
        assert call(src_seg=None) == -1 and b"src_seg NULL" in err() and name in err()
        assert call(dst_ptr=None) == -1 and b"dst_ptr NULL" in err()
        assert call(n_graphs=0) == -1 and b"n_graphs = 0" in err()
        assert call(n_graphs=-2) == -1 and b"n_graphs = -2" in err()
        assert call(n_graphs=1 << 31) == -1 and b"n_graphs = " in err()
        # every refusal of A23
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
    # the segmented bwd_dst keeps the query blocks' ranges in the workspace even where it has one split and no partials
    # (4 queries: one block): the unsegmented call needs no workspace there, this one does
    assert calls[2](ws=None) == -3 and b"workspace" in err()
    assert calls[2](ws_bytes=4) == -3 and b"workspace" in err()


def test_seg_workspace_covers_the_unsegmented_one():
    from hgin import _lib
    lib = _lib.lib()
    err = lib.hgin_last_error
    size, seg_size = lib.hgin_link_lse_workspace_size, lib.hgin_link_lse_seg_workspace_size
    a, b = ctypes.c_size_t(0), ctypes.c_size_t(0)
    for Q, n_dst, F in ((4, 300, 8), (300, 4, 8), (1, 1, 1), (129, 300, 36), (32768, 600, 8), (4096, 300_000, 256),
                        (100, 120, 8), (64, 1 << 20, 1 << 23)):
        assert size(Q, n_dst, F, ctypes.byref(a)) == 0 and seg_size(Q, n_dst, F, ctypes.byref(b)) == 0
        assert b.value >= a.value and b.value >= 8 * -(-Q // 128), (Q, n_dst, F)
    # (300, 4, 8): the g_dst partials (3 splits x 4 rows x 8 floats) are the largest need; the ranges sit behind them
    assert size(300, 4, 8, ctypes.byref(a)) == 0 and seg_size(300, 4, 8, ctypes.byref(b)) == 0
    assert b.value >= 3 * 4 * 8 * 4 + 3 * 8
    assert seg_size(4, 300, 8, None) == -1 and b"bytes" in err()
    assert seg_size(0, 300, 8, ctypes.byref(b)) == -1 and b"n_query = 0" in err()
    assert seg_size(4, 0, 8, ctypes.byref(b)) == -1 and b"n_dst" in err()
    assert seg_size(4, 300, 0, ctypes.byref(b)) == -1 and b"F " in err()
    assert seg_size(128, 1 << 20, 1 << 23, ctypes.byref(b)) == -1 and b"split partials of g_src" in err()


# ---------------------------------------------------------------------------------------------------
# Python refusals (CPU tensors: everything below is decided before a device is needed)
# ---------------------------------------------------------------------------------------------------
def test_python_refusals():
    from hgin import linkpred
    from hgin.linkpred import LinkSegments
    zs, zd = torch.zeros(3, 4), torch.zeros(5, 4)
    src = torch.tensor([0, 2])
    seg = LinkSegments(torch.tensor([0, 1, 1]), torch.tensor([0, 0, 1, 1, 1]))
    for fn in (linkpred.link_lse, linkpred.link_lse_unfused):
        with pytest.raises(TypeError, match="segments must be a LinkSegments, got tuple"):
            fn(zs, zd, src, segments=(seg.src_seg, seg.dst_ptr))
        with pytest.raises(ValueError, match="segments cover 3 source rows, z_src has 4"):
            fn(torch.zeros(4, 4), zd, src, segments=seg)
        with pytest.raises(ValueError, match="segments cover 5 destination rows, expected 6"):
            fn(zs, torch.zeros(6, 4), src, segments=seg)
        with pytest.raises(RuntimeError, match="no CPU fallback"):     # a good segmentation gets as far as the device check
            fn(zs, zd, src, segments=seg)
        with pytest.raises(ValueError, match="distinct"):
            fn(zs, zd, torch.tensor([1, 1]), segments=seg)
    pos = torch.tensor([[0, 1, 2], [1, 2, 4]])
    with pytest.raises(TypeError, match="segments must be a LinkSegments"):
        linkpred.full_softmax_link_loss(zs, zd, pos, segments=3)
    with pytest.raises(ValueError, match="segments cover 5 destination rows"):
        linkpred.full_softmax_link_loss(zs, torch.zeros(7, 4), pos, segments=seg)
    with pytest.raises(ValueError, match="a positive's destination lies outside its source's graph"):
        linkpred.full_softmax_link_loss(zs, zd, torch.tensor([[0, 1], [1, 1]]), segments=seg)     # 1 -> 1 leaves graph 1
    with pytest.raises(IndexError, match="pos src index out of range"):
        linkpred.full_softmax_link_loss(zs, zd, torch.tensor([[0, 3], [1, 2]]), segments=seg)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        linkpred.full_softmax_link_loss(zs, zd, pos, segments=seg)

    class Model:
        def encode(self, x, e):
            raise AssertionError("refused before any encode")

    rel = ("a", "to", "b")
    with pytest.raises(TypeError, match="segments must be a LinkSegments"):
        linkpred.LinkPredictor(Model(), rel, 1, 0).full_loss(None, segments="graphs")
    lp = linkpred.LinkPredictor(Model(), rel, 1, 0, graph_local=True)     # segments= is the way in; this stays refused
    with pytest.raises(ValueError, match="hard > 0 and graph_local = True are not supported"):
        lp.full_loss(None, segments=seg)


def test_bench_tool_plans_the_graph_cut_on_the_cpu():
    import importlib.util
    import os

    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("bench_linklse", os.path.join(ROOT, "tools", "bench_linklse.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    shape = tool.plan()[4]
    assert shape["name"] == "cfg2" and shape["known_degree"] == 0
    cut = tool.seg_plan(shape, 8)
    assert cut["graphs"] == 8 and cut["n_dst"] == shape["n_dst"] - shape["n_dst"] % 8
    assert cut["Q"] == shape["Q"] - shape["Q"] % 8 and cut["n_src"] == shape["n_src"] - shape["n_src"] % 8
    assert cut["dst_per_graph"] * 8 == cut["n_dst"] and cut["queries_per_graph"] * 8 == cut["Q"]
    assert cut["flop_seg"]["total"] * 8 == cut["flop"]["total"]
    with pytest.raises(ValueError, match="graphs"):
        tool.seg_plan(shape, 0)
