"""Sampled negatives drawn from each source's non-neighbours (include/hgin.h A20, ``known=``), host side (no GPU):
this file's numpy restatement of the filtered draw (the one tests/test_gpu_linkfilt.py checks the kernels against)
agrees with the segmented reference and the C oracle's sampler for an empty known set, gives the header's hand case,
maps r = 0 .. f - 1 increasingly onto exactly the complement of random rows, and keeps the unfiltered draw where the
window holds nothing but neighbours; the Python surface, the header section and the three entry points exist; the entry
points reject bad arguments before touching the device; a malformed ``known`` is refused before a device is needed; the
predictor passes ``known`` only when asked to; and the bench tool's plan is unchanged without ``--filter``."""
import ctypes
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

from test_linkseg_host import ref_seg_draws

_Q = ctypes.c_void_p(16)   # a non-NULL pointer that must never be dereferenced


# ---------------------------------------------------------------------------------------------------
# references (shared with tests/test_gpu_linkfilt.py)
# ---------------------------------------------------------------------------------------------------
def known_csr_np(known, n_src: int, n_dst: int):
    """(rowptr int64 [n_src + 1], col int64): ``known`` (an edge index [2, M]) by source, columns strictly increasing
    within a row (duplicates removed)."""
    known = np.asarray(known).reshape(2, -1)
    pairs = np.unique(known[0].astype(np.int64) * n_dst + known[1])
    rowptr = np.zeros(n_src + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(pairs // n_dst, minlength=n_src))
    return rowptr, pairs % n_dst


def filt_map(r: int, lo: int, cols) -> int:
    """The r-th (0-based) destination of a window starting at ``lo`` that is not one of ``cols`` (the window's known
    columns, strictly increasing): lo + r + j with j the smallest index such that (cols[j] - lo) - j > r."""
    j = 0
    while j < len(cols) and (int(cols[j]) - lo) - j <= r:
        j += 1
    return lo + r + j


def ref_filt_draws(seed: int, offset: int, src, k: int, src_seg, dst_ptr, known_rowptr, known_col) -> np.ndarray:
    """int32 [E * k]: ``ref_seg_draws`` with every draw taken from the window minus the known row of its source.
    ``src_seg`` None: one pool [0, dst_ptr[-1]).  Philox counter, block, word and key as ``ref_seg_draws``; with f free
    destinations in the window the draw is the hi32(word * f)-th of them, and the unfiltered lo + hi32(word * n) when
    f == 0."""
    from oracle import c_oracle
    src, dst_ptr = np.asarray(src), np.asarray(dst_ptr)
    known_rowptr, known_col = np.asarray(known_rowptr), np.asarray(known_col)
    key = [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]
    out = np.zeros(len(src) * k, np.int32)
    blocks, rows = {}, {}
    for i in range(len(src) * k):
        c = (offset + i) & (2**64 - 1)
        b = c >> 2
        if b not in blocks:
            blocks[b] = c_oracle.philox4x32_10([b & 0xFFFFFFFF, b >> 32, 0, 0], key)
        s = int(src[i // k])
        if s not in rows:
            g = 0 if src_seg is None else int(src_seg[s])
            lo, n = int(dst_ptr[g]), int(dst_ptr[g + 1] - dst_ptr[g])
            row = known_col[int(known_rowptr[s]):int(known_rowptr[s + 1])]
            rows[s] = (lo, n, row[(row >= lo) & (row < lo + n)])
        lo, n, cols = rows[s]
        w, f = int(blocks[b][c & 3]), n - len(cols)
        out[i] = lo + ((w * n) >> 32) if f == 0 else filt_map((w * f) >> 32, lo, cols)
    return out


# ---------------------------------------------------------------------------------------------------
# the draw
# ---------------------------------------------------------------------------------------------------
SEGS = ([2, 0, 1, 0, 2, 1, 0], [0, 4, 5, 53])


@pytest.mark.parametrize("offset", [0, 6, 2**32 + 1])
@pytest.mark.parametrize("k", [1, 3, 5])
def test_an_empty_known_set_gives_the_segmented_and_the_oracle_draws(k, offset):
    from oracle import c_oracle
    seed, E = 0x1234ABCD5678, 23
    src = np.arange(E) % 7
    empty = (np.zeros(8, np.int64), np.zeros(0, np.int64))
    got = ref_filt_draws(seed, offset, src, k, *SEGS, *empty)
    assert np.array_equal(got, ref_seg_draws(seed, offset, src, k, *SEGS))
    one = ref_filt_draws(seed, offset, src, k, None, [0, 53], *empty)
    assert np.array_equal(one, c_oracle.neg_sample(seed, offset, E * k, 53))
    assert np.array_equal(one, ref_filt_draws(seed, offset, src, k, np.zeros(7, np.int32), [0, 53], *empty))


def test_the_hand_case_of_the_header():
    """Window [10, 16), known columns {11, 12, 15} (and 3, 40 outside the window): free = {10, 13, 14}; seed 0, offset
    0 uses Random123's known-answer block, whose words give r = 1, 2, 2, 1."""
    from oracle import c_oracle
    words = [int(v) for v in c_oracle.philox4x32_10([0, 0, 0, 0], [0, 0])]
    assert words == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert [(w * 3) >> 32 for w in words] == [1, 2, 2, 1]
    got = ref_filt_draws(0, 0, [0], 4, [1], [0, 10, 16, 50], [0, 5], [3, 11, 12, 15, 40])
    assert got.tolist() == [13, 14, 14, 13]
    # one draw each for four positives of the same source: the same counters, the same draws
    assert ref_filt_draws(0, 0, [0, 0, 0, 0], 1, [1], [0, 10, 16, 50], [0, 5], [3, 11, 12, 15, 40]).tolist() == \
        [13, 14, 14, 13]


def test_the_map_is_increasing_onto_exactly_the_complement():
    rng = np.random.default_rng(5)
    for _ in range(300):
        lo, n = int(rng.integers(0, 20)), int(rng.integers(1, 40))
        cols = np.sort(rng.choice(np.arange(lo, lo + n), size=int(rng.integers(0, n)), replace=False))
        free = [c for c in range(lo, lo + n) if c not in set(cols.tolist())]
        assert [filt_map(r, lo, cols) for r in range(len(free))] == free
    # through the draw: every word lands on a free destination, and all of them are reached
    n_dst, rowptr, col = 12, [0, 7], [0, 1, 4, 5, 6, 9, 11]
    got = ref_filt_draws(3, 0, [0], 400, None, [0, n_dst], rowptr, col)
    assert sorted(set(got.tolist())) == [2, 3, 7, 8, 10]


def test_a_window_of_neighbours_only_keeps_the_unfiltered_draw():
    seed, k = 11, 6
    src_seg, ptr = [0, 1], [0, 5, 9]
    rowptr, col = known_csr_np([[1] * 6, [5, 6, 7, 8, 0, 2]], 2, 9)    # source 1: all of its graph, and two outside
    got = ref_filt_draws(seed, 0, [1, 0], k, src_seg, ptr, rowptr, col)
    assert np.array_equal(got, ref_seg_draws(seed, 0, [1, 0], k, src_seg, ptr))
    assert set(got[:k].tolist()) <= {5, 6, 7, 8}


# ---------------------------------------------------------------------------------------------------
# surface, header
# ---------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("hgin_neg_sample_filt", "hgin_link_loss_fwd_filt_f32", "hgin_link_rank_filt_f32")


def test_public_surface():
    from hgin import linkpred
    for fn in (linkpred.negative_edges, linkpred.link_loss, linkpred.sampled_link_loss, linkpred.link_ranks,
               linkpred.link_metrics):
        params = inspect.signature(fn).parameters
        assert list(params)[-1] == "known" and params["known"].default is None, fn.__name__
    init = inspect.signature(linkpred.LinkPredictor.__init__).parameters
    assert init["filter_negatives"].default is False
    for fn in (linkpred.LinkPredictor.loss, linkpred.LinkPredictor.metrics):
        assert inspect.signature(fn).parameters["known"].default is None
    # the mining functions keep their pinned parameter lists
    assert list(inspect.signature(linkpred.hard_negatives).parameters) == ["z_src", "z_dst", "pos", "m", "known", "seed",
                                                                           "offset"]
    assert list(inspect.signature(linkpred.hard_negatives_seg).parameters) == ["z_src", "z_dst", "pos", "m", "segments",
                                                                               "known", "seed", "offset"]
    assert "not filtered" in linkpred.hard_negatives.__doc__ and "A20" in linkpred.hard_negatives.__doc__


def test_abi_15_and_the_header_section():
    from conftest import ROOT
    from hgin import _lib
    assert _lib.ABI_VERSION >= 15
    assert _lib.lib().hgin_abi_version() == _lib.ABI_VERSION
    text = open(os.path.join(ROOT, "include", "hgin.h")).read()
    assert int(re.search(r"#define HGIN_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION
    a20 = text[text.index("---- A20"):]
    a20 = a20[:a20.index("---- F4")]
    for name in NEW_SYMBOLS:
        assert name in _lib.exported_symbols() and hasattr(_lib.lib(), name), name
        assert re.search(r"\bint " + name + r"\(", a20), name
    for word in ("known_rowptr", "r = hi32(w * f)", "lo + r + j", "f == 0", "13, 14, 14, 13", "6627e8d5", ",FILT",
                 "not filtered"):
        assert word in a20, word
    declared = set(re.findall(r"^(?:int|size_t|const char\*) (hgin_\w+)\(", text, re.M))
    assert declared == set(_lib.exported_symbols())


# ---------------------------------------------------------------------------------------------------
# C argument checks: HGIN_E_ARG before any launch
# ---------------------------------------------------------------------------------------------------
def _sample(lib, src=_Q, E=4, k=2, n_dst=3, seg=_Q, ptr=_Q, G=3, n_src=5, rowptr=_Q, col=_Q, out=_Q):
    return lib.hgin_neg_sample_filt(1, 0, src, E, k, n_dst, seg, ptr, G, n_src, rowptr, col, out, None)


def _fwd(lib, pos=_Q, E=4, k=2, n_dst=3, neg_dst=None, m=0, zs=_Q, zd=_Q, F=8, coef=_Q, neg=_Q, loss=_Q, ws=_Q,
         ws_bytes=1 << 20, objective=0, param=1.0, seg=_Q, ptr=_Q, G=3, n_src=5, rowptr=_Q, col=_Q):
    return lib.hgin_link_loss_fwd_filt_f32(pos, E, k, 1, 0, n_dst, neg_dst, m, zs, F, zd, F, F, coef, neg, loss, ws,
                                           ws_bytes, objective, param, seg, ptr, G, n_src, rowptr, col, None)


def _rank(lib, pos=_Q, E=4, k=2, n_dst=3, neg_dst=None, m=0, zs=_Q, zd=_Q, F=8, gt=_Q, eq=_Q, seg=_Q, ptr=_Q, G=3,
          n_src=5, rowptr=_Q, col=_Q):
    return lib.hgin_link_rank_filt_f32(pos, E, k, 1, 0, n_dst, neg_dst, m, zs, F, zd, F, F, gt, eq, seg, ptr, G, n_src,
                                       rowptr, col, None)


def test_argument_errors_do_not_touch_the_device():
    from hgin import _lib
    lib = _lib.lib()
    err = lib.hgin_last_error
    for call in (_sample, _fwd, _rank):
        # the known CSR and the source row count
        assert call(lib, col=None) == -1 and b"known_rowptr without known_col" in err(), call.__name__
        assert call(lib, rowptr=None) == -1 and b"known_col without known_rowptr" in err(), call.__name__
        assert call(lib, n_src=0) == -1 and b"n_src = 0" in err(), call.__name__
        assert call(lib, n_src=1 << 31) == -1 and b"n_src" in err(), call.__name__
        # the segmentation: both pointers with n_graphs >= 1, neither with n_graphs = 0
        assert call(lib, seg=None) == -1 and b"src_seg NULL" in err(), call.__name__
        assert call(lib, ptr=None) == -1 and b"dst_ptr NULL" in err(), call.__name__
        assert call(lib, G=0) == -1 and b"n_graphs = 0" in err(), call.__name__
        assert call(lib, G=-1) == -1 and b"n_graphs = -1" in err(), call.__name__
        assert call(lib, G=1 << 31) == -1 and b"n_graphs" in err(), call.__name__
        assert call(lib, n_dst=0) == -1 and b"n_dst" in err(), call.__name__
    # the sampler
    assert _sample(lib, E=-1) == -1 and b"E = -1" in err()
    assert _sample(lib, k=-1) == -1 and b"k = -1" in err()
    assert _sample(lib, E=1 << 20, k=1 << 11) == -1 and b"E * k" in err()
    assert _sample(lib, src=None) == -1 and b"src NULL" in err()
    assert _sample(lib, out=None) == -1 and b"out NULL" in err()
    assert _sample(lib, E=0, src=None, out=None) == 0 and _sample(lib, k=0, src=None, out=None) == 0   # nothing to draw
    assert _sample(lib, E=0, seg=None, ptr=None, G=0, rowptr=None, col=None) == 0      # one pool, no known edges
    # loss and ranks: the A13 ranges without a set, the A18 ranges with one
    for call in (_fwd, _rank):
        assert call(lib, E=0) == -1 and b"E = 0" in err()
        assert call(lib, k=0) == -1 and b"k = 0 must be >= 1" in err()
        assert call(lib, m=-1) == -1 and b"m = -1 must be >= 0" in err()
        assert call(lib, m=2, neg_dst=None) == -1 and b"neg_dst NULL" in err()
        assert call(lib, k=-1, m=2, neg_dst=_Q) == -1 and b"k = -1 must be >= 0" in err()
        assert call(lib, E=1 << 20, k=1 << 10, m=1 << 10, neg_dst=_Q) == -1 and b"E * (k + m)" in err()
        assert call(lib, F=1 << 24) == -1 and b"F " in err()
        assert call(lib, pos=None) == -1 and b"pos NULL" in err()
        assert call(lib, zs=None) == -1 and b"z_src NULL" in err()
        assert call(lib, zd=None) == -1 and b"z_dst NULL" in err()
        # legal shapes (k = 0 with a set; one pool): the error that comes back is the later one
        assert call(lib, k=0, m=2, neg_dst=_Q, col=None) == -1 and b"known_rowptr without known_col" in err()
        assert call(lib, seg=None, ptr=None, G=0, n_src=0) == -1 and b"n_src = 0" in err()
    assert _fwd(lib, coef=None) == -1 and b"coef NULL" in err()
    assert _fwd(lib, neg=None) == -1 and b"neg NULL" in err()
    assert _fwd(lib, loss=None) == -1 and b"loss NULL" in err()
    assert _rank(lib, gt=None) == -1 and b"n_greater NULL" in err()
    assert _rank(lib, eq=None) == -1 and b"n_equal NULL" in err()
    for obj in range(4):
        assert _fwd(lib, objective=obj, ws_bytes=8) == -3 and b"workspace" in err()
        assert _fwd(lib, objective=obj, ws=None) == -3 and b"workspace" in err()
    for bad in (-1, 4):
        assert _fwd(lib, objective=bad) == -1 and b"objective" in err()
    assert _fwd(lib, objective=1, param=0.0) == -1 and b"temperature" in err()
    assert _fwd(lib, objective=3, param=-1.0) == -1 and b"alpha" in err()


# ---------------------------------------------------------------------------------------------------
# the Python layer refuses a malformed known before a device is needed
# ---------------------------------------------------------------------------------------------------
POS = [[0, 1, 2, 3, 0], [0, 3, 5, 2, 2]]


def test_python_refusals_before_any_device_is_needed():
    from hgin import linkpred
    zs, zd, pos = torch.zeros(4, 4), torch.zeros(6, 4), torch.tensor(POS)
    fns = {"sampled_link_loss": lambda **kw: linkpred.sampled_link_loss(zs, zd, pos, 1, 0, **kw),
           "link_loss": lambda **kw: linkpred.link_loss(zs, zd, pos, 1, 0, **kw),
           "link_ranks": lambda **kw: linkpred.link_ranks(zs, zd, pos, 1, 0, **kw),
           "link_metrics": lambda **kw: linkpred.link_metrics(zs, zd, pos, 1, 0, **kw),
           "negative_edges": lambda **kw: linkpred.negative_edges(pos, 6, 1, 0, **kw)}
    for name, fn in fns.items():
        with pytest.raises(TypeError, match="known must be an int64 edge index"):
            fn(known=torch.tensor(POS, dtype=torch.int32))
        with pytest.raises(TypeError, match="known must be an int64 edge index"):
            fn(known=torch.tensor(POS, dtype=torch.float32))
        with pytest.raises(TypeError, match="known must be an int64 edge index"):
            fn(known=POS)
        with pytest.raises(ValueError, match=r"known must be an edge index \[2, M\]"):
            fn(known=torch.tensor(POS).t().contiguous())
        with pytest.raises(ValueError, match=r"known must be an edge index \[2, M\]"):
            fn(known=torch.tensor(POS[0]))
        with pytest.raises(RuntimeError, match="no CPU fallback"):   # well-formed, but nothing here runs on the host
            fn(known=pos)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(known=torch.zeros(2, 0, dtype=torch.long))


# ---------------------------------------------------------------------------------------------------
# the predictor: filter_negatives passes the relation's edges as known=, the default passes no known at all
# ---------------------------------------------------------------------------------------------------
class _Model:
    training = True

    def encode(self, x, e):
        return {"a": torch.zeros(4, 2), "b": torch.zeros(6, 2)}

    def eval(self):
        self.training = False

    def train(self, mode=True):
        self.training = mode


class _Graph:
    def __init__(self):
        self.edge_index = {("a", "to", "b"): torch.tensor(POS)}
        self.batch = {"a": torch.tensor([0, 1, 2, 0]), "b": torch.tensor([0, 0, 0, 1, 2, 2])}

    def x_dict(self):
        return {}

    def edge_index_dict(self):
        return {}


def test_predictor_filter_negatives_passes_known(monkeypatch):
    from hgin import linkpred
    seen = []

    def record(name, ret):
        def fake(*args, **kw):
            seen.append((name, kw))
            return ret
        return fake

    mined = torch.zeros(5, 2, dtype=torch.int32)
    monkeypatch.setattr(linkpred, "sampled_link_loss", record("loss", "loss"))
    monkeypatch.setattr(linkpred, "link_metrics", record("metrics", {}))
    monkeypatch.setattr(linkpred, "hard_negatives", record("mine", mined))
    monkeypatch.setattr(linkpred, "hard_negatives_seg",
                        lambda zs, zd, pos, m, segments, *a: (seen.append(("mine", {})), mined)[1])
    rel, g = ("a", "to", "b"), _Graph()
    own = g.edge_index[rel]
    for kw in ({}, {"hard": 2}, {"graph_local": True}, {"hard": 2, "graph_local": True, "objective": "bpr"}):
        del seen[:]
        pred = linkpred.LinkPredictor(_Model(), rel, 2, 9, filter_negatives=True, **kw)
        assert pred.filter_negatives is True
        pred.loss(g, step=1)
        pred.metrics(g)
        pred.metrics(g, neg_dst=mined)
        calls = [c for c in seen if c[0] != "mine"]
        assert [n for n, _ in calls] == ["loss", "metrics", "metrics"]
        assert all(c[1]["known"] is own for c in calls), kw
        assert all(("segments" in c[1]) == bool(kw.get("graph_local")) for c in calls)
        assert ("neg_dst" in calls[0][1]) == bool(kw.get("hard")) and "neg_dst" in calls[2][1]
        # a known of the call's own (train + valid + test edges) takes the relation's place
        more = torch.tensor([[0, 1], [1, 1]])
        del seen[:]
        pred.loss(g, step=2, known=more)
        pred.metrics(g, known=more)
        assert [c[1]["known"] is more for c in seen if c[0] != "mine"] == [True, True]
    # the default passes no known keyword at all, and a call's own known still goes through
    del seen[:]
    pred = linkpred.LinkPredictor(_Model(), rel, 2, 9, hard=2)
    assert pred.filter_negatives is False
    pred.loss(g, step=0)
    pred.metrics(g)
    pred.metrics(g, neg_dst=mined)
    assert len(seen) == 4 and all("known" not in kw for _, kw in seen)
    pred.loss(g, step=0, known=own)
    assert seen[-1][1]["known"] is own


def test_without_known_the_library_calls_are_todays(monkeypatch):
    """known=None issues exactly the entry point and argument count the call issued before A20 existed."""
    from hgin import _lib, linkpred, ops
    calls = []

    class Stop(Exception):
        pass

    def fake_call(name, *args):
        calls.append((name, len(args)))
        raise Stop

    monkeypatch.setattr(_lib, "call", fake_call)
    monkeypatch.setattr(ops, "require_device", lambda *a, **kw: None)
    monkeypatch.setattr(ops, "_stream", lambda t: None)
    pos = torch.tensor(POS)
    with pytest.raises(Stop):
        linkpred.negative_edges(pos, 6, 2, 0)
    with pytest.raises(Stop):
        linkpred.negative_edges(pos, 6, 2, 0, known=None)
    assert calls == [("hgin_neg_sample", 6), ("hgin_neg_sample", 6)]
    seg = linkpred.LinkSegments(torch.tensor([0, 1, 2, 0]), torch.tensor([0, 0, 0, 1, 2, 2]))
    del calls[:]
    with pytest.raises(Stop):
        linkpred.negative_edges(pos, 6, 2, 0, segments=seg)
    assert calls == [("hgin_neg_sample_seg", 10)]
    # with known (CPU tensors build the CSR; the launch is what is stopped): the filtered sampler, its 14 arguments
    del calls[:]
    with pytest.raises(Stop):
        linkpred.negative_edges(pos, 6, 2, 0, known=pos)
    with pytest.raises(Stop):
        linkpred.negative_edges(pos, 6, 2, 0, segments=seg, known=pos)
    assert calls == [("hgin_neg_sample_filt", 14), ("hgin_neg_sample_filt", 14)]


def test_known_csr_row_count_for_negative_edges():
    """negative_edges has no source row count: segments.n_src when given, else 1 + the largest source over the positives
    and known; cached per (known version, positives tensor)."""
    from hgin import linkpred
    pos = torch.tensor(POS)
    known = torch.tensor([[0, 6, 0], [5, 1, 2]])
    rowptr, col = linkpred._known_csr(known, None, 6, src_of=pos)
    assert rowptr.dtype == torch.int32 and rowptr.tolist() == [0, 2, 2, 2, 2, 2, 2, 3] and col.tolist() == [2, 5, 1]
    assert linkpred._known_csr(known, None, 6, src_of=pos)[0] is rowptr             # cached
    wider = linkpred._known_csr(known, None, 6, src_of=torch.tensor([[8], [0]]))      # other positives: rebuilt
    assert wider[0].numel() == 10 and wider[1].tolist() == [2, 5, 1]
    rowptr, col = linkpred._known_csr(torch.zeros(2, 0, dtype=torch.long), None, 6, src_of=pos)
    assert rowptr.tolist() == [0] * 5
    assert linkpred._known_csr(known, 9, 6)[0].numel() == 10                        # the explicit form is unchanged
    with pytest.raises(IndexError, match="dst index out of range"):
        linkpred._known_csr(torch.tensor([[0], [6]]), None, 6, src_of=pos)


# ---------------------------------------------------------------------------------------------------
# the bench tool
# ---------------------------------------------------------------------------------------------------
def test_bench_plan_is_unchanged_without_filter(capsys):
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("bench_linkpred", os.path.join(ROOT, "tools", "bench_linkpred.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    shape = tool.plan(["cfg2"], [1], 1.0)[0]
    assert sorted(shape) == ["E", "F", "config", "fwd_algorithmic_bytes", "k", "n_dst", "n_src",
                             "rank_algorithmic_bytes", "scale"]
    assert shape["fwd_algorithmic_bytes"] == tool.fwd_algorithmic_bytes(shape["E"], 1, shape["F"])
    assert "--filter" in tool.__doc__
    if not torch.cuda.is_available():
        args = ["--configs", "cfg1", "--scale", "0.1", "--k", "1"]
        rc = tool.main(args)
        plain = capsys.readouterr().err
        for extra in (["--filter"], ["--filter", "--graphs", "8"]):
            rc_f = tool.main(args + extra)
            filt = capsys.readouterr().err
            assert rc == rc_f == 2 and "no HIP device" in filt
            assert [ln for ln in filt.splitlines() if ln.startswith("plan:")] == \
                   [ln for ln in plain.splitlines() if ln.startswith("plan:")]
    with pytest.raises(SystemExit):
        tool.main(["--configs", "cfg1", "--k", "1", "--filter", "--hard", "2"])
