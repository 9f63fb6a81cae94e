"""Graph-local negatives and candidates of the link head (include/hgin.h A19), host side (no GPU): this file's numpy
references (the ones tests/test_gpu_linkseg.py checks the kernels against) agree with the C oracle's sampler at one
graph and give hand-computed cases, ``LinkSegments`` validates what it says it validates on CPU tensors, the Python
layer refuses a segmentation that does not fit before any launch, the five new entry points reject bad arguments before
touching the device, the surface and the header section exist, and the bench tools' plans are unchanged by
``--graphs``."""
import ctypes
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

from test_linkrank_host import candidate_mask

_Q = ctypes.c_void_p(16)   # a non-NULL pointer that must never be dereferenced


# ---------------------------------------------------------------------------------------------------
# references (shared with tests/test_gpu_linkseg.py)
# ---------------------------------------------------------------------------------------------------
def ref_seg_draws(seed: int, offset: int, src, k: int, src_seg, dst_ptr) -> np.ndarray:
    """int32 [E * k]: draw i belongs to positive i // k; its Philox counter c = offset + i selects block c >> 2, word
    c & 3 (key = seed), and the draw is lo + hi32(word * n) over the destinations [lo, lo + n) of the source's graph."""
    from oracle import c_oracle
    src, src_seg, dst_ptr = np.asarray(src), np.asarray(src_seg), np.asarray(dst_ptr)
    key = [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]
    out = np.zeros(len(src) * k, np.int32)
    blocks = {}
    for i in range(len(src) * k):
        c = (offset + i) & (2**64 - 1)
        b = c >> 2
        if b not in blocks:
            blocks[b] = c_oracle.philox4x32_10([b & 0xFFFFFFFF, b >> 32, 0, 0], key)
        g = int(src_seg[src[i // k]])
        lo, n = int(dst_ptr[g]), int(dst_ptr[g + 1] - dst_ptr[g])
        out[i] = lo + ((int(blocks[b][c & 3]) * n) >> 32)
    return out


def in_segment_mask(pos_src, src_seg, dst_ptr, n_dst: int) -> np.ndarray:
    """bool [Q, n_dst]: destination c lies in the graph of source pos_src[q]."""
    g = np.asarray(src_seg)[np.asarray(pos_src)]
    ptr = np.asarray(dst_ptr)
    c = np.arange(n_dst)[None, :]
    return (c >= ptr[g][:, None]) & (c < ptr[g + 1][:, None])


def ref_seg_full_ranks(zs, zd, pos, known, src_seg, dst_ptr):
    """(n_greater, n_equal, n_cand), int64 [E]: ``ref_full_ranks`` of tests/test_linkrank_host.py with its candidate
    mask ANDed with the in-segment mask."""
    zs, zd, pos = np.asarray(zs, np.float64), np.asarray(zd, np.float64), np.asarray(pos)
    score = zs[pos[0]] @ zd.T
    thr = score[np.arange(pos.shape[1]), pos[1]][:, None]
    mask = candidate_mask(pos, zs.shape[0], zd.shape[0], known) & in_segment_mask(pos[0], src_seg, dst_ptr, zd.shape[0])
    return ((score > thr) & mask).sum(1), ((score == thr) & mask).sum(1), mask.sum(1)


# ---------------------------------------------------------------------------------------------------
# the draw
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 6, 2**32 + 1])
@pytest.mark.parametrize("k", [1, 3, 5])
def test_one_graph_draws_are_the_oracle_samplers(k, offset):
    from oracle import c_oracle
    seed, E, n_dst = 0x1234ABCD5678, 23, 53
    src = np.arange(E) % 7
    got = ref_seg_draws(seed, offset, src, k, np.zeros(7, np.int32), [0, n_dst])
    assert np.array_equal(got, c_oracle.neg_sample(seed, offset, E * k, n_dst))


def test_draws_on_the_hand_computed_three_graph_case():
    """seed 0, offset 0: the four draws use Random123's known-answer block philox4x32_10(0, 0) = 6627e8d5 e169c58d
    bc57ac4c 9b00dbd8, i.e. the fractions 0.3990, 0.8805, 0.7357, 0.6055 of a segment.  Graphs own the destinations
    [0, 4), [4, 5), [5, 15); the sources 0 .. 3 lie in the graphs 2, 0, 1, 0."""
    from oracle import c_oracle
    assert [int(v) for v in c_oracle.philox4x32_10([0, 0, 0, 0], [0, 0])] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C,
                                                                             0x9B00DBD8]
    got = ref_seg_draws(0, 0, [0, 1, 2, 3], 1, [2, 0, 1, 0], [0, 4, 5, 15])
    # 5 + floor(0.3990 * 10) = 8, floor(0.8805 * 4) = 3, 4 + floor(0.7357 * 1) = 4, floor(0.6055 * 4) = 2
    assert got.tolist() == [8, 3, 4, 2]
    # k = 2 over the first two sources: draws 0, 1 belong to source 0 (graph 2), draws 2, 3 to source 1 (graph 0)
    got = ref_seg_draws(0, 0, [0, 1], 2, [2, 0, 1, 0], [0, 4, 5, 15])
    assert got.tolist() == [8, 5 + 8, 2, 2]   # 5 + floor(0.8805 * 10), floor(0.7357 * 4), floor(0.6055 * 4)


# ---------------------------------------------------------------------------------------------------
# the candidates: 4 sources, 6 destinations, F = 2; graphs own the destinations [0, 3), [3, 4), [4, 6)
#   scores   d0  d1  d2 | d3 | d4  d5      (destination rows 0 and 1 are identical)
#   s0 (g0)   2   2   0 | -1 |  3  -3
#   s1 (g1)   1   1   3 | -2 |  0   5
#   s2 (g2)  -2  -2   0 |  1 | -3   3
#   s3 (g0)   3   3   3 | -3 |  3   2
# ---------------------------------------------------------------------------------------------------
ZS = [[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [1.0, 1.0]]
ZD = [[2.0, 1.0], [2.0, 1.0], [0.0, 3.0], [-1.0, -2.0], [3.0, 0.0], [-3.0, 5.0]]
SRC_SEG = [0, 1, 2, 0]
DST_PTR = [0, 3, 4, 6]
POS = [[0, 1, 2, 3, 0], [0, 3, 5, 2, 2]]
# (0, 4) leaves graph 0; (0, 1) is listed twice; (3, 0) and (2, 4) are in-graph
KNOWN = [[0, 0, 0, 3, 2], [4, 1, 1, 0, 4]]


def test_full_rank_reference_on_the_hand_computed_case():
    gt, eq, nc = ref_seg_full_ranks(ZS, ZD, POS, None, SRC_SEG, DST_PTR)
    # (0 -> 0) thr 2: d1 ties, d2 below, d4 = 3 is another graph's; (1 -> 3): the only destination of its graph;
    # (2 -> 5) thr 3: d4 below; (3 -> 2) thr 3: d0, d1 tie; (0 -> 2) thr 0: d0, d1 above
    assert gt.tolist() == [0, 0, 0, 0, 2] and eq.tolist() == [1, 0, 0, 2, 0] and nc.tolist() == [2, 0, 1, 2, 2]
    gt, eq, nc = ref_seg_full_ranks(ZS, ZD, POS, KNOWN, SRC_SEG, DST_PTR)
    # the cross-graph (0, 4) is not subtracted: source 0 loses d1 only (once)
    assert gt.tolist() == [0, 0, 0, 0, 1] and eq.tolist() == [0, 0, 0, 1, 0] and nc.tolist() == [1, 0, 0, 1, 1]
    # one graph: the unsegmented reference
    from test_linkrank_host import ref_full_ranks
    one = ref_seg_full_ranks(ZS, ZD, POS, KNOWN, [0, 0, 0, 0], [0, 6])
    assert all(np.array_equal(a, b) for a, b in zip(one, ref_full_ranks(ZS, ZD, POS, KNOWN)))


# ---------------------------------------------------------------------------------------------------
# LinkSegments and the Python layer's checks (CPU tensors: everything here runs before a device is needed)
# ---------------------------------------------------------------------------------------------------
def test_link_segments_construction_and_validation():
    from hgin import LinkSegments
    seg = LinkSegments(torch.tensor([2, 0, 1, 0]), torch.tensor([0, 0, 0, 1, 2, 2]))
    assert seg.n_graphs == 3 and (seg.n_src, seg.n_dst) == (4, 6)
    assert seg.src_seg.dtype == torch.int32 and seg.src_seg.tolist() == [2, 0, 1, 0]
    assert seg.dst_ptr.dtype == torch.int32 and seg.dst_ptr.tolist() == [0, 3, 4, 6]
    # empty graphs on either side, int32 ids, an explicit graph count past the largest id
    seg = LinkSegments(torch.tensor([3, 3], dtype=torch.int32), torch.tensor([1, 1, 3], dtype=torch.int32), n_graphs=6)
    assert seg.n_graphs == 6 and seg.dst_ptr.tolist() == [0, 0, 2, 2, 3, 3, 3]
    seg = LinkSegments(torch.zeros(0, dtype=torch.long), torch.zeros(0, dtype=torch.long))
    assert seg.n_graphs == 1 and seg.dst_ptr.tolist() == [0, 0]
    with pytest.raises(ValueError, match="non-decreasing"):
        LinkSegments(torch.tensor([0, 1]), torch.tensor([0, 1, 0]))
    with pytest.raises(IndexError, match=r"out of range \[0, 2\)"):
        LinkSegments(torch.tensor([0, 2]), torch.tensor([0, 1]), n_graphs=2)
    with pytest.raises(IndexError, match="out of range"):
        LinkSegments(torch.tensor([0, 1]), torch.tensor([0, 3]), n_graphs=3)
    with pytest.raises(IndexError, match="out of range"):
        LinkSegments(torch.tensor([-1, 1]), torch.tensor([0, 1]))
    with pytest.raises(ValueError, match="n_graphs"):
        LinkSegments(torch.zeros(0, dtype=torch.long), torch.zeros(0, dtype=torch.long), n_graphs=0)
    with pytest.raises(TypeError, match="int32 or int64"):
        LinkSegments(torch.tensor([0.0]), torch.tensor([0]))
    with pytest.raises(TypeError, match="int32 or int64"):
        LinkSegments([0, 1], torch.tensor([0]))
    with pytest.raises(ValueError, match="one-dimensional"):
        LinkSegments(torch.zeros(2, 2, dtype=torch.long), torch.tensor([0]))


def test_link_segments_of_a_collated_graph_and_padded_batches_are_refused():
    from hgin import LinkSegments
    from hgin.data import CONFIGS, component_graph
    from hgin.store import PaddedBatch
    g = component_graph(CONFIGS["cfg1"], 4)
    seg = LinkSegments.of(g, ("path", "uses", "link"))
    assert seg.n_graphs == 4 and seg.n_src == g.num_nodes("path") and seg.n_dst == g.num_nodes("link")
    assert seg.dst_ptr.tolist() == [0, 75, 150, 225, 300]
    assert torch.equal(seg.src_seg.long(), g.batch["path"])
    # every edge of a collated relation stays inside its graph: the relation's own edges pass the positives' check
    from hgin import linkpred
    linkpred._check_segments("t", seg, seg.n_src, seg.n_dst, g.edge_index[("path", "uses", "link")])
    pb = PaddedBatch(g.x, g.edge_index, g.y, g.batch)
    with pytest.raises(ValueError, match="PaddedBatch"):
        LinkSegments.of(pb, ("path", "uses", "link"))


def test_python_errors_before_any_launch():
    from hgin import LinkSegments, linkpred
    zs, zd = torch.zeros(4, 4), torch.zeros(6, 4)
    seg = LinkSegments(torch.tensor(SRC_SEG), torch.tensor([0, 0, 0, 1, 2, 2]))
    pos = torch.tensor(POS)
    src = pos[0].contiguous()
    fns = {"sampled_link_loss": lambda zs, zd, pos, **kw: linkpred.sampled_link_loss(zs, zd, pos, 1, 0, **kw),
           "link_loss": lambda zs, zd, pos, **kw: linkpred.link_loss(zs, zd, pos, 1, 0, **kw),
           "link_ranks": lambda zs, zd, pos, **kw: linkpred.link_ranks(zs, zd, pos, 1, 0, **kw),
           "link_metrics": lambda zs, zd, pos, **kw: linkpred.link_metrics(zs, zd, pos, 1, 0, **kw),
           "link_full_ranks": lambda zs, zd, pos, **kw: linkpred.link_full_ranks(zs, zd, pos, **kw),
           "link_full_metrics": lambda zs, zd, pos, **kw: linkpred.link_full_metrics(zs, zd, pos, **kw),
           "hard_negatives_seg": lambda zs, zd, pos, segments: linkpred.hard_negatives_seg(zs, zd, pos, 2, segments)}
    leaves = torch.tensor([[0, 1], [0, 4]])      # source 1 lies in graph 1 = {d3}
    for name, fn in fns.items():
        with pytest.raises(ValueError, match="source rows"):
            fn(torch.zeros(5, 4), zd, pos, segments=seg)
        with pytest.raises(ValueError, match="destination rows"):
            fn(zs, torch.zeros(7, 4), pos, segments=seg)
        with pytest.raises(ValueError, match="outside its source's graph"):
            fn(zs, zd, leaves, segments=seg)
        with pytest.raises(TypeError, match="LinkSegments"):
            fn(zs, zd, pos, segments=(seg.src_seg, seg.dst_ptr))
        with pytest.raises(RuntimeError, match="no CPU fallback"):   # well-formed, but nothing here runs on the host
            fn(zs, zd, pos, segments=seg)
    with pytest.raises(IndexError, match="src index out of range"):
        linkpred.sampled_link_loss(zs, zd, torch.tensor([[0, 4], [0, 0]]), 1, 0, segments=seg)
    # negative_edges knows the destination count only
    with pytest.raises(ValueError, match="destination rows"):
        linkpred.negative_edges(pos, 7, 1, 0, segments=seg)
    with pytest.raises(ValueError, match="outside its source's graph"):
        linkpred.negative_edges(leaves, 6, 1, 0, segments=seg)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        linkpred.negative_edges(pos, 6, 1, 0, segments=seg)
    # link_topk has no positives: row counts only
    with pytest.raises(ValueError, match="source rows"):
        linkpred.link_topk(torch.zeros(5, 4), zd, src, 2, segments=seg)
    with pytest.raises(ValueError, match="destination rows"):
        linkpred.link_topk(zs, torch.zeros(7, 4), src, 2, segments=seg)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        linkpred.link_topk(zs, zd, src, 2, segments=seg)


def test_the_positives_check_is_cached_per_tensor_version_and_segments(monkeypatch):
    from hgin import LinkSegments, linkpred
    seg = LinkSegments(torch.tensor(SRC_SEG), torch.tensor([0, 0, 0, 1, 2, 2]))
    other = LinkSegments(torch.tensor(SRC_SEG), torch.tensor([0, 0, 0, 1, 2, 2]))
    pos = torch.tensor(POS)
    syncs = []
    real = torch.Tensor.tolist
    monkeypatch.setattr(torch.Tensor, "tolist", lambda t: (syncs.append(1), real(t))[1])
    linkpred._check_segments("t", seg, 4, 6, pos)
    linkpred._check_segments("t", seg, 4, 6, pos)
    assert len(syncs) == 1
    linkpred._check_segments("t", other, 4, 6, pos)   # another segmentation: checked again
    assert len(syncs) == 2
    pos[1, 1] = 4                                     # an in-place edit bumps the version: checked again, and fails
    with pytest.raises(ValueError, match="outside its source's graph"):
        linkpred._check_segments("t", seg, 4, 6, pos)
    assert len(syncs) == 3


# ---------------------------------------------------------------------------------------------------
# the predictor: graph_local builds one segmentation per graph object and passes it by keyword
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
        self.batch = {"a": torch.tensor(SRC_SEG), "b": torch.tensor([0, 0, 0, 1, 2, 2])}

    def x_dict(self):
        return {}

    def edge_index_dict(self):
        return {}


def test_predictor_graph_local_passes_one_cached_segmentation(monkeypatch):
    from hgin import LinkSegments, linkpred
    seen = []

    def record(name, ret):
        def fake(*args, **kw):
            seen.append((name, kw))
            return ret
        return fake

    monkeypatch.setattr(linkpred, "sampled_link_loss", record("loss", "loss"))
    def no_plain_mining(*args, **kw):
        raise AssertionError("graph_local must mine with hard_negatives_seg")

    mined = torch.zeros(5, 2, dtype=torch.int32)
    monkeypatch.setattr(linkpred, "hard_negatives", no_plain_mining)
    monkeypatch.setattr(linkpred, "hard_negatives_seg",
                        lambda zs, zd, pos, m, segments, *a: (seen.append(("mine", {"segments": segments})), mined)[1])
    monkeypatch.setattr(linkpred, "link_metrics", record("metrics", {}))
    monkeypatch.setattr(linkpred, "link_full_metrics", record("full", {}))
    monkeypatch.setattr(linkpred, "link_topk", record("topk", (None, None)))
    rel = ("a", "to", "b")
    assert inspect.signature(linkpred.LinkPredictor.__init__).parameters["graph_local"].default is False
    g = _Graph()
    pred = linkpred.LinkPredictor(_Model(), rel, 2, 9, hard=2, graph_local=True)
    pred.loss(g, step=0)
    pred.mine(g)
    pred.metrics(g)
    pred.full_metrics(g)
    pred.predict(g, k=3)
    assert [n for n, _ in seen] == ["mine", "loss", "mine", "metrics", "full", "topk"]
    segs = [kw["segments"] for _, kw in seen]
    assert isinstance(segs[0], LinkSegments) and all(s is segs[0] for s in segs)
    assert segs[0].dst_ptr.tolist() == DST_PTR and segs[0].src_seg.tolist() == SRC_SEG
    del seen[:]
    pred.loss(_Graph(), step=1)                       # another graph object: another segmentation
    assert seen[-1][1]["segments"] is not segs[0]
    # the default passes no segmentation at all
    del seen[:]
    monkeypatch.setattr(linkpred, "hard_negatives", record("mine", mined))
    pred = linkpred.LinkPredictor(_Model(), rel, 2, 9, hard=2)
    pred.loss(g, step=0)
    pred.metrics(g)
    pred.full_metrics(g)
    pred.predict(g, k=3)
    assert seen and all("segments" not in kw for _, kw in seen)


# ---------------------------------------------------------------------------------------------------
# surface, header, C argument checks
# ---------------------------------------------------------------------------------------------------
def test_public_surface():
    import hgin
    from hgin import linkpred
    assert "LinkSegments" in hgin.__all__ and hgin.LinkSegments is linkpred.LinkSegments
    assert callable(hgin.LinkSegments.of)
    for fn in (linkpred.negative_edges, linkpred.link_loss, linkpred.sampled_link_loss, linkpred.link_ranks,
               linkpred.link_metrics, linkpred.link_full_ranks, linkpred.link_full_metrics, linkpred.link_topk):
        assert inspect.signature(fn).parameters["segments"].default is None, fn.__name__
    # mining: hard_negatives keeps its pinned parameter list, the graph-local form is a function of its own
    assert "hard_negatives_seg" in hgin.__all__ and hgin.hard_negatives_seg is linkpred.hard_negatives_seg
    assert list(inspect.signature(linkpred.hard_negatives_seg).parameters) == ["z_src", "z_dst", "pos", "m", "segments",
                                                                                "known", "seed", "offset"]
    assert "segments" not in inspect.signature(linkpred.hard_negatives).parameters
    names = list(inspect.signature(linkpred.LinkSegments.__init__).parameters)
    assert names == ["self", "batch_src", "batch_dst", "n_graphs"]


NEW_SYMBOLS = ("hgin_neg_sample_seg", "hgin_link_loss_fwd_seg_f32", "hgin_link_rank_seg_f32",
               "hgin_link_full_rank_seg_f32", "hgin_link_topk_seg_f32")


def test_abi_14_and_the_header_section():
    from conftest import ROOT
    from hgin import _lib
    assert _lib.ABI_VERSION >= 14
    assert _lib.lib().hgin_abi_version() == _lib.ABI_VERSION
    text = open(os.path.join(ROOT, "include", "hgin.h")).read()
    assert int(re.search(r"#define HGIN_ABI_VERSION (\d+)", text).group(1)) >= 14
    a19 = text[text.index("---- A19"):]
    a19 = a19[:a19.index("---- F4")]
    for name in NEW_SYMBOLS:
        assert name in _lib.exported_symbols() and re.search(r"\bint " + name + r"\(", a19), name
    for word in ("src_seg", "dst_ptr", "lo + hi32(word(c) * n)", "n_cand = n - 1 -", "fully padded row", "G = 1"):
        assert word in a19, word
    declared = set(re.findall(r"^(?:int|size_t|const char\*) (hgin_\w+)\(", text, re.M))
    assert declared == set(_lib.exported_symbols())


def _sample(lib, seed=1, offset=0, src=_Q, E=4, k=2, seg=_Q, ptr=_Q, G=3, out=_Q):
    return lib.hgin_neg_sample_seg(seed, offset, src, E, k, seg, ptr, G, out, None)


def _fwd(lib, pos=_Q, E=4, k=2, n_dst=3, neg_dst=None, m=0, zs=_Q, zd=_Q, F=8, coef=_Q, neg=_Q, loss=_Q, ws=_Q,
         ws_bytes=1 << 20, objective=0, param=1.0, seg=_Q, ptr=_Q, G=3):
    return lib.hgin_link_loss_fwd_seg_f32(pos, E, k, 1, 0, n_dst, neg_dst, m, zs, F, zd, F, F, coef, neg, loss, ws,
                                          ws_bytes, objective, param, seg, ptr, G, None)


def _rank(lib, pos=_Q, E=4, k=2, n_dst=3, neg_dst=None, m=0, zs=_Q, zd=_Q, F=8, gt=_Q, eq=_Q, seg=_Q, ptr=_Q, G=3):
    return lib.hgin_link_rank_seg_f32(pos, E, k, 1, 0, n_dst, neg_dst, m, zs, F, zd, F, F, gt, eq, seg, ptr, G, None)


def _full(lib, pos=_Q, E=4, n_src=5, n_dst=3, zs=_Q, lds=8, zd=_Q, ldd=8, F=8, rowptr=None, col=None, gt=_Q, eq=_Q,
          nc=_Q, ws=_Q, ws_bytes=1 << 20, seg=_Q, ptr=_Q, G=3):
    return lib.hgin_link_full_rank_seg_f32(pos, E, n_src, n_dst, zs, lds, zd, ldd, F, rowptr, col, gt, eq, nc, ws,
                                           ws_bytes, seg, ptr, G, None)


def _topk(lib, src=_Q, Q=4, n_src=5, n_dst=3, zs=_Q, lds=8, zd=_Q, ldd=8, F=8, rowptr=None, col=None, k=2, idx=_Q,
          score=_Q, ws=_Q, ws_bytes=1 << 20, seg=_Q, ptr=_Q, G=3):
    return lib.hgin_link_topk_seg_f32(src, Q, n_src, n_dst, zs, lds, zd, ldd, F, rowptr, col, k, idx, score, ws,
                                      ws_bytes, seg, ptr, G, None)


def test_argument_errors_do_not_touch_the_device():
    from hgin import _lib
    lib = _lib.lib()
    err = lib.hgin_last_error
    for call in (_sample, _fwd, _rank, _full, _topk):
        assert call(lib, seg=None) == -1 and b"src_seg NULL" in err(), call.__name__
        assert call(lib, ptr=None) == -1 and b"dst_ptr NULL" in err(), call.__name__
        assert call(lib, G=0) == -1 and b"n_graphs = 0" in err(), call.__name__
        assert call(lib, G=1 << 31) == -1 and b"n_graphs" in err(), call.__name__
    # the sampler
    assert _sample(lib, E=-1) == -1 and b"E = -1" in err()
    assert _sample(lib, k=-1) == -1 and b"k = -1" in err()
    assert _sample(lib, E=1 << 20, k=1 << 11) == -1 and b"E * k" in err()
    assert _sample(lib, src=None) == -1 and b"src NULL" in err()
    assert _sample(lib, out=None) == -1 and b"out NULL" in err()
    assert _sample(lib, E=0, src=None, out=None) == 0 and _sample(lib, k=0, src=None, out=None) == 0   # nothing to draw
    # loss and ranks: the A13 ranges without a set, the A18 ranges with one
    for call in (_fwd, _rank):
        assert call(lib, E=0) == -1 and b"E = 0" in err()
        assert call(lib, k=0) == -1 and b"k = 0 must be >= 1" in err()
        assert call(lib, m=-1) == -1 and b"m = -1 must be >= 0" in err()
        assert call(lib, m=2, neg_dst=None) == -1 and b"neg_dst NULL" in err()
        assert call(lib, k=-1, m=2, neg_dst=_Q) == -1 and b"k = -1 must be >= 0" in err()
        assert call(lib, E=1 << 20, k=1 << 10, m=1 << 10, neg_dst=_Q) == -1 and b"E * (k + m)" in err()
        assert call(lib, n_dst=0) == -1 and b"n_dst" in err()
        assert call(lib, F=1 << 24) == -1 and b"F " in err()
        assert call(lib, pos=None) == -1 and b"pos NULL" in err()
        assert call(lib, zs=None) == -1 and b"z_src NULL" in err()
        assert call(lib, zd=None) == -1 and b"z_dst NULL" in err()
        # k = 0 with a set is a legal shape: the error that comes back is the later one
        assert call(lib, k=0, m=2, neg_dst=_Q, seg=None) == -1 and b"src_seg NULL" in err()
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
    # full ranks and top-K: their unsegmented checks
    for call in (_full, _topk):
        assert call(lib, n_src=0) == -1 and b"n_src" in err()
        assert call(lib, n_dst=1 << 31) == -1 and b"n_dst" in err()
        assert call(lib, F=0) == -1 and b"F " in err()
        assert call(lib, zs=None) == -1 and b"z_src NULL" in err()
        assert call(lib, ldd=7) == -1 and b"leading dimension" in err()
        assert call(lib, rowptr=_Q, col=None) == -1 and b"known_rowptr without known_col" in err()
        assert call(lib, ws_bytes=8) == -3 and b"workspace" in err()
        assert call(lib, ws=None) == -3 and b"workspace" in err()
    assert _full(lib, E=0) == -1 and b"E = 0" in err()
    assert _full(lib, pos=None) == -1 and b"pos NULL" in err()
    assert _full(lib, nc=None) == -1 and b"n_cand NULL" in err()
    assert _topk(lib, Q=0) == -1 and b"n_query = 0" in err()
    assert _topk(lib, k=129) == -1 and b"k = 129" in err()
    assert _topk(lib, src=None) == -1 and b"src NULL" in err()
    assert _topk(lib, idx=None) == -1 and b"top_idx NULL" in err()


# ---------------------------------------------------------------------------------------------------
# the bench tools
# ---------------------------------------------------------------------------------------------------
def _tool(name):
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_bench_tools_graphs_option_leaves_the_plans_alone(capsys):
    pred, rank = _tool("bench_linkpred"), _tool("bench_linkrank")
    # --graphs splits the planned shapes at run time: plan() itself is what it was
    assert sorted(pred.plan(["cfg2"], [1], 1.0)[0]) == ["E", "F", "config", "fwd_algorithmic_bytes", "k", "n_dst",
                                                        "n_src", "rank_algorithmic_bytes", "scale"]
    assert rank.plan(["cfg2"], 65536, 1.0)[0]["n_dst"] == 300_000
    # the split itself: equal graphs, positives sorted by graph, every positive inside its graph
    for tool in (pred, rank):
        pos, batch_src, batch_dst = tool.split_graphs(n_src=50, n_dst=21, E=200, graphs=4, seed=3)
        assert batch_dst.tolist() == sorted(batch_dst.tolist()) and int(batch_dst.max()) == 3
        assert torch.bincount(batch_dst).tolist() == [6, 5, 5, 5] and torch.bincount(batch_src).tolist() == [13, 13, 12, 12]
        g = batch_src[pos[0]]
        assert g.tolist() == sorted(g.tolist()) and torch.equal(g, batch_dst[pos[1]])
    if not torch.cuda.is_available():
        for tool, args in ((pred, ["--configs", "cfg1", "--scale", "0.1", "--k", "1"]),
                           (rank, ["--configs", "cfg1", "--scale", "0.1", "--queries", "64"])):
            rc = tool.main(args)
            plain = capsys.readouterr().err
            rc_g = tool.main(args + ["--graphs", "8"])
            split = capsys.readouterr().err
            assert rc == rc_g == 2 and "no HIP device" in split
            assert [ln for ln in split.splitlines() if ln.startswith("plan:")] == \
                   [ln for ln in plain.splitlines() if ln.startswith("plan:")]
    for tool, args in ((pred, ["--configs", "cfg1", "--k", "1"]), (rank, ["--configs", "cfg1"])):
        with pytest.raises(SystemExit):
            tool.main(args + ["--graphs", "0"])
