"""Link-prediction head: Philox negative sampler (A10) + dot-product decoder (A11) on libhgin.so.

NOT IN REFERENCE: the reference trains a path-delay regressor; BASELINE.json's north
star asks for a negative-edge sampler and a dot-product link decoder as HIP kernels.  This module is an
*additional* head over HetroGIN's node embeddings; it does not replace the readout train.py calls.

Specs (include/hgin.h): sampler out[i] = hi32(philox4x32_10(block (offset+i)>>2)[(offset+i)&3] * n_dst);
decoder score[e] = <z_src[src[e]], z_dst[dst[e]]>, backward = weighted segmented sums over the pairs'
CSR / CSC (bit-exact against oracle/hgin_oracle.c).

Training path (A13 / A14, also not in the reference): ``sampled_link_loss`` is ``link_loss`` as one fused forward
(negatives regenerated in the kernel, source row read once, loss and coefficients in the same pass) with a
deterministic store-and-sum backward; ``link_ranks`` / ``link_metrics`` evaluate with the same kernel and another
epilogue; ``LinkPredictor`` puts them behind ``model.encode`` (hgin/train.py::link_train_step).  ``link_loss`` and
the unfused pieces stay as the baseline the fused path is checked and timed against (tools/bench_linkpred.py).

Objectives (A17, not in the reference): ``sampled_link_loss`` / ``link_loss`` / ``LinkPredictor`` take ``objective`` =
"bce" (default), "softmax", "bpr" or "selfadv"; in the fused path each is another forward epilogue that writes the same
coefficient array, so the backward is shared.

Full evaluation (A15, not in the reference either): ``link_full_ranks`` / ``link_full_metrics`` /
``LinkPredictor.full_metrics`` rank every positive against *every* destination, optionally filtered by a set of known
edges, on the fp32 matrix cores without materialising a score (csrc/hgin_linkrank.hip).

Prediction (A16, not in the reference): ``link_topk`` / ``LinkPredictor.predict`` return the k best destinations of
every query source, known edges left out, from the same sweep with a selecting epilogue (csrc/hgin_linktopk.hip).

Given negatives (A18, not in the reference): ``negative_edges`` / ``link_loss`` / ``sampled_link_loss`` / ``link_ranks``
/ ``link_metrics`` take ``neg_dst`` = an integer [E, m] tensor of destinations that join each positive's k uniform draws
(k may then be 0); ``hard_negatives`` mines such a set with ``link_topk``, ``LinkPredictor(hard=m)`` trains on it.

Batches of graphs (A19, not in the reference): ``LinkSegments`` records which graph of a collated batch every source /
destination row belongs to; the functions above take it as ``segments=`` (mining: ``hard_negatives_seg``) and then draw
a negative from the positive's own graph and rank / retrieve among that graph's destinations only;
``LinkPredictor(graph_local=True)`` builds it from ``graph.batch``.  Without it nothing changes.

Filtered draws (A20, not in the reference): ``negative_edges`` / ``link_loss`` / ``sampled_link_loss`` / ``link_ranks`` /
``link_metrics`` take ``known=`` (an edge index [2, M], as ``link_full_ranks`` takes it) and then draw every negative
uniformly from the destinations of its window (all of them, or with ``segments=`` its graph's) that are *not* known
neighbours of its source: one Philox word mapped onto the r-th non-neighbour, same counters, no rejection loop.  A
source whose window is all neighbours keeps the unfiltered draw; given negatives (``neg_dst``) are never filtered.
``LinkPredictor(filter_negatives=True)`` passes the relation's own edges.  Without ``known`` nothing changes.

Mini-batches (A22, not in the reference): ``link_neighbor_batch`` seeds a ``hgin.neighbor.NeighborSampler`` with a batch's
positives (and given negatives) and returns them as local rows of the sampled subgraph; ``LinkPredictor.batch_loss``
draws the negatives ``loss`` would draw, encodes that subgraph only and scores on the fused loss
(hgin/train.py::link_minibatch_step).  ``link_neighbor_batch_excl`` / ``LinkPredictor(exclude_targets=True)`` (A25) keep
the batch's own positives, and their flips in the reverse relation, out of the neighbourhood that batch is encoded on.

Full softmax (A23, not in the reference): ``link_lse`` is the log-sum-exp of a source's scores over *every* destination
(known edges masked), forward and backward on the matrix cores without a score matrix (csrc/hgin_linklse.hip);
``full_softmax_link_loss`` is the per-positive cross-entropy over it, ``LinkPredictor.full_loss`` /
``batch_full_loss`` train on it (the latter with a mini-batch's destination seeds as in-batch negatives);
``link_lse_unfused`` is the kept torch baseline.  With ``segments=`` (A24) all of them sum over the destinations of
the source's own graph only, and sweep only the tiles those graphs cover.
"""
from __future__ import annotations

import ctypes
import math
import weakref
from typing import NamedTuple, Optional

import torch
from torch import Tensor

from . import _lib, ops


def sample_negative_dst(n: int, n_dst: int, seed: int, offset: int = 0, device="cuda") -> Tensor:
    out = torch.empty(n, dtype=torch.int32, device=device)
    if n:
        _lib.call("hgin_neg_sample", int(seed) & (2**64 - 1), int(offset), n, int(n_dst), ops._p(out),
                  ops._stream(out))
    return out


def _given_shape(what: str, neg_dst, pos: Tensor) -> int:
    """m of a caller-supplied negative set ``neg_dst`` (integer [E, m], m >= 1), 0 for None; TypeError / ValueError
    for anything else.  Looks at shapes and dtypes only, so it runs before any device is needed."""
    if neg_dst is None:
        return 0
    if not isinstance(neg_dst, Tensor) or neg_dst.dtype not in (torch.int32, torch.int64):
        got = neg_dst.dtype if isinstance(neg_dst, Tensor) else type(neg_dst).__name__
        raise TypeError(f"{what}: neg_dst must be an int32 or int64 tensor, got {got}")
    E = int(pos.size(1)) if pos.dim() == 2 else -1
    if neg_dst.dim() != 2 or int(neg_dst.size(0)) != E or int(neg_dst.size(1)) < 1:
        raise ValueError(f"{what}: neg_dst must be [E, m] with E = {E} and m >= 1, got {tuple(neg_dst.shape)}")
    return int(neg_dst.size(1))


def _mark_checked(neg32: Tensor, n_dst: int) -> None:
    """Record on an int32 contiguous set that its values are known to lie in [0, n_dst)."""
    try:
        neg32._hgin_neg_dst = (neg32._version, {int(n_dst): neg32})
    except (AttributeError, RuntimeError):
        pass


def _given_negatives(what: str, neg_dst: Tensor, n_dst: int) -> Tensor:
    """``neg_dst`` as the kernels read it: int32, contiguous (an int32 contiguous tensor is passed as it is), values
    range-checked against [0, n_dst) (one host sync; IndexError) once per tensor version and cached on the tensor,
    the way ``_known_csr`` does it."""
    ops.require_device(neg_dst, what=what)
    key = int(n_dst)
    cache = getattr(neg_dst, "_hgin_neg_dst", None)
    ver = neg_dst._version
    if cache is not None and cache[0] == ver and key in cache[1]:
        return cache[1][key]
    lo, hi = torch.stack([neg_dst.amin(), neg_dst.amax()]).tolist()
    if lo < 0 or hi >= n_dst:
        raise IndexError(f"{what}: neg_dst index out of range [0, {n_dst})")
    out = neg_dst if neg_dst.dtype == torch.int32 and neg_dst.is_contiguous() else neg_dst.to(torch.int32).contiguous()
    if cache is None or cache[0] != ver:
        cache = (ver, {})
    cache[1][key] = out
    try:
        neg_dst._hgin_neg_dst = cache
    except (AttributeError, RuntimeError):
        pass
    return out


# ---------------------------------------------------------------------------------------------------
# A19: graph-local negatives and candidates (NOT IN REFERENCE)
# ---------------------------------------------------------------------------------------------------
class LinkSegments:
    """Which graph of a collated batch every row of a relation's two node types belongs to (include/hgin.h A19).

    ``batch_src`` integer [n_src]: the graph id of every source row, in any order; ``batch_dst`` integer [n_dst]: the
    graph id of every destination row, non-decreasing (each graph's destinations form one contiguous block, which is
    what ``hgin.data.collate`` produces).  Keeps ``src_seg`` (int32 [n_src]), ``dst_ptr`` (int32 [G + 1], dst_ptr[0]
    = 0, dst_ptr[G] = n_dst) and ``n_graphs`` = G (default: the largest id + 1).  Graphs without rows are allowed on
    either side.  Validated once, here, with one host sync: ValueError for an unsorted ``batch_dst`` or G < 1,
    IndexError for an id outside [0, G).

    Passed as ``segments=`` to the link functions, a negative is drawn from the positive's own graph and ranking /
    top-K see only that graph's destinations."""

    def __init__(self, batch_src: Tensor, batch_dst: Tensor, n_graphs: int = None):
        what = "LinkSegments"
        for name, b in (("batch_src", batch_src), ("batch_dst", batch_dst)):
            if not isinstance(b, Tensor) or b.dtype not in (torch.int32, torch.int64):
                got = b.dtype if isinstance(b, Tensor) else type(b).__name__
                raise TypeError(f"{what}: {name} must be an int32 or int64 tensor, got {got}")
            if b.dim() != 1:
                raise ValueError(f"{what}: {name} must be one-dimensional, got {tuple(b.shape)}")
        if batch_src.device != batch_dst.device:
            raise ValueError(f"{what}: batch_src is on {batch_src.device}, batch_dst on {batch_dst.device}")
        n_src, n_dst = int(batch_src.numel()), int(batch_dst.numel())
        if n_src >= 2**31 or n_dst >= 2**31:
            raise ValueError(f"{what}: more than 2^31 rows")
        dev = batch_dst.device
        both = torch.cat([batch_src.reshape(-1).long(), batch_dst.reshape(-1).long()])
        if both.numel():
            unsorted = (batch_dst[1:] < batch_dst[:-1]).any().long() if n_dst > 1 else \
                torch.zeros((), dtype=torch.long, device=dev)
            lo, hi, unsorted = torch.stack([both.amin(), both.amax(), unsorted]).tolist()   # the one host sync
        else:
            lo, hi, unsorted = 0, -1, 0
        if unsorted:
            raise ValueError(f"{what}: batch_dst must be non-decreasing (each graph's destinations one contiguous block)")
        G = int(hi) + 1 if n_graphs is None else int(n_graphs)
        if n_graphs is None and G < 1:
            G = 1
        if G < 1 or G >= 2**31:
            raise ValueError(f"{what}: n_graphs = {G} must be in [1, 2^31)")
        if lo < 0 or hi >= G:
            raise IndexError(f"{what}: graph id out of range [0, {G})")
        self.n_graphs, self.n_src, self.n_dst = G, n_src, n_dst
        self.src_seg = batch_src.to(torch.int32).contiguous()
        ptr = torch.zeros(G + 1, dtype=torch.int64, device=dev)
        ptr[1:] = torch.cumsum(torch.bincount(batch_dst.long(), minlength=G), 0)
        self.dst_ptr = ptr.to(torch.int32)

    @classmethod
    def of(cls, graph, relation) -> "LinkSegments":
        """The segmentation of ``relation`` = (src_type, name, dst_type) in a collated ``HeteroGraph``, from
        ``graph.batch``.  A ``PaddedBatch`` is refused: its padding rows carry the id ``cap_graphs``."""
        from .store import PaddedBatch
        if isinstance(graph, PaddedBatch):
            raise ValueError("LinkSegments.of: a PaddedBatch is not supported (its padding rows carry the graph id "
                             "cap_graphs, past every real graph); collate the graphs with hgin.data.collate instead")
        relation = tuple(relation)
        return cls(graph.batch[relation[0]], graph.batch[relation[2]])

    @property
    def device(self):
        return self.src_seg.device


def _check_segments(what: str, segments, n_src: int, n_dst: int, pos: Tensor = None) -> None:
    """``segments`` fits the embeddings' row counts, and (with ``pos``) every positive's source is a row of the
    segmentation and its destination lies in its source's graph: ValueError (IndexError for a source out of range).
    The positives' check costs one host sync, cached per (pos tensor version, segments) the way ``_known_csr`` caches.
    Runs on whatever device the tensors live on, so it is reached before a device is needed."""
    if not isinstance(segments, LinkSegments):
        raise TypeError(f"{what}: segments must be a LinkSegments, got {type(segments).__name__}")
    if n_src is not None and int(n_src) != segments.n_src:
        raise ValueError(f"{what}: segments cover {segments.n_src} source rows, z_src has {int(n_src)}")
    if int(n_dst) != segments.n_dst:
        raise ValueError(f"{what}: segments cover {segments.n_dst} destination rows, expected {int(n_dst)}")
    if pos is None:
        return
    ops.check_edge_index(pos)
    if pos.device != segments.device:
        raise ValueError(f"{what}: pos is on {pos.device}, segments on {segments.device}")
    cache = getattr(pos, "_hgin_seg_ok", None)
    ver = pos._version
    if cache is not None and cache[0] == ver and segments in cache[1]:
        return
    if pos.size(1):
        if segments.n_src == 0:
            raise IndexError(f"{what}: pos src index out of range [0, 0)")
        s, d = pos[0], pos[1]
        oob = (s < 0) | (s >= segments.n_src)
        g = segments.src_seg[s.clamp(0, segments.n_src - 1)].long()
        ptr = segments.dst_ptr.long()
        leaves = (d < ptr[g]) | (d >= ptr[g + 1])
        oob, leaves = torch.stack([oob.any(), leaves.any()]).tolist()   # the one host sync
        if oob:
            raise IndexError(f"{what}: pos src index out of range [0, {segments.n_src})")
        if leaves:
            raise ValueError(f"{what}: a positive's destination lies outside its source's graph")
    if cache is None or cache[0] != ver:
        cache = (ver, weakref.WeakSet())
    cache[1].add(segments)
    try:
        pos._hgin_seg_ok = cache
    except (AttributeError, RuntimeError):
        pass


def _known_shape(what: str, known) -> None:
    """``known`` is an int64 [2, M] edge index: TypeError / ValueError otherwise.  Looks at the dtype and the shape only,
    so it runs before any device is needed."""
    if not isinstance(known, Tensor) or known.dtype != torch.long:
        got = known.dtype if isinstance(known, Tensor) else type(known).__name__
        raise TypeError(f"{what}: known must be an int64 edge index [2, M], got {got}")
    if known.dim() != 2 or int(known.size(0)) != 2:
        raise ValueError(f"{what}: known must be an edge index [2, M], got {tuple(known.shape)}")


def _sample_filt(src: Tensor, k: int, seed: int, offset: int, n_dst: int, segments, csr) -> Tensor:
    """int32 [E * k]: ``_sample_seg``'s draws (``segments`` None: ``sample_negative_dst``'s) taken from the
    non-neighbours of each draw's source in ``csr`` = (rowptr, col) by source (include/hgin.h A20)."""
    E, k = int(src.numel()), int(k)
    out = torch.empty(E * k, dtype=torch.int32, device=src.device)
    if E * k:
        seg = (None, None, 0) if segments is None else (segments.src_seg, segments.dst_ptr, segments.n_graphs)
        _lib.call("hgin_neg_sample_filt", int(seed) & (2**64 - 1), int(offset) & (2**64 - 1), ops._p(src.contiguous()),
                  E, k, int(n_dst), ops._p(seg[0]), ops._p(seg[1]), seg[2], int(csr[0].numel()) - 1, ops._p(csr[0]),
                  ops._p(csr[1]), ops._p(out), ops._stream(out))
    return out


def _sample_seg(src: Tensor, k: int, seed: int, offset: int, segments: LinkSegments) -> Tensor:
    """int32 [E * k]: draw i belongs to positive i // k (source ``src[i // k]``) and has Philox counter offset + i,
    drawn from that source's graph (include/hgin.h A19)."""
    E, k = int(src.numel()), int(k)
    out = torch.empty(E * k, dtype=torch.int32, device=src.device)
    if E * k:
        _lib.call("hgin_neg_sample_seg", int(seed) & (2**64 - 1), int(offset) & (2**64 - 1), ops._p(src.contiguous()),
                  E, k, ops._p(segments.src_seg), ops._p(segments.dst_ptr), segments.n_graphs, ops._p(out),
                  ops._stream(out))
    return out


def negative_edges(edge_index: Tensor, n_dst: int, k: int, seed: int, offset: int = 0,
                   neg_dst: Tensor = None, segments: LinkSegments = None, known: Tensor = None) -> Tensor:
    """k corrupted copies of every positive edge: src kept, dst drawn uniformly.  With ``neg_dst``
    (integer [E, m]; include/hgin.h A18) every positive gets k + m copies, destinations [k drawn | m given]; k may be
    0.  With ``segments`` (a ``LinkSegments``; A19) every draw comes from its positive's own graph.  With ``known``
    (an edge index [2, M]; A20) a draw is uniform over the destinations that are not known neighbours of its source
    (given ones are not filtered); the source row count is ``segments.n_src``, else 1 + the largest source of
    ``edge_index`` and ``known``."""
    m = _given_shape("negative_edges", neg_dst, edge_index)
    if known is not None:
        _known_shape("negative_edges", known)
    if segments is not None:
        _check_segments("negative_edges", segments, None, n_dst, edge_index)
    ops.require_device(edge_index, known, what="negative_edges")
    E = int(edge_index.size(1))
    csr = None
    if known is not None:
        ops.check_edge_index(edge_index)
        csr = _known_csr(known, None if segments is None else segments.n_src, n_dst, src_of=edge_index)

    def draw(n_per):
        if csr is not None:
            if n_per < 0 or E * n_per >= 2**31:
                raise ValueError(f"negative_edges: need k >= 0 and E * k < 2^31 (E = {E}, k = {n_per})")
            return _sample_filt(edge_index[0], n_per, seed, offset, n_dst, segments, csr)
        if segments is None:
            return sample_negative_dst(E * n_per, n_dst, seed, offset, edge_index.device)
        if n_per < 0 or E * n_per >= 2**31:
            raise ValueError(f"negative_edges: need k >= 0 and E * k < 2^31 (E = {E}, k = {n_per})")
        return _sample_seg(edge_index[0], n_per, seed, offset, segments)

    if m == 0:
        dst = draw(int(k)).long()
        src = edge_index[0].repeat_interleave(k)
        return torch.stack([src, dst])
    k = int(k)
    if k < 0 or E * (k + m) >= 2**31:
        raise ValueError(f"negative_edges: need k >= 0 and E * (k + m) < 2^31 (E = {E}, k = {k}, m = {m})")
    given = _given_negatives("negative_edges", neg_dst, n_dst)
    drawn = draw(k).view(E, k)
    dst = torch.cat([drawn, given], 1).reshape(-1).long()
    return torch.stack([edge_index[0].repeat_interleave(k + m), dst])


class _DotDecodeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z_src, z_dst, pairs: Tensor, graph: ops.RelationGraph):
        n = int(pairs.size(1))
        F = int(z_src.size(1))
        src32 = pairs[0].to(torch.int32).contiguous()
        dst32 = pairs[1].to(torch.int32).contiguous()
        score = torch.empty(n, dtype=torch.float32, device=z_src.device)
        _lib.call("hgin_dot_decode_fwd_f32", ops._p(src32), ops._p(dst32), n, ops._p(z_src), z_src.stride(0),
                  ops._p(z_dst), z_dst.stride(0), F, ops._p(score), ops._stream(score))
        ctx.graph = graph
        ctx.save_for_backward(z_src, z_dst)
        return score

    @staticmethod
    def backward(ctx, g):
        z_src, z_dst = ctx.saved_tensors
        g = g.contiguous()
        graph = ctx.graph
        F = int(z_src.size(1))
        g_src = g_dst = None
        if ctx.needs_input_grad[0]:
            csc = graph.csc           # rows = src, col = dst
            g_src = torch.empty_like(z_src)
            _lib.call("hgin_dot_decode_bwd_f32", ops._p(csc.rowptr), ops._p(csc.col), ops._p(csc.perm), csc.n_rows,
                      ops._p(g), ops._p(z_dst), z_dst.stride(0), F, ops._p(g_src), g_src.stride(0),
                      ops._stream(g))
        if ctx.needs_input_grad[1]:
            csr = graph.csr           # rows = dst, col = src
            g_dst = torch.empty_like(z_dst)
            _lib.call("hgin_dot_decode_bwd_f32", ops._p(csr.rowptr), ops._p(csr.col), ops._p(csr.perm), csr.n_rows,
                      ops._p(g), ops._p(z_src), z_src.stride(0), F, ops._p(g_dst), g_dst.stride(0),
                      ops._stream(g))
        return g_src, g_dst, None, None


def dot_decode(z_src: Tensor, z_dst: Tensor, pairs: Tensor) -> Tensor:
    """score[e] = <z_src[pairs[0, e]], z_dst[pairs[1, e]]> with a HIP backward."""
    ops.require_device(z_src, z_dst, pairs, what="dot_decode")
    z_src = ops._rowmajor(ops._f32(z_src, "z_src"))
    z_dst = ops._rowmajor(ops._f32(z_dst, "z_dst"))
    if z_src.size(1) != z_dst.size(1):
        raise RuntimeError("dot_decode: embedding widths differ")
    graph = ops.relation_graph(pairs, z_src.size(0), z_dst.size(0))
    return _DotDecodeFn.apply(z_src, z_dst, pairs, graph)


# the objectives of the sampled link loss (include/hgin.h A17), in the order of the C ABI's codes
LINK_OBJECTIVES = ("bce", "softmax", "bpr", "selfadv")


def _objective(what: str, objective, temperature, alpha):
    """(code, param) of the C ABI for a checked objective; ValueError for anything else, before any launch."""
    if objective not in LINK_OBJECTIVES:
        raise ValueError(f"{what}: unknown objective {objective!r} (one of {', '.join(LINK_OBJECTIVES)})")
    temperature, alpha = float(temperature), float(alpha)
    if not (math.isfinite(temperature) and temperature > 0.0):
        raise ValueError(f"{what}: temperature must be finite and > 0, got {temperature}")
    if not (math.isfinite(alpha) and alpha >= 0.0):
        raise ValueError(f"{what}: alpha must be finite and >= 0, got {alpha}")
    code = LINK_OBJECTIVES.index(objective)
    return code, {1: temperature, 3: alpha}.get(code, 0.0)


def link_loss(z_src: Tensor, z_dst: Tensor, pos: Tensor, k: int, seed: int, offset: int = 0, objective: str = "bce",
              temperature: float = 1.0, alpha: float = 1.0, neg_dst: Tensor = None,
              segments: LinkSegments = None, known: Tensor = None) -> Tensor:
    """The unfused sampled link loss over positives and k uniform negatives per positive: ``objective`` "bce"
    (BCE-with-logits, the default), "softmax", "bpr" or "selfadv" (include/hgin.h A17), as torch ops on the two
    ``dot_decode`` score vectors.  ``neg_dst`` (integer [E, m]) adds m given negatives per positive (A18);
    ``segments`` (a ``LinkSegments``) draws every negative from its positive's own graph (A19); ``known`` (an edge
    index [2, M]) draws it from the destinations that are not known neighbours of its source (A20), through
    ``negative_edges(known=)``."""
    code, param = _objective("link_loss", objective, temperature, alpha)
    m = _given_shape("link_loss", neg_dst, pos)
    if known is not None:
        _known_shape("link_loss", known)
        if segments is not None:
            _check_segments("link_loss", segments, z_src.size(0), z_dst.size(0), pos)
        neg = negative_edges(pos, z_dst.size(0), k, seed, offset, neg_dst, segments=segments, known=known)
    elif segments is not None:
        _check_segments("link_loss", segments, z_src.size(0), z_dst.size(0), pos)
        neg = negative_edges(pos, z_dst.size(0), k, seed, offset, neg_dst, segments=segments)
    else:
        neg = negative_edges(pos, z_dst.size(0), k, seed, offset) if m == 0 else \
            negative_edges(pos, z_dst.size(0), k, seed, offset, neg_dst)
    k = int(k) + m
    s_pos = dot_decode(z_src, z_dst, pos)
    s_neg = dot_decode(z_src, z_dst, neg)
    fn = torch.nn.functional
    if code == 0:
        bce = fn.binary_cross_entropy_with_logits
        return bce(s_pos, torch.ones_like(s_pos)) * 0.5 + bce(s_neg, torch.zeros_like(s_neg)) * 0.5
    s_neg = s_neg.reshape(-1, int(k))
    if code == 1:
        x = torch.cat([s_pos.unsqueeze(1), s_neg], 1) / param
        return (torch.logsumexp(x, 1) - x[:, 0]).mean()
    if code == 2:
        return fn.softplus(s_neg - s_pos.unsqueeze(1)).mean()
    p = torch.softmax(param * s_neg, 1).detach()
    return 0.5 * (fn.softplus(-s_pos) + (p * fn.softplus(s_neg)).sum(1)).mean()


# ---------------------------------------------------------------------------------------------------
# A13 / A14: the fused sampled link loss, sampled ranks and the training head (NOT IN REFERENCE)
# ---------------------------------------------------------------------------------------------------
def _link_operands(what: str, z_src: Tensor, z_dst: Tensor, pos: Tensor, k: int, neg_dst: Tensor = None,
                   segments: LinkSegments = None):
    """Checked operands of the fused kernels: fp32 row-major embeddings of one width, validated positives; with
    ``neg_dst`` the checked int32 [E, m] set comes back as a seventh item (and k may be 0).  ``segments`` is checked
    against the row counts and the positives (``_check_segments``)."""
    m = _given_shape(what, neg_dst, pos)
    if int(k) < (0 if m else 1):
        raise ValueError(f"{what}: need E >= 1, k >= {0 if m else 1} and E * k < 2^31 (k = {int(k)})")
    if segments is not None:
        _check_segments(what, segments, z_src.size(0) if z_src.dim() else -1, z_dst.size(0) if z_dst.dim() else -1, pos)
    ops.require_device(z_src, z_dst, pos, neg_dst, what=what)
    for name, z in (("z_src", z_src), ("z_dst", z_dst)):
        if z.dtype != torch.float32:
            raise TypeError(f"{what}: {name} must be float32 (the fused link kernels are fp32 only), got {z.dtype}")
        if z.dim() != 2:
            raise RuntimeError(f"{what}: {name} must be [N, F]")
    if z_src.size(1) != z_dst.size(1):
        raise RuntimeError(f"{what}: embedding widths differ")
    ops.check_edge_index(pos)
    E, k = int(pos.size(1)), int(k)
    if m:
        if E < 1 or E * (k + m) >= 2**31:
            raise ValueError(f"{what}: need E >= 1, k >= 0 and E * (k + m) < 2^31 (E = {E}, k = {k}, m = {m})")
    elif E < 1 or k < 1 or E * k >= 2**31:
        raise ValueError(f"{what}: need E >= 1, k >= 1 and E * k < 2^31 (E = {E}, k = {k})")
    # the static CSR / CSC of the positives: built (and range-checked) once per pos tensor, cached on it
    graph = ops.relation_graph(pos, z_src.size(0), z_dst.size(0))
    out = (ops._rowmajor(z_src), ops._rowmajor(z_dst), pos.contiguous(), graph, E, k)
    return out if m == 0 else out + (_given_negatives(what, neg_dst, int(z_dst.size(0))),)


_SIDE_STREAMS: dict = {}


def _side_stream(device) -> "torch.cuda.Stream":
    """One extra stream per device for the per-step sort of the negatives (see _SampledLinkLossFn.backward)."""
    key = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    s = _SIDE_STREAMS.get(key)
    if s is None:
        s = _SIDE_STREAMS[key] = torch.cuda.Stream(device=key)
    return s


class _SampledLinkLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z_src, z_dst, pos, graph: ops.RelationGraph, k: int, seed: int, offset: int, objective: int = 0,
                param: float = 0.0, neg_dst: Tensor = None, segments: LinkSegments = None, known_csr=None):
        E, F, dev = int(pos.size(1)), int(z_src.size(1)), z_src.device
        m = 0 if neg_dst is None else int(neg_dst.size(1))   # A18: k uniform + m given negatives per positive
        K = k + m
        coef = torch.empty(E * (1 + K), dtype=torch.float32, device=dev)
        neg = torch.empty((2, E * K), dtype=torch.int64, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        nbytes = ctypes.c_size_t(0)
        _lib.check(_lib.lib().hgin_link_loss_workspace_size(E, ctypes.byref(nbytes)), "hgin_link_loss_workspace_size")
        ws = ops._workspace(nbytes.value, dev)
        if known_csr is not None:   # A20: draws from the non-neighbours, segmented or not, given negatives or not
            seg = (None, None, 0) if segments is None else (segments.src_seg, segments.dst_ptr, segments.n_graphs)
            _lib.call("hgin_link_loss_fwd_filt_f32", ops._p(pos), E, k, int(seed) & (2**64 - 1),
                      int(offset) & (2**64 - 1), int(z_dst.size(0)), ops._p(neg_dst), m, ops._p(z_src), z_src.stride(0),
                      ops._p(z_dst), z_dst.stride(0), F, ops._p(coef), ops._p(neg), ops._p(loss), ops._p(ws),
                      nbytes.value, objective, param, ops._p(seg[0]), ops._p(seg[1]), seg[2], int(z_src.size(0)),
                      ops._p(known_csr[0]), ops._p(known_csr[1]), ops._stream(loss))
        elif segments is not None:   # A19: graph-local draws, given negatives or not; coef / neg as below
            _lib.call("hgin_link_loss_fwd_seg_f32", ops._p(pos), E, k, int(seed) & (2**64 - 1),
                      int(offset) & (2**64 - 1), int(z_dst.size(0)), ops._p(neg_dst), m, ops._p(z_src), z_src.stride(0),
                      ops._p(z_dst), z_dst.stride(0), F, ops._p(coef), ops._p(neg), ops._p(loss), ops._p(ws),
                      nbytes.value, objective, param, ops._p(segments.src_seg), ops._p(segments.dst_ptr),
                      segments.n_graphs, ops._stream(loss))
        elif m:   # the same coef / neg layout with K in place of k: the backward below does not know the difference
            _lib.call("hgin_link_loss_fwd_neg_f32", ops._p(pos), E, k, int(seed) & (2**64 - 1),
                      int(offset) & (2**64 - 1), int(z_dst.size(0)), ops._p(neg_dst), m, ops._p(z_src), z_src.stride(0),
                      ops._p(z_dst), z_dst.stride(0), F, ops._p(coef), ops._p(neg), ops._p(loss), ops._p(ws),
                      nbytes.value, objective, param, ops._stream(loss))
        elif objective == 0:
            _lib.call("hgin_link_loss_fwd_f32", ops._p(pos), E, k, int(seed) & (2**64 - 1), int(offset) & (2**64 - 1),
                      int(z_dst.size(0)), ops._p(z_src), z_src.stride(0), ops._p(z_dst), z_dst.stride(0), F,
                      ops._p(coef), ops._p(neg), ops._p(loss), ops._p(ws), nbytes.value, ops._stream(loss))
        else:   # another epilogue writes the same coef / neg (A17): the backward below serves every objective
            _lib.call("hgin_link_loss_fwd_obj_f32", ops._p(pos), E, k, int(seed) & (2**64 - 1),
                      int(offset) & (2**64 - 1), int(z_dst.size(0)), ops._p(z_src), z_src.stride(0), ops._p(z_dst),
                      z_dst.stride(0), F, ops._p(coef), ops._p(neg), ops._p(loss), ops._p(ws), nbytes.value,
                      objective, param, ops._stream(loss))
        ctx.graph, ctx.k = graph, K
        ctx.save_for_backward(coef, neg, z_src, z_dst)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        coef, neg, z_src, z_dst = ctx.saved_tensors
        graph, k = ctx.graph, ctx.k
        E, F, dev = graph.n_edges, int(z_src.size(1)), z_src.device
        g = g.reshape(1).to(torch.float32).contiguous()   # device scalar: no host sync
        g_src = g_dst = None
        cur = torch.cuda.current_stream(dev)
        side = None
        if ctx.needs_input_grad[1]:
            csr = graph.csr           # rows = dst, col = src (static)
            n_dst, n_neg = int(z_dst.size(0)), E * k
            # this step's negatives by destination: one stable sort, no validation sync (sources are the
            # positives', destinations are < n_dst by construction).  Its buffers are allocated on the current
            # stream; when the source side runs too, the sort (many short passes, far from the HBM rate) is issued on
            # a side stream so that it overlaps the source-side gather, and the current stream waits for it below.
            nrow = torch.empty(n_dst + 1, dtype=torch.int32, device=dev)
            ncol = torch.empty(n_neg, dtype=torch.int32, device=dev)
            nperm = torch.empty(n_neg, dtype=torch.int32, device=dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            nbytes = ctypes.c_size_t(0)
            _lib.check(_lib.lib().hgin_csr_workspace_size(n_neg, n_dst, ctypes.byref(nbytes)),
                       "hgin_csr_workspace_size")
            ws = ops._workspace(nbytes.value, dev)
            sort_stream = cur
            if ctx.needs_input_grad[0]:
                side = sort_stream = _side_stream(dev)
                side.wait_stream(cur)
            _lib.call("hgin_csr_build", ops._p(neg), n_neg, 1, n_dst, int(z_src.size(0)), ops._p(nrow), ops._p(ncol),
                      ops._p(nperm), ops._p(status), ops._p(ws), nbytes.value, ctypes.c_void_p(sort_stream.cuda_stream))
        if ctx.needs_input_grad[0]:
            csc = graph.csc           # rows = src, col = dst (static)
            g_src = torch.empty((z_src.size(0), F), dtype=torch.float32, device=dev)
            _lib.call("hgin_link_loss_bwd_src_f32", ops._p(csc.rowptr), ops._p(csc.col), ops._p(csc.perm), csc.n_rows,
                      E, k, ops._p(g), ops._p(coef), ops._p(neg), ops._p(z_dst), z_dst.stride(0), F, ops._p(g_src),
                      g_src.stride(0), ops._stream(g))
        if ctx.needs_input_grad[1]:
            if side is not None:
                cur.wait_stream(side)   # every later use (and reuse) of the sort's buffers is ordered after it
            g_dst = torch.empty((n_dst, F), dtype=torch.float32, device=dev)
            _lib.call("hgin_link_loss_bwd_dst_f32", ops._p(csr.rowptr), ops._p(csr.col), ops._p(csr.perm),
                      ops._p(nrow), ops._p(ncol), ops._p(nperm), n_dst, E, ops._p(g), ops._p(coef), ops._p(z_src),
                      z_src.stride(0), F, ops._p(g_dst), g_dst.stride(0), ops._stream(g))
        return g_src, g_dst, None, None, None, None, None, None, None, None, None, None


def sampled_link_loss(z_src: Tensor, z_dst: Tensor, pos: Tensor, k: int, seed: int, offset: int = 0,
                      objective: str = "bce", temperature: float = 1.0, alpha: float = 1.0,
                      neg_dst: Tensor = None, segments: LinkSegments = None, known: Tensor = None) -> Tensor:
    """``link_loss`` in fused form (include/hgin.h A13 / A17): the same pairs (``negative_edges(pos, n_dst, k, seed,
    offset)``) and the same loss, one forward pass that draws the negatives in the kernel and reads every source
    row once, and a deterministic store-and-sum backward (static CSC / CSR of ``pos`` + one sort of the step's
    negatives).  ``objective``: "bce" (default), "softmax" (InfoNCE over the positive and its k negatives at
    ``temperature``), "bpr" (pairwise) or "selfadv" (BCE with the negatives weighted by a detached
    softmax(``alpha`` * score)); only the forward epilogue differs.  ``neg_dst`` (int32 or int64 [E, m] on the device,
    values in [0, n_dst): checked once per tensor version, one host sync) adds m given negatives after each
    positive's k drawn ones (include/hgin.h A18): K = k + m takes k's place in every weight and normaliser, k may be
    0, and a given destination contributes exactly what the same destination would as a draw.  ``segments`` (a
    ``LinkSegments``; include/hgin.h A19) draws every negative from its positive's own graph, at the same Philox
    counters; with one graph the result is bit for bit the unsegmented one.  ``known`` (an int64 edge index [2, M] on the
    device; include/hgin.h A20; its CSR is built and range-checked once per tensor version, as ``link_full_ranks``
    builds it) draws every negative uniformly from the destinations of its window (all of them, or its graph's) that
    are not known neighbours of its source, at the same counters: a source without known edges keeps today's draw bit
    for bit, a source whose window is all neighbours keeps the unfiltered draw (it has no true negative), and
    ``neg_dst`` is never filtered.  Returns a scalar; fp32 embeddings only."""
    code, param = _objective("sampled_link_loss", objective, temperature, alpha)
    if known is not None:
        _known_shape("sampled_link_loss", known)
        ops_ = _link_operands("sampled_link_loss", z_src, z_dst, pos, k, neg_dst, segments)
        ops.require_device(known, what="sampled_link_loss")
        z_src, z_dst, pos, graph, _, k = ops_[:6]
        given = ops_[6] if len(ops_) > 6 else None
        csr = _known_csr(known, int(z_src.size(0)), int(z_dst.size(0)))
        return _SampledLinkLossFn.apply(z_src, z_dst, pos, graph, k, int(seed), int(offset), code, param, given,
                                        segments, csr)
    if segments is not None:
        ops_ = _link_operands("sampled_link_loss", z_src, z_dst, pos, k, neg_dst, segments)
        z_src, z_dst, pos, graph, _, k = ops_[:6]
        given = ops_[6] if len(ops_) > 6 else None
        return _SampledLinkLossFn.apply(z_src, z_dst, pos, graph, k, int(seed), int(offset), code, param, given,
                                        segments)
    if neg_dst is None:
        z_src, z_dst, pos, graph, _, k = _link_operands("sampled_link_loss", z_src, z_dst, pos, k)
        return _SampledLinkLossFn.apply(z_src, z_dst, pos, graph, k, int(seed), int(offset), code, param)
    z_src, z_dst, pos, graph, _, k, given = _link_operands("sampled_link_loss", z_src, z_dst, pos, k, neg_dst)
    return _SampledLinkLossFn.apply(z_src, z_dst, pos, graph, k, int(seed), int(offset), code, param, given)


def link_ranks(z_src: Tensor, z_dst: Tensor, pos: Tensor, k: int, seed: int, offset: int = 0, neg_dst: Tensor = None,
               segments: LinkSegments = None, known: Tensor = None):
    """(n_greater, n_equal), int32 [E]: how many of each positive's k sampled negatives (the draws of
    ``sampled_link_loss``) score above / exactly equal to it (include/hgin.h A14); with ``neg_dst`` (integer [E, m],
    e.g. a fixed evaluation set; A18) the counts cover the k draws and the m given negatives, and k may be 0.  With
    ``segments`` (a ``LinkSegments``; A19) the draws come from each positive's own graph.  With ``known`` (an edge
    index [2, M]; A20) the draws are ``sampled_link_loss(known=)``'s: no known neighbour of the source is counted as a
    beaten or lost candidate (unless its window holds nothing else).  No gradient."""
    given = None
    if known is not None:
        _known_shape("link_ranks", known)
    if neg_dst is None:
        z_src, z_dst, pos, _, E, k = _link_operands("link_ranks", z_src, z_dst, pos, k, None, segments)
    else:
        z_src, z_dst, pos, _, E, k, given = _link_operands("link_ranks", z_src, z_dst, pos, k, neg_dst, segments)
    z_src, z_dst = z_src.detach(), z_dst.detach()
    n_gt = torch.empty(E, dtype=torch.int32, device=z_src.device)
    n_eq = torch.empty(E, dtype=torch.int32, device=z_src.device)
    if known is not None:
        ops.require_device(known, what="link_ranks")
        csr = _known_csr(known, int(z_src.size(0)), int(z_dst.size(0)))
        seg = (None, None, 0) if segments is None else (segments.src_seg, segments.dst_ptr, segments.n_graphs)
        _lib.call("hgin_link_rank_filt_f32", ops._p(pos), E, k, int(seed) & (2**64 - 1), int(offset) & (2**64 - 1),
                  int(z_dst.size(0)), ops._p(given), 0 if given is None else int(given.size(1)), ops._p(z_src),
                  z_src.stride(0), ops._p(z_dst), z_dst.stride(0), int(z_src.size(1)), ops._p(n_gt), ops._p(n_eq),
                  ops._p(seg[0]), ops._p(seg[1]), seg[2], int(z_src.size(0)), ops._p(csr[0]), ops._p(csr[1]),
                  ops._stream(n_gt))
        return n_gt, n_eq
    if segments is not None:
        _lib.call("hgin_link_rank_seg_f32", ops._p(pos), E, k, int(seed) & (2**64 - 1), int(offset) & (2**64 - 1),
                  int(z_dst.size(0)), ops._p(given), 0 if given is None else int(given.size(1)), ops._p(z_src),
                  z_src.stride(0), ops._p(z_dst), z_dst.stride(0), int(z_src.size(1)), ops._p(n_gt), ops._p(n_eq),
                  ops._p(segments.src_seg), ops._p(segments.dst_ptr), segments.n_graphs, ops._stream(n_gt))
        return n_gt, n_eq
    if given is not None:
        _lib.call("hgin_link_rank_neg_f32", ops._p(pos), E, k, int(seed) & (2**64 - 1), int(offset) & (2**64 - 1),
                  int(z_dst.size(0)), ops._p(given), int(given.size(1)), ops._p(z_src), z_src.stride(0), ops._p(z_dst),
                  z_dst.stride(0), int(z_src.size(1)), ops._p(n_gt), ops._p(n_eq), ops._stream(n_gt))
        return n_gt, n_eq
    _lib.call("hgin_link_rank_f32", ops._p(pos), E, k, int(seed) & (2**64 - 1), int(offset) & (2**64 - 1),
              int(z_dst.size(0)), ops._p(z_src), z_src.stride(0), ops._p(z_dst), z_dst.stride(0), int(z_src.size(1)),
              ops._p(n_gt), ops._p(n_eq), ops._stream(n_gt))
    return n_gt, n_eq


def metrics_from_ranks(n_greater: Tensor, n_equal: Tensor, k: int) -> dict:
    """Sampled ranking metrics as 0-dim tensors on the ranks' device (nothing is synchronised):
    auc = 1 - (sum greater + 0.5 sum equal) / (E k); with rank = 1 + greater + equal / 2 (ties share the middle
    rank): mrr = mean 1 / rank, hits@K = mean [rank <= K]."""
    gt, eq = n_greater.to(torch.float64), n_equal.to(torch.float64)
    E = gt.numel()
    rank = 1.0 + gt + 0.5 * eq
    out = {"auc": 1.0 - (gt.sum() + 0.5 * eq.sum()) / float(E * int(k)), "mrr": (1.0 / rank).mean()}
    for K in (1, 3, 10):
        out[f"hits@{K}"] = (rank <= K).to(torch.float64).mean()
    return out


def link_metrics(z_src: Tensor, z_dst: Tensor, pos: Tensor, k: int, seed: int, offset: int = 0,
                 neg_dst: Tensor = None, segments: LinkSegments = None, known: Tensor = None) -> dict:
    """auc / mrr / hits@1 / hits@3 / hits@10 of the positives against k sampled negatives each, as device scalars
    (float64): the ranking kernel + a few reductions over [E]; no host sync before the caller reads a value.  With
    ``neg_dst`` (integer [E, m]; A18) against the k draws and the m given negatives (the set's one-off range check
    aside).  ``segments`` (a ``LinkSegments``; A19): the draws come from each positive's own graph.  ``known``
    (an edge index [2, M]; A20): the draws leave out the known neighbours of each positive's source, as the full
    metrics' ``known`` leaves them out of the candidates."""
    if known is not None:
        n_gt, n_eq = link_ranks(z_src, z_dst, pos, k, seed, offset, neg_dst, segments=segments, known=known)
        return metrics_from_ranks(n_gt, n_eq, int(k) + (0 if neg_dst is None else int(neg_dst.size(1))))
    if segments is not None:
        n_gt, n_eq = link_ranks(z_src, z_dst, pos, k, seed, offset, neg_dst, segments=segments)
        return metrics_from_ranks(n_gt, n_eq, int(k) + (0 if neg_dst is None else int(neg_dst.size(1))))
    if neg_dst is None:
        n_gt, n_eq = link_ranks(z_src, z_dst, pos, k, seed, offset)
        return metrics_from_ranks(n_gt, n_eq, k)
    n_gt, n_eq = link_ranks(z_src, z_dst, pos, k, seed, offset, neg_dst)
    return metrics_from_ranks(n_gt, n_eq, int(k) + int(neg_dst.size(1)))


# ---------------------------------------------------------------------------------------------------
# A15: full-candidate filtered ranking (NOT IN REFERENCE)
# ---------------------------------------------------------------------------------------------------
def _known_csr(known: Tensor, n_src: int, n_dst: int, src_of: Tensor = None):
    """(rowptr int32 [n_src + 1], col int32) of ``known`` by source: columns sorted within a row, duplicates removed.
    Built (and range-checked, one host sync) once per tensor version and cached on the tensor.  ``n_src`` None (a
    caller without a row count: ``negative_edges``): 1 + the largest source over ``known`` and the edge index
    ``src_of`` (one more sync inside the same cached build), cached per (``src_of`` tensor, its version)."""
    cache = getattr(known, "_hgin_known_csr", None)
    ver = known._version
    if n_src is None:
        key = ("auto", int(n_dst))
        hit = cache[1].get(key) if cache is not None and cache[0] == ver else None
        if hit is not None and hit[0]() is src_of and hit[1] == src_of._version:
            return hit[2]
    else:
        key = (int(n_src), int(n_dst))
        if cache is not None and cache[0] == ver and key in cache[1]:
            return cache[1][key]
    ops.check_edge_index(known)
    dev = known.device
    if n_src is None:
        if known.device != src_of.device:
            raise ValueError(f"known is on {known.device}, the positives on {src_of.device}")
        tops = [t[0].amax() for t in (known, src_of) if t.size(1)]
        n_src = 1 + max(int(torch.stack(tops).amax()) if tops else 0, 0)
        if n_src >= 2**31:
            raise IndexError("known: src index out of range [0, 2^31)")
        out = _known_csr(known, n_src, n_dst)
        cache = getattr(known, "_hgin_known_csr", None)
        if cache is not None and cache[0] == ver:
            cache[1][key] = (weakref.ref(src_of), src_of._version, out)
        return out
    if known.size(1):
        lo, hi = known.amin(1), known.amax(1)
        bounds = torch.stack([lo[0], hi[0], lo[1], hi[1]]).tolist()
        if bounds[0] < 0 or bounds[1] >= n_src:
            raise IndexError(f"known: src index out of range [0, {n_src})")
        if bounds[2] < 0 or bounds[3] >= n_dst:
            raise IndexError(f"known: dst index out of range [0, {n_dst})")
    pairs = torch.unique(known[0] * int(n_dst) + known[1])   # sorted: by source, then by destination
    if pairs.numel() >= 2**31:
        raise ValueError("known: more than 2^31 distinct edges")
    src = torch.div(pairs, int(n_dst), rounding_mode="floor")
    col = (pairs - src * int(n_dst)).to(torch.int32)
    rowptr = torch.zeros(n_src + 1, dtype=torch.int64, device=dev)
    rowptr[1:] = torch.cumsum(torch.bincount(src, minlength=n_src), 0)
    out = (rowptr.to(torch.int32), col if col.numel() else torch.zeros(1, dtype=torch.int32, device=dev))
    if cache is None or cache[0] != ver:
        cache = (ver, {})
    cache[1][key] = out
    try:
        known._hgin_known_csr = cache
    except (AttributeError, RuntimeError):
        pass
    return out


def link_full_ranks(z_src: Tensor, z_dst: Tensor, pos: Tensor, known: Tensor = None, segments: LinkSegments = None):
    """(n_greater, n_equal, n_cand), int32 [E] (include/hgin.h A15): every positive (s, d) of ``pos`` is ranked against
    every destination c != d, minus the c with (s, c) in ``known`` (an edge index [2, M]; None: unfiltered).
    n_greater / n_equal count the candidates scoring above / exactly equal to the positive, n_cand the candidates.
    Scores are fp32 dot products on the matrix cores and are never written.  With ``segments`` (a ``LinkSegments``;
    include/hgin.h A19) the candidates of (s, d) are only the destinations of s's own graph (known edges that leave
    the graph are never candidates and are not subtracted), and a block of 128 queries sweeps only the destination
    tiles its graphs cover: sort the positives by graph to visit n_dst / G instead of n_dst.  No gradient."""
    what = "link_full_ranks"
    if segments is not None:
        _check_segments(what, segments, z_src.size(0) if z_src.dim() else -1, z_dst.size(0) if z_dst.dim() else -1,
                        pos if isinstance(pos, Tensor) and pos.dim() == 2 and pos.dtype == torch.long else None)
    ops.require_device(known, what=what)
    z_src, z_dst, pos, _, E, _ = _link_operands(what, z_src, z_dst, pos, 1)
    z_src, z_dst = z_src.detach(), z_dst.detach()
    dev = z_src.device
    n_src, n_dst, F = int(z_src.size(0)), int(z_dst.size(0)), int(z_src.size(1))
    if F < 1:
        raise ValueError(f"{what}: embeddings need at least one feature")
    rowptr = col = None
    if known is not None:
        rowptr, col = _known_csr(known, n_src, n_dst)
    n_gt = torch.empty(E, dtype=torch.int32, device=dev)
    n_eq = torch.empty(E, dtype=torch.int32, device=dev)
    n_cand = torch.empty(E, dtype=torch.int32, device=dev)
    nbytes = ctypes.c_size_t(0)
    _lib.check(_lib.lib().hgin_link_full_rank_workspace_size(E, n_dst, F, ctypes.byref(nbytes)),
               "hgin_link_full_rank_workspace_size")
    ws = ops._workspace(nbytes.value, dev)
    if segments is not None:
        _lib.call("hgin_link_full_rank_seg_f32", ops._p(pos), E, n_src, n_dst, ops._p(z_src), z_src.stride(0),
                  ops._p(z_dst), z_dst.stride(0), F, ops._p(rowptr), ops._p(col), ops._p(n_gt), ops._p(n_eq),
                  ops._p(n_cand), ops._p(ws), nbytes.value, ops._p(segments.src_seg), ops._p(segments.dst_ptr),
                  segments.n_graphs, ops._stream(n_gt))
        return n_gt, n_eq, n_cand
    _lib.call("hgin_link_full_rank_f32", ops._p(pos), E, n_src, n_dst, ops._p(z_src), z_src.stride(0), ops._p(z_dst),
              z_dst.stride(0), F, ops._p(rowptr), ops._p(col), ops._p(n_gt), ops._p(n_eq), ops._p(n_cand), ops._p(ws),
              nbytes.value, ops._stream(n_gt))
    return n_gt, n_eq, n_cand


def full_metrics_from_ranks(n_greater: Tensor, n_equal: Tensor, n_cand: Tensor) -> dict:
    """Full ranking metrics as 0-dim float64 tensors on the counts' device (nothing is synchronised), keys as
    ``metrics_from_ranks``: rank = 1 + greater + equal / 2 (ties share the middle rank), mrr = mean 1 / rank,
    hits@K = mean [rank <= K], auc = mean over the queries that have a candidate of
    1 - (greater + equal / 2) / n_cand."""
    gt, eq, nc = n_greater.to(torch.float64), n_equal.to(torch.float64), n_cand.to(torch.float64)
    above = gt + 0.5 * eq
    rank = 1.0 + above
    has = nc > 0
    per_query = torch.where(has, 1.0 - above / torch.where(has, nc, torch.ones_like(nc)), torch.zeros_like(nc))
    out = {"auc": per_query.sum() / has.to(torch.float64).sum(), "mrr": (1.0 / rank).mean()}
    for K in (1, 3, 10):
        out[f"hits@{K}"] = (rank <= K).to(torch.float64).mean()
    return out


def link_full_metrics(z_src: Tensor, z_dst: Tensor, pos: Tensor, known: Tensor = None,
                      segments: LinkSegments = None) -> dict:
    """auc / mrr / hits@1 / hits@3 / hits@10 of the positives against every (filtered) destination, as float64
    device scalars: ``link_full_ranks`` + a few reductions over [E]; no host sync before the caller reads a value.
    ``segments`` (a ``LinkSegments``; A19): against the destinations of each positive's own graph."""
    if segments is not None:
        return full_metrics_from_ranks(*link_full_ranks(z_src, z_dst, pos, known, segments=segments))
    return full_metrics_from_ranks(*link_full_ranks(z_src, z_dst, pos, known))


# ---------------------------------------------------------------------------------------------------
# A16: top-K retrieval (NOT IN REFERENCE)
# ---------------------------------------------------------------------------------------------------
TOPK_MAX = 128


def link_topk(z_src: Tensor, z_dst: Tensor, src: Tensor, k: int, known: Tensor = None, segments: LinkSegments = None):
    """(idx int32 [Q, k], score float32 [Q, k]) (include/hgin.h A16): for every source ``src[q]`` (int64 [Q], repeats
    allowed) the k best destinations c by <z_src[src[q]], z_dst[c]>, minus the c with (src[q], c) in ``known`` (an
    edge index [2, M]; None: unfiltered), ordered by (score descending, index ascending); rows with fewer than k
    candidates are padded with idx -1 / score -inf.  The scores are the bits ``link_full_ranks`` compares; no
    [Q, n_dst] score matrix exists.  1 <= k <= 128.  With ``segments`` (a ``LinkSegments``; include/hgin.h A19) a
    query's candidates are only the destinations of its source's own graph; a source whose graph has no destination
    gets a fully padded row.  No gradient."""
    what = "link_topk"
    for name, z in (("z_src", z_src), ("z_dst", z_dst)):
        if z.dtype != torch.float32:
            raise TypeError(f"{what}: {name} must be float32 (the fused link kernels are fp32 only), got {z.dtype}")
        if z.dim() != 2:
            raise RuntimeError(f"{what}: {name} must be [N, F]")
    if z_src.size(1) != z_dst.size(1):
        raise RuntimeError(f"{what}: embedding widths differ")
    if src.dtype != torch.long or src.dim() != 1:
        raise ValueError(f"{what}: src must be an int64 [Q] tensor, got {src.dtype} {tuple(src.shape)}")
    if segments is not None:
        _check_segments(what, segments, z_src.size(0), z_dst.size(0))
    ops.require_device(z_src, z_dst, src, known, what=what)
    Q, k = int(src.numel()), int(k)
    n_src, n_dst, F = int(z_src.size(0)), int(z_dst.size(0)), int(z_src.size(1))
    if Q < 1 or Q >= 2**31 or not 1 <= k <= TOPK_MAX:
        raise ValueError(f"{what}: need 1 <= Q < 2^31 and 1 <= k <= {TOPK_MAX} (Q = {Q}, k = {k})")
    if F < 1 or n_src < 1 or n_dst < 1:
        raise ValueError(f"{what}: embeddings need at least one row and one feature")
    lo, hi = torch.stack([src.amin(), src.amax()]).tolist()   # the one host sync
    if lo < 0 or hi >= n_src:
        raise IndexError(f"{what}: src index out of range [0, {n_src})")
    z_src, z_dst = ops._rowmajor(z_src.detach()), ops._rowmajor(z_dst.detach())
    src, dev = src.contiguous(), z_src.device
    rowptr = col = None
    if known is not None:
        rowptr, col = _known_csr(known, n_src, n_dst)
    idx = torch.empty((Q, k), dtype=torch.int32, device=dev)
    score = torch.empty((Q, k), dtype=torch.float32, device=dev)
    nbytes = ctypes.c_size_t(0)
    _lib.check(_lib.lib().hgin_link_topk_workspace_size(Q, n_dst, F, k, ctypes.byref(nbytes)),
               "hgin_link_topk_workspace_size")
    ws = ops._workspace(nbytes.value, dev)
    if segments is not None:
        ops.require_device(segments.src_seg, what=what)
        _lib.call("hgin_link_topk_seg_f32", ops._p(src), Q, n_src, n_dst, ops._p(z_src), z_src.stride(0), ops._p(z_dst),
                  z_dst.stride(0), F, ops._p(rowptr), ops._p(col), k, ops._p(idx), ops._p(score), ops._p(ws),
                  nbytes.value, ops._p(segments.src_seg), ops._p(segments.dst_ptr), segments.n_graphs,
                  ops._stream(idx))
        return idx, score
    _lib.call("hgin_link_topk_f32", ops._p(src), Q, n_src, n_dst, ops._p(z_src), z_src.stride(0), ops._p(z_dst),
              z_dst.stride(0), F, ops._p(rowptr), ops._p(col), k, ops._p(idx), ops._p(score), ops._p(ws),
              nbytes.value, ops._stream(idx))
    return idx, score


def hard_negatives(z_src: Tensor, z_dst: Tensor, pos: Tensor, m: int, known: Tensor = None, seed: int = 0,
                   offset: int = 0) -> Tensor:
    """int32 [E, m] (include/hgin.h A18's ``neg_dst``): for every positive (s, d) of ``pos`` the m best-scoring
    destinations of s that are not an edge of ``known`` (an edge index [2, M]; default: ``pos`` itself), best first
    (score descending, index ascending): ``link_topk`` on the unique sources of ``pos``, gathered back per positive.
    A source with fewer than m such destinations leaves padded slots; slot (e, j) is then filled with the uniform
    draw ``sample_negative_dst(E * m, n_dst, seed, offset)[e * m + j]``, which is not filtered and may be a known
    edge (the filtered draws of include/hgin.h A20 do not reach this fill, and the parameter list stays as it is).
    1 <= m <= 128.  No gradient.  ``hard_negatives_seg`` is the graph-local form."""
    return _hard_negatives("hard_negatives", z_src, z_dst, pos, m, known, seed, offset, None)


def hard_negatives_seg(z_src: Tensor, z_dst: Tensor, pos: Tensor, m: int, segments: LinkSegments, known: Tensor = None,
                       seed: int = 0, offset: int = 0) -> Tensor:
    """``hard_negatives`` inside each positive's own graph (``segments``: a ``LinkSegments``; include/hgin.h A19): the
    mining goes through the segmented ``link_topk`` and the padded slots take the segmented draws of the same stream
    (counter offset + e * m + j), so every entry lies in its positive's graph.  A function of its own, and not a
    ``segments=`` on ``hard_negatives``, whose parameter list is a fixed part of the public surface.  The fill is
    unfiltered here too (A20 leaves it alone)."""
    if not isinstance(segments, LinkSegments):
        raise TypeError(f"hard_negatives_seg: segments must be a LinkSegments, got {type(segments).__name__}")
    return _hard_negatives("hard_negatives_seg", z_src, z_dst, pos, m, known, seed, offset, segments)


def _hard_negatives(what, z_src, z_dst, pos, m, known, seed, offset, segments):
    m = int(m)
    if not 1 <= m <= TOPK_MAX:
        raise ValueError(f"{what}: need 1 <= m <= {TOPK_MAX}, got m = {m}")
    ops.check_edge_index(pos)
    E, n_dst = int(pos.size(1)), int(z_dst.size(0))
    if E < 1 or E * m >= 2**31:
        raise ValueError(f"{what}: need E >= 1 and E * m < 2^31 (E = {E}, m = {m})")
    if segments is not None:
        _check_segments(what, segments, z_src.size(0), n_dst, pos)
    ops.require_device(z_src, z_dst, pos, known, what=what)
    src, inverse = torch.unique(pos[0], return_inverse=True)
    if segments is not None:
        idx, _ = link_topk(z_src, z_dst, src, m, pos if known is None else known, segments=segments)
        mined = idx[inverse]
        fill = _sample_seg(pos[0], m, seed, offset, segments).view(E, m)
    else:
        idx, _ = link_topk(z_src, z_dst, src, m, pos if known is None else known)
        mined = idx[inverse]
        fill = sample_negative_dst(E * m, n_dst, seed, offset, mined.device).view(E, m)
    out = torch.where(mined < 0, fill, mined).contiguous()
    _mark_checked(out, n_dst)   # in range by construction: no range-check sync when the set is used
    return out


# ---------------------------------------------------------------------------------------------------
# A23: full-candidate softmax loss (NOT IN REFERENCE)
# ---------------------------------------------------------------------------------------------------
def _distinct_sources(what: str, src: Tensor, n_src: int) -> None:
    """``src`` holds distinct values in [0, n_src): IndexError / ValueError otherwise.  One host sync, once per tensor
    version (cached on the tensor, as ``_given_negatives`` does it)."""
    key = int(n_src)
    cache = getattr(src, "_hgin_distinct", None)
    ver = src._version
    if cache is not None and cache[0] == ver and key in cache[1]:
        return
    srt = torch.sort(src).values
    dup = (srt[1:] == srt[:-1]).any().to(torch.long)
    lo, hi, dup = torch.stack([srt[0], srt[-1], dup]).tolist()
    if lo < 0 or hi >= n_src:
        raise IndexError(f"{what}: src index out of range [0, {n_src})")
    if dup:
        raise ValueError(f"{what}: src must hold distinct sources (a repeated value was found)")
    if cache is None or cache[0] != ver:
        cache = (ver, set())
    cache[1].add(key)
    try:
        src._hgin_distinct = cache
    except (AttributeError, RuntimeError):
        pass


def _lse_operands(what: str, z_src: Tensor, z_dst: Tensor, src: Tensor, temperature, known):
    """Checked operands of ``link_lse`` / ``link_lse_unfused``: (z_src, z_dst, src, inv_t, rowptr, col)."""
    for name, z in (("z_src", z_src), ("z_dst", z_dst)):
        if z.dtype != torch.float32:
            raise TypeError(f"{what}: {name} must be float32 (the fused link kernels are fp32 only), got {z.dtype}")
        if z.dim() != 2:
            raise RuntimeError(f"{what}: {name} must be [N, F]")
    if z_src.size(1) != z_dst.size(1):
        raise RuntimeError(f"{what}: embedding widths differ")
    if not isinstance(src, Tensor) or src.dtype != torch.long or src.dim() != 1:
        got = f"{src.dtype} {tuple(src.shape)}" if isinstance(src, Tensor) else type(src).__name__
        raise ValueError(f"{what}: src must be an int64 [Q] tensor, got {got}")
    temperature = float(temperature)
    if not (math.isfinite(temperature) and temperature > 0.0):
        raise ValueError(f"{what}: temperature must be finite and > 0, got {temperature}")
    if known is not None:
        _known_shape(what, known)
    Q = int(src.numel())
    n_src, n_dst, F = int(z_src.size(0)), int(z_dst.size(0)), int(z_src.size(1))
    if Q < 1 or Q >= 2**31:
        raise ValueError(f"{what}: need 1 <= Q < 2^31 (Q = {Q})")
    if F < 1 or n_src < 1 or n_dst < 1:
        raise ValueError(f"{what}: embeddings need at least one row and one feature")
    src = src.contiguous()
    _distinct_sources(what, src, n_src)      # plain torch: a repeated source is reported wherever the tensor lives
    ops.require_device(z_src, z_dst, src, known, what=what)
    rowptr = col = None
    if known is not None:
        rowptr, col = _known_csr(known, n_src, n_dst)
    inv_t = ctypes.c_float(1.0 / temperature).value    # fl32(1 / temperature), the value the kernels multiply by
    return ops._rowmajor(z_src), ops._rowmajor(z_dst), src, inv_t, rowptr, col


class _LinkLseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z_src, z_dst, src, inv_t: float, rowptr, col, segments=None):
        dev = z_src.device
        Q, n_src, n_dst, F = int(src.numel()), int(z_src.size(0)), int(z_dst.size(0)), int(z_src.size(1))
        nbytes = ctypes.c_size_t(0)
        size = "hgin_link_lse_workspace_size" if segments is None else "hgin_link_lse_seg_workspace_size"
        _lib.check(getattr(_lib.lib(), size)(Q, n_dst, F, ctypes.byref(nbytes)), size)
        ws = ops._workspace(nbytes.value, dev)
        lse = torch.empty(Q, dtype=torch.float32, device=dev)
        if segments is None:
            _lib.call("hgin_link_lse_fwd_f32", ops._p(src), Q, n_src, n_dst, ops._p(z_src), z_src.stride(0),
                      ops._p(z_dst), z_dst.stride(0), F, inv_t, ops._p(rowptr), ops._p(col), ops._p(lse), ops._p(ws),
                      nbytes.value, ops._stream(lse))
        else:
            _lib.call("hgin_link_lse_fwd_seg_f32", ops._p(src), Q, n_src, n_dst, ops._p(z_src), z_src.stride(0),
                      ops._p(z_dst), z_dst.stride(0), F, inv_t, ops._p(rowptr), ops._p(col), ops._p(lse), ops._p(ws),
                      nbytes.value, ops._p(segments.src_seg), ops._p(segments.dst_ptr), segments.n_graphs,
                      ops._stream(lse))
        ctx.inv_t, ctx.ws_bytes, ctx.known, ctx.segments = inv_t, nbytes.value, (rowptr, col), segments
        ctx.save_for_backward(z_src, z_dst, src, lse)
        return lse

    @staticmethod
    def backward(ctx, g):
        z_src, z_dst, src, lse = ctx.saved_tensors
        rowptr, col = ctx.known
        seg = ctx.segments
        g = g.to(torch.float32).contiguous()
        Q, n_src, n_dst, F = int(src.numel()), int(z_src.size(0)), int(z_dst.size(0)), int(z_src.size(1))
        g_src = g_dst = None
        ws = None       # one workspace for both kernels: they run one after the other on this stream
        for i, side in ((0, "src"), (1, "dst")):
            if not ctx.needs_input_grad[i]:
                continue
            out = torch.empty_like(z_src if i == 0 else z_dst, memory_format=torch.contiguous_format)
            if ws is None:
                ws = ops._workspace(ctx.ws_bytes, z_src.device)
            if seg is None:
                _lib.call(f"hgin_link_lse_bwd_{side}_f32", ops._p(src), Q, n_src, n_dst, ops._p(z_src), z_src.stride(0),
                          ops._p(z_dst), z_dst.stride(0), F, ctx.inv_t, ops._p(rowptr), ops._p(col), ops._p(lse),
                          ops._p(g), ops._p(out), out.stride(0), ops._p(ws), ctx.ws_bytes, ops._stream(out))
            else:
                _lib.call(f"hgin_link_lse_bwd_{side}_seg_f32", ops._p(src), Q, n_src, n_dst, ops._p(z_src),
                          z_src.stride(0), ops._p(z_dst), z_dst.stride(0), F, ctx.inv_t, ops._p(rowptr), ops._p(col),
                          ops._p(lse), ops._p(g), ops._p(out), out.stride(0), ops._p(ws), ctx.ws_bytes,
                          ops._p(seg.src_seg), ops._p(seg.dst_ptr), seg.n_graphs, ops._stream(out))
            if i == 0:
                g_src = out
            else:
                g_dst = out
        return g_src, g_dst, None, None, None, None, None


def _lse_segments(what: str, segments, z_src, z_dst) -> None:
    """``segments`` of ``link_lse`` / ``link_lse_unfused``: a ``LinkSegments`` that fits the embeddings' row counts and
    lives on their device (checked before a device is needed)."""
    _check_segments(what, segments, z_src.size(0) if isinstance(z_src, Tensor) and z_src.dim() else -1,
                    z_dst.size(0) if isinstance(z_dst, Tensor) and z_dst.dim() else -1)
    if isinstance(z_src, Tensor) and z_src.device != segments.device:
        raise ValueError(f"{what}: z_src is on {z_src.device}, segments on {segments.device}")


def link_lse(z_src: Tensor, z_dst: Tensor, src: Tensor, temperature: float = 1.0, known: Tensor = None,
             segments: LinkSegments = None) -> Tensor:
    """float32 [Q] (include/hgin.h A23): for every source ``src[q]`` (int64 [Q], distinct: checked once per tensor
    version with one host sync, ValueError) the log-sum-exp over *every* destination c of
    <z_src[src[q]], z_dst[c]> / temperature, minus the c with (src[q], c) in ``known`` (an edge index [2, M]; None: every
    destination); -inf for a source whose destinations are all known.  The scores are the bits ``link_full_ranks`` /
    ``link_topk`` compare; no [Q, n_dst] matrix exists in the forward or in the backward (two kernels that recompute the
    scores, csrc/hgin_linklse.hip); forward and gradients are run-to-run identical.

    With ``segments`` (a ``LinkSegments``; include/hgin.h A24) the sum runs only over the destinations of the source's
    own graph: known neighbours outside it are irrelevant, a source whose graph has no destination gives -inf and no
    gradient, and a block of 128 queries sweeps only the destination tiles its graphs cover, so sort ``src`` by graph
    to visit n_dst / G instead of n_dst (any order is correct).  One graph gives the unsegmented bits."""
    what = "link_lse"
    if segments is not None:
        _lse_segments(what, segments, z_src, z_dst)
    z_src, z_dst, src, inv_t, rowptr, col = _lse_operands(what, z_src, z_dst, src, temperature, known)
    return _LinkLseFn.apply(z_src, z_dst, src, inv_t, rowptr, col, segments)


LSE_UNFUSED_BYTES = 1 << 30     # fp32 scores per chunk of the unfused baseline


def link_lse_unfused(z_src: Tensor, z_dst: Tensor, src: Tensor, temperature: float = 1.0, known: Tensor = None,
                     chunk_rows: int = None, segments: LinkSegments = None) -> Tensor:
    """``link_lse`` as plain torch, the kept baseline the fused path is checked and timed against: chunks of query rows
    (about 1 GB of fp32 scores each, or ``chunk_rows``) of ``z_src[src] @ z_dst.T * fl32(1 / temperature)``, known edges
    (and, with ``segments``, the columns outside the source's own graph) set to -inf, ``torch.logsumexp``.  It
    materialises a chunk of the [Q, n_dst] matrix, and autograd keeps it."""
    what = "link_lse_unfused"
    if segments is not None:
        _lse_segments(what, segments, z_src, z_dst)
    z_src, z_dst, src, inv_t, rowptr, col = _lse_operands(what, z_src, z_dst, src, temperature, known)
    Q, n_dst = int(src.numel()), int(z_dst.size(0))
    rows = int(chunk_rows) if chunk_rows else max(1, LSE_UNFUSED_BYTES // (4 * n_dst))
    out = []
    for a in range(0, Q, rows):
        s = src[a:a + rows]
        t = (z_src[s] @ z_dst.t()) * inv_t
        if rowptr is not None:
            beg, end = rowptr[s].long(), rowptr[s + 1].long()
            deg = end - beg
            qi = torch.repeat_interleave(torch.arange(s.numel(), device=s.device), deg)
            first = torch.repeat_interleave(beg - (torch.cumsum(deg, 0) - deg), deg)
            ci = col[(torch.arange(qi.numel(), device=s.device) + first)].long() if qi.numel() else qi
            mask = torch.zeros_like(t, dtype=torch.bool)
            mask[qi, ci] = True
            t = t.masked_fill(mask, float("-inf"))
        if segments is not None:
            gph = segments.src_seg[s].long()
            ptr = segments.dst_ptr.long()
            c = torch.arange(n_dst, device=s.device)
            outside = (c[None, :] < ptr[gph][:, None]) | (c[None, :] >= ptr[gph + 1][:, None])
            t = t.masked_fill(outside, float("-inf"))
        out.append(torch.logsumexp(t, 1))
    return torch.cat(out)


def _full_softmax_plan(pos: Tensor, known: Optional[Tensor], n_src: int, n_dst: int):
    """(u, cnt, known u pos or None) of the positives, cached on ``pos`` per (its version, ``known`` and its version): u
    the distinct sources in ascending order, cnt how many positives each has."""
    cache = getattr(pos, "_hgin_full_softmax", None)
    ver = pos._version
    if cache is not None and cache[0] == ver and cache[1] == (n_src, n_dst) and \
            (cache[2] is None) == (known is None) and \
            (known is None or (cache[2]() is known and cache[3] == known._version)):
        return cache[4]
    u, cnt = torch.unique(pos[0], return_counts=True)
    try:
        u._hgin_distinct = (u._version, {int(n_src)})   # distinct by construction, in range by relation_graph's check
    except (AttributeError, RuntimeError):
        pass
    both = None if known is None else torch.cat([known, pos], 1)
    plan = (u, cnt.to(torch.float32), both)
    try:
        pos._hgin_full_softmax = (ver, (n_src, n_dst), None if known is None else weakref.ref(known),
                                  None if known is None else known._version, plan)
    except (AttributeError, RuntimeError):
        pass
    return plan


def full_softmax_link_loss(z_src: Tensor, z_dst: Tensor, pos: Tensor, temperature: float = 1.0,
                           known: Tensor = None, segments: LinkSegments = None) -> Tensor:
    """Softmax cross-entropy of every positive (s, d) of ``pos`` (int64 [2, E]) against *every* destination (a scalar):
    mean over the positives of log sum_c exp(score(s, c) / T) - score(s, d) / T, on ``link_lse`` (one query per distinct
    source) and ``dot_decode``.  ``known`` = None: the sum runs over every destination,
    loss = (sum_q cnt_q lse_q - sum_e s_e) / E.  With ``known`` (an edge index [2, M]) a source's other true edges leave
    the denominator while the positive stays in its own: lse_neg = ``link_lse`` filtered by ``known`` and ``pos``
    together, loss = mean_e softplus(lse_neg[s_e] - s_e).  Deterministic forward and backward: the per-positive read of
    lse_neg is a ``dot_decode`` of a one-column embedding against a column of ones, whose backward is the store-and-sum
    over the static CSC of ``pos``.  With ``segments`` (a ``LinkSegments``; include/hgin.h A24) "every destination" is
    every destination of the positive's own graph, the denominator ``link_full_metrics(segments=)`` ranks against; a
    positive whose destination lies outside its source's graph is refused (ValueError)."""
    what = "full_softmax_link_loss"
    if segments is not None:
        _check_segments(what, segments, z_src.size(0) if z_src.dim() else -1, z_dst.size(0) if z_dst.dim() else -1,
                        pos if isinstance(pos, Tensor) and pos.dim() == 2 and pos.dtype == torch.long else None)
    for name, z in (("z_src", z_src), ("z_dst", z_dst)):
        if z.dtype != torch.float32:
            raise TypeError(f"{what}: {name} must be float32 (the fused link kernels are fp32 only), got {z.dtype}")
    temperature = float(temperature)
    if not (math.isfinite(temperature) and temperature > 0.0):
        raise ValueError(f"{what}: temperature must be finite and > 0, got {temperature}")
    if known is not None:
        _known_shape(what, known)
    ops.require_device(z_src, z_dst, pos, known, what=what)
    ops.check_edge_index(pos)
    E = int(pos.size(1))
    if E < 1:
        raise ValueError(f"{what}: need E >= 1")
    n_src, n_dst = int(z_src.size(0)), int(z_dst.size(0))
    s_e = dot_decode(z_src, z_dst, pos) * ctypes.c_float(1.0 / temperature).value   # range-checks pos (relation_graph)
    u, cnt, both = _full_softmax_plan(pos, known, n_src, n_dst)
    if known is None:
        lse = link_lse(z_src, z_dst, u, temperature, segments=segments)
        return ((cnt * lse).sum() - s_e.sum()) / E
    lse_neg = link_lse(z_src, z_dst, u, temperature, known=both, segments=segments)
    col = torch.zeros(n_src, dtype=torch.float32, device=z_src.device).index_copy(0, u, lse_neg)
    ones = torch.ones(n_dst, 1, dtype=torch.float32, device=z_src.device)
    lse_e = dot_decode(col.unsqueeze(1), ones, pos)     # lse_neg of every positive's source: x * 1.0 is exact
    return torch.nn.functional.softplus(lse_e - s_e).mean()


class LinkPredictor:
    """Link-prediction head over a model's node embeddings: ``relation`` = (src_type, name, dst_type), k uniform
    negatives per positive, dot-product decoder, and the training objective of ``sampled_link_loss`` ("bce" by
    default; "softmax" with ``temperature``, "bpr", "selfadv" with ``alpha``).  The objective only shapes ``loss``;
    ``metrics``, ``full_metrics`` and ``predict`` do not depend on it.

    ``hard`` = m > 0 adds m mined negatives per positive (``hard_negatives``, filtered by the relation's edges) to
    the k uniform ones, and k may then be 0.  The set is kept as ``self.neg_dst``; ``loss`` re-mines it from the
    step's own embeddings every ``mine_every`` steps (0: only ``mine`` changes it once it exists).

    ``graph_local`` = True is for a collated batch of independent graphs (``hgin.data.collate``, ``component_graph``):
    ``LinkSegments.of(graph, relation)`` is built once per graph object and passed to ``loss``, ``mine``, ``metrics``,
    ``full_metrics`` and ``predict``, so negatives, candidates and proposals stay inside each positive's / source's own
    graph (include/hgin.h A19).  The default treats the destinations as one pool, as before.

    ``filter_negatives`` = True draws the uniform negatives of ``loss`` and ``metrics`` from each source's
    non-neighbours (include/hgin.h A20): ``known`` = the relation's edges in the graph, or what the call's own
    ``known=`` gives (train + valid + test edges for held-out positives).  It composes with ``graph_local``, ``hard``
    (whose mined set is filtered by the relation's edges already; its padding fill is not) and every objective.

    ``exclude_targets`` = True makes ``batch_loss`` and ``batch_full_loss`` build their mini-batch with
    ``link_neighbor_batch_excl`` (include/hgin.h A25): the batch's positives, and their flips in ``rev_relation``
    (``"auto"``, None or a relation, resolved against the sampler's graph as ``link_split`` resolves it), are not edges
    of the neighbourhood that batch is encoded on.  Drawn or given negatives are seeds, never excluded pairs.  The
    default leaves every output as it was."""

    def __init__(self, model, relation, k: int, seed: int, objective: str = "bce", temperature: float = 1.0,
                 alpha: float = 1.0, hard: int = 0, mine_every: int = 1, graph_local: bool = False,
                 filter_negatives: bool = False, exclude_targets: bool = False, rev_relation="auto"):
        if not hasattr(model, "encode"):
            raise TypeError("LinkPredictor: the model has no encode(x_dict, edge_index_dict)")
        _objective("LinkPredictor", objective, temperature, alpha)
        hard, mine_every = int(hard), int(mine_every)
        if not 0 <= hard <= TOPK_MAX:
            raise ValueError(f"LinkPredictor: hard must be in [0, {TOPK_MAX}], got {hard}")
        if mine_every < 0:
            raise ValueError(f"LinkPredictor: mine_every must be >= 0, got {mine_every}")
        if int(k) < (0 if hard else 1):
            raise ValueError(f"LinkPredictor: need k >= 1, or k >= 0 with hard >= 1 (k = {int(k)}, hard = {hard})")
        self.model, self.relation, self.k, self.seed = model, tuple(relation), int(k), int(seed)
        self.objective, self.temperature, self.alpha = objective, float(temperature), float(alpha)
        self.hard, self.mine_every = hard, mine_every
        self.neg_dst = None       # the mined set, int32 [E, hard], of the positives self._mined_for
        self._mined_for = None
        self.graph_local = bool(graph_local)
        self._segments = None     # (graph, its LinkSegments) of the last graph seen with graph_local
        self.filter_negatives = bool(filter_negatives)
        self.exclude_targets = bool(exclude_targets)
        self.rev_relation = rev_relation

    def _batch(self, sampler, pos, neg, step) -> "LinkBatch":
        """The mini-batch of ``batch_loss`` / ``batch_full_loss``: ``link_neighbor_batch``, or with ``exclude_targets``
        ``link_neighbor_batch_excl`` (the positives and their flips leave the batch's own neighbourhood)."""
        if self.exclude_targets:
            return link_neighbor_batch_excl(sampler, self.relation, pos, neg, offset=int(step),
                                            rev_relation=self.rev_relation)
        return link_neighbor_batch(sampler, self.relation, pos, neg, offset=int(step))

    def _seg_kw(self, graph) -> dict:
        """{} by default (every call below is then exactly the unsegmented one), {"segments": ...} with graph_local."""
        if not self.graph_local:
            return {}
        if self._segments is None or self._segments[0] is not graph:
            self._segments = (graph, LinkSegments.of(graph, self.relation))
        return {"segments": self._segments[1]}

    def _known_kw(self, graph, known) -> dict:
        """{} by default (the calls below then carry no ``known`` keyword at all); {"known": ...} when the call gives
        one or ``filter_negatives`` is set (then the relation's own edges)."""
        if known is not None:
            return {"known": known}
        return {"known": graph.edge_index[self.relation]} if self.filter_negatives else {}

    def _pos(self, graph, pos):
        return graph.edge_index[self.relation] if pos is None else pos

    def _mine(self, z, graph, pos, known, offset):
        """Padded slots are filled from the stream of seed + 1, apart from the uniform negatives' (seed)."""
        if known is None:
            known = graph.edge_index[self.relation]
        zs, zd = z[self.relation[0]].detach(), z[self.relation[2]].detach()
        if self.graph_local:
            self.neg_dst = hard_negatives_seg(zs, zd, pos, self.hard, self._seg_kw(graph)["segments"], known,
                                              self.seed + 1, offset)
        else:
            self.neg_dst = hard_negatives(zs, zd, pos, self.hard, known, self.seed + 1, offset)
        self._mined_for = pos
        return self.neg_dst

    def loss(self, graph, pos: Tensor = None, step: int = 0, known: Tensor = None) -> Tensor:
        """The sampled loss of ``pos`` (default: the relation's own edges); step s draws the negatives at
        offset s * E * k, so every step sees fresh ones.  With ``hard`` > 0 the mined set joins them; it is mined
        again from this step's embeddings (detached; no second encode) when ``mine_every`` > 0 divides the step, or
        when there is none for this ``pos`` yet (padded slots: draws at offset s * E * hard).  ``known`` (an edge
        index; default with ``filter_negatives``: the relation's own edges) filters the uniform draws (A20)."""
        pos = self._pos(graph, pos)
        z = self.model.encode(graph.x_dict(), graph.edge_index_dict())
        offset = int(step) * int(pos.size(1)) * self.k
        if self.hard == 0:
            return sampled_link_loss(z[self.relation[0]], z[self.relation[2]], pos, self.k, self.seed, offset,
                                     self.objective, self.temperature, self.alpha, **self._seg_kw(graph),
                                     **self._known_kw(graph, known))
        if self.neg_dst is None or self._mined_for is not pos or \
                (self.mine_every > 0 and int(step) % self.mine_every == 0):
            self._mine(z, graph, pos, None, int(step) * int(pos.size(1)) * self.hard)
        return sampled_link_loss(z[self.relation[0]], z[self.relation[2]], pos, self.k, self.seed, offset,
                                 self.objective, self.temperature, self.alpha, neg_dst=self.neg_dst,
                                 **self._seg_kw(graph), **self._known_kw(graph, known))

    def mine(self, graph, pos: Tensor = None, known: Tensor = None) -> Tensor:
        """Mine ``self.neg_dst`` now, from an eval-mode encode without gradients (the mode is restored), as
        ``metrics`` encodes: ``hard`` negatives per positive of ``pos`` (default: the relation's own edges), filtered
        by ``known`` (default: the relation's own edges).  Returns the set."""
        if self.hard == 0:
            raise ValueError("LinkPredictor.mine: the predictor was built with hard = 0")
        pos = self._pos(graph, pos)
        was_training = self.model.training
        self.model.eval()
        try:
            with torch.no_grad():
                z = self.model.encode(graph.x_dict(), graph.edge_index_dict())
                return self._mine(z, graph, pos, known, 0)
        finally:
            self.model.train(was_training)

    def metrics(self, graph, pos: Tensor = None, neg_dst: Tensor = None, known: Tensor = None) -> dict:
        """``link_metrics`` of the model's embeddings in eval mode, without gradients (the mode is restored);
        ``neg_dst`` (integer [E, m]) is an evaluation set ranked along with the k uniform draws.  ``known`` (an edge
        index; default with ``filter_negatives``: the relation's own edges) filters the uniform draws (A20)."""
        pos = self._pos(graph, pos)
        was_training = self.model.training
        self.model.eval()
        try:
            with torch.no_grad():
                z = self.model.encode(graph.x_dict(), graph.edge_index_dict())
                if neg_dst is not None:
                    return link_metrics(z[self.relation[0]], z[self.relation[2]], pos, self.k, self.seed,
                                        neg_dst=neg_dst, **self._seg_kw(graph), **self._known_kw(graph, known))
                return link_metrics(z[self.relation[0]], z[self.relation[2]], pos, self.k, self.seed,
                                    **self._seg_kw(graph), **self._known_kw(graph, known))
        finally:
            self.model.train(was_training)

    def full_metrics(self, graph, pos: Tensor = None, known: Tensor = None) -> dict:
        """``link_full_metrics`` of the model's embeddings in eval mode, without gradients (the mode is restored):
        ``pos`` (default: the relation's own edges) ranked against every destination, filtered by ``known`` (default:
        the relation's own edges in ``graph``; for held-out positives pass train + valid + test edges)."""
        pos = self._pos(graph, pos)
        if known is None:
            known = graph.edge_index[self.relation]
        was_training = self.model.training
        self.model.eval()
        try:
            with torch.no_grad():
                z = self.model.encode(graph.x_dict(), graph.edge_index_dict())
                return link_full_metrics(z[self.relation[0]], z[self.relation[2]], pos, known, **self._seg_kw(graph))
        finally:
            self.model.train(was_training)

    def predict(self, graph, src: Tensor = None, k: int = 10, known: Tensor = None):
        """``link_topk`` of the model's embeddings in eval mode, without gradients (the mode is restored): the k best
        destinations of every source in ``src`` (default: every source node of the relation), minus ``known``
        (default: the relation's own edges in ``graph``, so only new links are proposed)."""
        if known is None:
            known = graph.edge_index[self.relation]
        was_training = self.model.training
        self.model.eval()
        try:
            with torch.no_grad():
                z = self.model.encode(graph.x_dict(), graph.edge_index_dict())
                z_src, z_dst = z[self.relation[0]], z[self.relation[2]]
                if src is None:
                    src = torch.arange(z_src.size(0), dtype=torch.long, device=z_src.device)
                return link_topk(z_src, z_dst, src, k, known, **self._seg_kw(graph))
        finally:
            self.model.train(was_training)

    def batch_loss(self, sampler, pos: Tensor, step: int = 0, known: Tensor = None) -> Tensor:
        """``loss`` on a neighbour-sampled mini-batch (include/hgin.h A22): the k negatives of every positive of ``pos``
        (global int64 [2, B]) are drawn as ``loss`` draws them (``negative_edges`` with ``seed``, offset step * B * k,
        and ``known=`` / ``filter_negatives``: the relation's edges of ``sampler.graph``), ``link_neighbor_batch`` samples
        the neighbourhood of the sources, destinations and negatives with ``offset=step``, the model encodes that
        subgraph only, and the fused loss scores the local pairs with the negatives as given ones.  With
        ``fanouts = [-1] * layers`` this is ``loss(sampler.graph, pos, step, known)`` up to summation order.
        ``hard`` > 0 and ``graph_local`` are not supported here (ValueError)."""
        what = "LinkPredictor.batch_loss"
        if self.hard > 0 or self.graph_local:
            raise ValueError(f"{what}: hard > 0 and graph_local = True are not supported on sampled mini-batches")
        from .neighbor import NeighborSampler
        if not isinstance(sampler, NeighborSampler):
            raise TypeError(f"{what}: sampler must be a NeighborSampler, got {type(sampler).__name__}")
        if self.relation[0] not in sampler.num_nodes or self.relation[2] not in sampler.num_nodes:
            raise ValueError(f"{what}: the sampler's graph lacks a node type of {self.relation!r}")
        if not isinstance(pos, Tensor) or pos.dtype != torch.long:
            got = pos.dtype if isinstance(pos, Tensor) else type(pos).__name__
            raise TypeError(f"{what}: pos must be an int64 edge index [2, B], got {got}")
        if pos.dim() != 2 or int(pos.size(0)) != 2 or int(pos.size(1)) < 1:
            raise ValueError(f"{what}: pos must be [2, B] with B >= 1, got {tuple(pos.shape)}")
        B, n_dst = int(pos.size(1)), sampler.num_nodes[self.relation[2]]
        if known is None and self.filter_negatives:
            if self.relation not in sampler.graph.edge_index:
                raise ValueError(f"{what}: the sampler's graph has no relation {self.relation!r} to filter by")
            known = sampler.graph.edge_index[self.relation]
        if known is not None:
            _known_shape(what, known)
        ops.require_device(pos, known, what=what)
        if B * self.k >= 2**31:
            raise ValueError(f"{what}: need B * k < 2^31 (B = {B}, k = {self.k})")
        # negative_edges' destinations, with the known CSR keyed by the graph's row count (cached on ``known``)
        draw_at = int(step) * B * self.k
        if known is None:
            neg = sample_negative_dst(B * self.k, n_dst, self.seed, draw_at, pos.device)
        else:
            csr = _known_csr(known, sampler.num_nodes[self.relation[0]], n_dst)
            neg = _sample_filt(pos[0], self.k, self.seed, draw_at, n_dst, None, csr)
        neg = neg.view(B, self.k)
        batch = self._batch(sampler, pos, neg, step)
        g = batch.sub.graph
        z = self.model.encode(g.x_dict(), g.edge_index_dict())
        return sampled_link_loss(z[self.relation[0]], z[self.relation[2]], batch.pos, 0, self.seed, 0, self.objective,
                                 self.temperature, self.alpha, neg_dst=batch.neg_dst)

    def _no_full(self, what: str) -> None:
        if self.hard > 0 or self.graph_local:
            raise ValueError(f"{what}: hard > 0 and graph_local = True are not supported by the full softmax loss")

    def full_loss(self, graph, pos: Tensor = None, known: Tensor = None, segments: LinkSegments = None) -> Tensor:
        """``full_softmax_link_loss`` of ``pos`` (default: the relation's own edges) at the predictor's ``temperature``:
        every positive against every destination of the graph (include/hgin.h A23); k, seed and the objective play no
        part.  ``known`` (an edge index; default with ``filter_negatives``: the relation's own edges) takes a source's
        other true edges out of the denominator.  On a collated batch of graphs pass
        ``segments=LinkSegments.of(graph, relation)`` (include/hgin.h A24): every positive then stands against the
        destinations of its own graph only, the denominator ``full_metrics`` of a ``graph_local`` predictor ranks
        against.  ``segments=`` is the way in: ``hard`` > 0 and a predictor built with ``graph_local`` are still refused
        (ValueError)."""
        self._no_full("LinkPredictor.full_loss")
        if segments is not None and not isinstance(segments, LinkSegments):
            raise TypeError(f"LinkPredictor.full_loss: segments must be a LinkSegments, got {type(segments).__name__}")
        pos = self._pos(graph, pos)
        z = self.model.encode(graph.x_dict(), graph.edge_index_dict())
        if segments is not None:
            return full_softmax_link_loss(z[self.relation[0]], z[self.relation[2]], pos, self.temperature,
                                          segments=segments, **self._known_kw(graph, known))
        return full_softmax_link_loss(z[self.relation[0]], z[self.relation[2]], pos, self.temperature,
                                      **self._known_kw(graph, known))

    def batch_full_loss(self, sampler, pos: Tensor, step: int = 0, known: Tensor = None) -> Tensor:
        """The softmax loss with in-batch negatives on a neighbour-sampled mini-batch: ``link_neighbor_batch`` seeds the
        sampler with the positives ``pos`` (global int64 [2, B]) alone (``offset=step``), the model encodes that subgraph,
        and every positive is scored against the destination-type seeds of the batch (the leading rows of the local
        embedding: a slice, no gather) with ``full_softmax_link_loss``.  The batch's own positives are always known
        edges (a source's other positives leave its denominator); with ``known=`` or ``filter_negatives`` (the relation's
        edges of ``sampler.graph``) so are the known edges whose endpoints are both seeds
        (``SampledSubgraph.local_edges``).  ``hard`` > 0 and ``graph_local`` are not supported (ValueError)."""
        what = "LinkPredictor.batch_full_loss"
        self._no_full(what)
        from .neighbor import NeighborSampler
        if not isinstance(sampler, NeighborSampler):
            raise TypeError(f"{what}: sampler must be a NeighborSampler, got {type(sampler).__name__}")
        if self.relation[0] not in sampler.num_nodes or self.relation[2] not in sampler.num_nodes:
            raise ValueError(f"{what}: the sampler's graph lacks a node type of {self.relation!r}")
        if not isinstance(pos, Tensor) or pos.dtype != torch.long:
            got = pos.dtype if isinstance(pos, Tensor) else type(pos).__name__
            raise TypeError(f"{what}: pos must be an int64 edge index [2, B], got {got}")
        if pos.dim() != 2 or int(pos.size(0)) != 2 or int(pos.size(1)) < 1:
            raise ValueError(f"{what}: pos must be [2, B] with B >= 1, got {tuple(pos.shape)}")
        if known is None and self.filter_negatives:
            if self.relation not in sampler.graph.edge_index:
                raise ValueError(f"{what}: the sampler's graph has no relation {self.relation!r} to filter by")
            known = sampler.graph.edge_index[self.relation]
        if known is not None:
            _known_shape(what, known)
        ops.require_device(pos, known, what=what)
        s_type, d_type = self.relation[0], self.relation[2]
        batch = self._batch(sampler, pos, None, step)
        g = batch.sub.graph
        z = self.model.encode(g.x_dict(), g.edge_index_dict())
        local_known = batch.pos
        if known is not None:
            local_known = torch.cat([batch.pos, batch.sub.local_edges(s_type, d_type, known)], 1)
        return full_softmax_link_loss(z[s_type], z[d_type][:batch.sub.n_seed[d_type]], batch.pos, self.temperature,
                                      known=local_known)


class LinkBatch(NamedTuple):
    """``link_neighbor_batch``'s result: ``sub`` the ``SampledSubgraph``, ``pos`` the positives as local rows (int64
    [2, B]), ``neg_dst`` the given negatives as local destination rows (int32 [B, m], range-checked) or None."""

    sub: object
    pos: Tensor
    neg_dst: Optional[Tensor]


def link_neighbor_batch(sampler, relation, pos: Tensor, neg_dst: Tensor = None, offset: int = 0) -> LinkBatch:
    """The neighbour-sampled mini-batch of the positives ``pos`` (global int64 [2, B]) of ``relation`` = (src_type,
    name, dst_type): the seeds are ``pos[0]`` (sources), ``pos[1]`` and, when given, the global integer [B, m]
    ``neg_dst`` (destinations); ``offset`` is the batch number of ``NeighborSampler.sample``.  Every endpoint is a seed,
    so its local row is found by a binary search in the sorted seed block, without a host read."""
    what = "link_neighbor_batch"
    relation = tuple(relation)
    if len(relation) != 3:
        raise ValueError(f"{what}: relation must be (src_type, name, dst_type), got {relation!r}")
    if not isinstance(pos, Tensor) or pos.dtype != torch.long:
        got = pos.dtype if isinstance(pos, Tensor) else type(pos).__name__
        raise TypeError(f"{what}: pos must be an int64 edge index [2, B], got {got}")
    if pos.dim() != 2 or int(pos.size(0)) != 2:
        raise ValueError(f"{what}: pos must be [2, B], got {tuple(pos.shape)}")
    return _link_batch(what, sampler, relation, pos, neg_dst, offset, None)


def _link_batch(what, sampler, relation, pos, neg_dst, offset, exclude) -> LinkBatch:
    """``link_neighbor_batch``'s body; ``exclude`` = None samples with ``sampler.sample``, a dict with
    ``sampler.sample_excluding``."""
    m = _given_shape(what, neg_dst, pos)
    s_type, d_type = relation[0], relation[2]
    dst = pos[1] if m == 0 else torch.cat([pos[1], neg_dst.reshape(-1).long()])
    seeds = {s_type: torch.cat([pos[0], dst])} if s_type == d_type else {s_type: pos[0], d_type: dst}
    if exclude is None:
        sub = sampler.sample(seeds, offset=offset)
    else:
        sub = sampler.sample_excluding(seeds, exclude, offset=offset)
    local = torch.stack([sub._rows(s_type, pos[0]), sub._rows(d_type, pos[1])])
    neg_local = None
    if m:
        neg_local = sub._rows(d_type, neg_dst.long().contiguous()).to(torch.int32)
        _mark_checked(neg_local, int(sub.n_id[d_type].numel()))
    return LinkBatch(sub, local, neg_local)


def link_neighbor_batch_excl(sampler, relation, pos: Tensor, neg_dst: Tensor = None, offset: int = 0,
                             rev_relation="auto") -> LinkBatch:
    """``link_neighbor_batch`` without the batch's own target edges (include/hgin.h A25): the seeds are the same, and
    the subgraph comes from ``sampler.sample_excluding`` with the pairs ``pos`` in ``relation`` and their flips
    ``pos.flip(0)`` in ``rev_relation``, each only where the sampler convolves over that relation.  ``rev_relation`` is
    resolved against ``sampler.graph`` as ``link_split`` resolves it: ``"auto"`` = the one relation (dst_type, *,
    src_type), none when there is no such relation, ValueError when there are several; None = none; or a relation.
    The negatives ``neg_dst`` are seeds, never excluded pairs."""
    from .linksplit import _reverse_of
    from .neighbor import NeighborSampler
    what = "link_neighbor_batch_excl"
    if not isinstance(sampler, NeighborSampler):
        raise TypeError(f"{what}: sampler must be a NeighborSampler, got {type(sampler).__name__}")
    relation = tuple(relation)
    if len(relation) != 3:
        raise ValueError(f"{what}: relation must be (src_type, name, dst_type), got {relation!r}")
    if not isinstance(pos, Tensor) or pos.dtype != torch.long:
        got = pos.dtype if isinstance(pos, Tensor) else type(pos).__name__
        raise TypeError(f"{what}: pos must be an int64 edge index [2, B], got {got}")
    if pos.dim() != 2 or int(pos.size(0)) != 2:
        raise ValueError(f"{what}: pos must be [2, B], got {tuple(pos.shape)}")
    rev = _reverse_of(what, sampler.graph, relation, rev_relation)
    exclude = {}
    if relation in sampler.relations:
        exclude[relation] = pos
    if rev is not None and rev in sampler.relations:
        exclude[rev] = pos.flip(0)
    return _link_batch(what, sampler, relation, pos, neg_dst, offset, exclude)

