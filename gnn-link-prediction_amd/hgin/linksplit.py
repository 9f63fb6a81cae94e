"""Leakage-free train / valid / test edge splits for link prediction (include/hgin.h A21) on libhgin.so.

NOT IN REFERENCE (the reference regresses path delay and holds no edge out).  ``LinkPredictor.loss`` / ``metrics`` /
``full_metrics`` / ``predict`` encode the graph they are given; when that graph still holds the positives being scored,
the encoder passes messages over the very edges the decoder is asked about.  ``link_split`` removes them:

    split = hgin.link_split(graph, REL_PL, val=0.1, test=0.1, seed=7)
    pred = hgin.LinkPredictor(model, REL_PL, k=8, seed=1)
    for step in range(steps):
        hgin.link_train_step(model, opt, split.train_graph, pred, step, pos=split.train_pos)
    pred.full_metrics(split.val_graph, pos=split.val_pos, known=split.known)
    pred.full_metrics(split.test_graph, pos=split.test_pos, known=split.known)

The part of an edge is a function of its endpoint pair (one Philox evaluation, counter = {s, d, 1, 0}, key = seed), not
of its position: part 3 = test, 2 = valid, 1 = train edges used for supervision only (``disjoint`` > 0), 0 = train edges
that carry messages.  So a pair and its flipped twin in the reverse relation land in the same part without a join, every
copy of a multi-edge lands in the same part, and the part does not depend on edge order.  Part sizes are binomial, not
exact counts.  The selection is a stable compaction on the device (the output keeps the input order, which the
bit-reproducible aggregates need), not ``torch.rand`` + boolean indexing.
"""
from __future__ import annotations

import ctypes
import math
import numbers
from dataclasses import dataclass
from typing import Iterable, Optional, Tuple

import torch
from torch import Tensor

from . import _lib, ops

TWO32 = 1 << 32
_COUNTS = "_hgin_split_counts"


def _fraction(what: str, name: str, v) -> float:
    if isinstance(v, bool) or not isinstance(v, numbers.Real):
        raise TypeError(f"{what}: {name} must be a real number in [0, 1], got {type(v).__name__}")
    v = float(v)
    if not 0.0 <= v <= 1.0:      # also refuses NaN
        raise ValueError(f"{what}: {name} must be in [0, 1], got {v}")
    return v


def split_bounds(val, test, disjoint=0.0, what: str = "link_split") -> Tuple[int, int, int]:
    """(b_test, b_val, b_sup) of include/hgin.h A21: floor(test 2^32), floor((test + val) 2^32), floor(disjoint 2^32).
    TypeError / ValueError for fractions outside [0, 1] or val + test > 1."""
    val, test = _fraction(what, "val", val), _fraction(what, "test", test)
    disjoint = _fraction(what, "disjoint", disjoint)
    if test + val > 1.0:
        raise ValueError(f"{what}: val + test must be at most 1, got {val} + {test}")
    return int(math.floor(test * TWO32)), int(math.floor((test + val) * TWO32)), int(math.floor(disjoint * TWO32))


def _seed(what: str, seed) -> int:
    if isinstance(seed, bool) or not isinstance(seed, numbers.Integral):
        raise TypeError(f"{what}: seed must be an integer, got {type(seed).__name__}")
    return int(seed) & (2**64 - 1)


def _edge_shape(what: str, edge_index) -> int:
    """E of an int64 [2, E] edge index; TypeError / ValueError otherwise.  Shapes and dtypes only: no device needed."""
    if not isinstance(edge_index, Tensor) or edge_index.dtype != torch.int64:
        got = edge_index.dtype if isinstance(edge_index, Tensor) else type(edge_index).__name__
        raise TypeError(f"{what}: edge_index must be an int64 tensor, got {got}")
    if edge_index.dim() != 2 or int(edge_index.size(0)) != 2:
        raise ValueError(f"{what}: edge_index must be [2, E], got {tuple(edge_index.shape)}")
    return int(edge_index.size(1))


def _keep_mask(what: str, keep: Iterable[int]) -> int:
    mask = 0
    for p in keep:
        if isinstance(p, bool) or not isinstance(p, numbers.Integral):
            raise TypeError(f"{what}: keep must hold part numbers 0..3, got {type(p).__name__}")
        if not 0 <= int(p) <= 3:
            raise ValueError(f"{what}: keep must hold part numbers 0..3, got {int(p)}")
        mask |= 1 << int(p)
    return mask


def split_geometry() -> Tuple[int, int]:
    """(tile_edges, scan_width) of the selection kernels in this build."""
    t, w = ctypes.c_int(0), ctypes.c_int(0)
    _lib.call("hgin_link_split_geometry", ctypes.byref(t), ctypes.byref(w))
    return int(t.value), int(w.value)


def _parts(what: str, edge_index: Tensor, seed: int, bounds, swap: bool) -> Tuple[Tensor, Tensor]:
    ops.require_device(edge_index, what=what)
    E = int(edge_index.size(1))
    ei = edge_index.contiguous()
    part = torch.empty(E, dtype=torch.uint8, device=ei.device)
    counts = torch.zeros(4, dtype=torch.int64, device=ei.device)
    if E:
        _lib.call("hgin_link_split_parts", ops._p(ei), E, int(bool(swap)), seed, bounds[0], bounds[1], bounds[2],
                  ops._p(part), ops._p(counts), ops._stream(ei))
    try:
        setattr(part, _COUNTS, (part._version, counts))
    except (AttributeError, RuntimeError):
        pass
    return part, counts


def link_split_parts(edge_index: Tensor, seed: int, val, test, disjoint=0.0, swap: bool = False
                     ) -> Tuple[Tensor, Tensor]:
    """(part uint8 [E], counts int64 [4] on the device) of include/hgin.h A21 for an int64 [2, E] edge index: 3 = test,
    2 = valid, 1 = train supervision only, 0 = train message.  ``swap`` = True reads the edges as (d, s), for the reverse
    relation: ``link_split_parts(ei.flip(0), ..., swap=True)`` equals ``link_split_parts(ei, ...)``."""
    what = "link_split_parts"
    bounds = split_bounds(val, test, disjoint, what)
    seed = _seed(what, seed)
    _edge_shape(what, edge_index)
    return _parts(what, edge_index, seed, bounds, swap)


def _select(what: str, edge_index: Tensor, part: Tensor, mask: int, n_out: int) -> Tuple[Tensor, Tensor]:
    E = int(edge_index.size(1))
    ei = edge_index.contiguous()
    out = torch.empty(2, n_out, dtype=torch.int64, device=ei.device)
    eid = torch.empty(n_out, dtype=torch.int64, device=ei.device)
    if E:
        size = ctypes.c_size_t(0)
        _lib.call("hgin_link_split_select_workspace_size", E, ctypes.byref(size))
        ws = torch.empty(int(size.value), dtype=torch.uint8, device=ei.device)
        _lib.call("hgin_link_split_select", ops._p(ei), ops._p(part), E, mask, ops._p(out), ops._p(eid), n_out,
                  ops._p(ws), int(size.value), ops._stream(ei))
    return out, eid


def _part_counts(part: Tensor) -> Tensor:
    """The histogram of ``part``: what ``link_split_parts`` left on it while the tensor is unchanged, else counted."""
    cached = getattr(part, _COUNTS, None)
    if cached is not None and cached[0] == part._version:
        return cached[1]
    return torch.bincount(part.to(torch.int64) & 3, minlength=4)


def link_split_select(edge_index: Tensor, part: Tensor, keep: Iterable[int]) -> Tuple[Tensor, Tensor]:
    """(edge_index_out int64 [2, n], eid int64 [n]): the edges whose part is in ``keep`` (an iterable of part numbers),
    in input order, and their original positions.  Costs one host read of the part counts to size the output."""
    what = "link_split_select"
    E = _edge_shape(what, edge_index)
    if not isinstance(part, Tensor) or part.dtype != torch.uint8:
        got = part.dtype if isinstance(part, Tensor) else type(part).__name__
        raise TypeError(f"{what}: part must be a uint8 tensor, got {got}")
    if part.dim() != 1 or int(part.size(0)) != E:
        raise ValueError(f"{what}: part must be [E] with E = {E}, got {tuple(part.shape)}")
    mask = _keep_mask(what, keep)
    ops.require_device(edge_index, part, what=what)
    part = part.contiguous() if not part.is_contiguous() else part
    counts = _part_counts(part).tolist()
    n_out = sum(int(c) for p, c in enumerate(counts) if (mask >> p) & 1)
    return _select(what, edge_index, part, mask, n_out)


@dataclass
class LinkSplit:
    """What ``link_split`` returns.  ``train_graph`` / ``val_graph`` / ``test_graph`` are ``HeteroGraph``s whose split
    relation (and its reverse) holds parts {0} / {0, 1} / {0, 1, 2}; ``x``, ``y``, ``batch`` and every other relation's
    edge tensor are the input graph's own objects.  ``train_pos`` / ``val_pos`` / ``test_pos`` are the positives to score
    against them (parts {1}, or ``train_graph``'s own edge tensor when ``disjoint`` = 0; {2}; {3}), ``known`` the
    relation's original edge tensor (every true edge, for filtered ranking and filtered negatives), ``counts`` the four
    part sizes (host ints), ``part`` the relation's part codes and ``*_eid`` the original positions of the edges of
    ``train_graph``'s relation and of the three positive sets."""

    relation: tuple
    rev_relation: Optional[tuple]
    train_graph: object
    val_graph: object
    test_graph: object
    train_pos: Tensor
    val_pos: Tensor
    test_pos: Tensor
    known: Tensor
    counts: Tuple[int, int, int, int]
    part: Tensor
    train_eid: Tensor
    train_pos_eid: Tensor
    val_pos_eid: Tensor
    test_pos_eid: Tensor


def _reverse_of(what: str, graph, relation, rev_relation):
    if rev_relation is None:
        return None
    if isinstance(rev_relation, str):
        if rev_relation != "auto":
            raise ValueError(f"{what}: rev_relation must be \"auto\", None or a relation, got {rev_relation!r}")
        found = [r for r in graph.edge_index if r[0] == relation[2] and r[2] == relation[0] and r != relation]
        if len(found) > 1:
            raise ValueError(f"{what}: several relations run from {relation[2]!r} to {relation[0]!r} ({found}); "
                             f"name the reverse one, or pass None")
        return found[0] if found else None
    rev_relation = tuple(rev_relation)
    if rev_relation not in graph.edge_index:
        raise ValueError(f"{what}: the graph has no relation {rev_relation!r}")
    if rev_relation == relation or rev_relation[0] != relation[2] or rev_relation[2] != relation[0]:
        raise ValueError(f"{what}: {rev_relation!r} does not run from {relation[2]!r} to {relation[0]!r}")
    return rev_relation


def link_split(graph, relation, rev_relation="auto", val=0.1, test=0.1, disjoint=0.0, seed: int = 0) -> LinkSplit:
    """Split ``relation`` of ``graph`` into train / valid / test edges by endpoint pair (include/hgin.h A21) and take the
    held-out edges out of the relation and of ``rev_relation`` (``"auto"``: the one relation (dst_type, *, src_type) of
    the graph, none when there is no such relation, ValueError when there are several; None: none).  ``val`` / ``test``
    are the expected fractions of the pairs held out; ``disjoint`` > 0 also sets that fraction of the remaining train
    pairs aside as supervision-only positives, which ``train_graph`` does not pass messages over.  See ``LinkSplit``.

    Each of the three graphs caches its own CSR and, for a resident graph, its own first-layer aggregate (they are keyed
    by the relation's edge tensor); with ``disjoint`` = 0 ``val_graph`` shares ``train_graph``'s tensors and caches."""
    from .data import HeteroGraph
    from .store import PaddedBatch
    what = "link_split"
    if isinstance(graph, PaddedBatch):
        raise ValueError("link_split: a PaddedBatch is not supported (its edge lists are padded and refilled in place)")
    bounds = split_bounds(val, test, disjoint, what)
    seed = _seed(what, seed)
    relation = tuple(relation)
    if relation not in graph.edge_index:
        raise ValueError(f"{what}: the graph has no relation {relation!r}")
    rev = _reverse_of(what, graph, relation, rev_relation)
    fwd_ei = graph.edge_index[relation]
    _edge_shape(what, fwd_ei)
    if rev is not None:
        _edge_shape(what, graph.edge_index[rev])

    part, counts_dev = _parts(what, fwd_ei, seed, bounds, False)
    counts = tuple(int(c) for c in counts_dev.tolist())
    size = lambda parts: sum(counts[p] for p in parts)  # noqa: E731
    sel = lambda parts: _select(what, fwd_ei, part, _keep_mask(what, parts), size(parts))  # noqa: E731
    has_sup = bounds[2] > 0
    train_ei, train_eid = sel((0,))
    val_ei = sel((0, 1))[0] if has_sup else train_ei
    test_ei = sel((0, 1, 2))[0]
    train_pos, train_pos_eid = sel((1,)) if has_sup else (train_ei, train_eid)
    val_pos, val_pos_eid = sel((2,))
    test_pos, test_pos_eid = sel((3,))

    rels = {"train": {relation: train_ei}, "val": {relation: val_ei}, "test": {relation: test_ei}}
    if rev is not None:
        rev_ei = graph.edge_index[rev]
        rpart, rcounts_dev = _parts(what, rev_ei, seed, bounds, True)
        rcounts = [int(c) for c in rcounts_dev.tolist()]
        rsel = lambda parts: _select(what, rev_ei, rpart, _keep_mask(what, parts),  # noqa: E731
                                     sum(rcounts[p] for p in parts))[0]
        rels["train"][rev] = rsel((0,))
        rels["val"][rev] = rsel((0, 1)) if has_sup else rels["train"][rev]
        rels["test"][rev] = rsel((0, 1, 2))

    def variant(own):
        g = HeteroGraph(dict(graph.x), {r: own.get(r, e) for r, e in graph.edge_index.items()}, graph.y,
                        dict(graph.batch))
        if not graph.static_features:       # features refilled in place stay volatile in the variants
            g.static_features = False
        return g

    return LinkSplit(relation, rev, variant(rels["train"]), variant(rels["val"]), variant(rels["test"]), train_pos,
                     val_pos, test_pos, fwd_ei, counts, part, train_eid, train_pos_eid, val_pos_eid, test_pos_eid)
