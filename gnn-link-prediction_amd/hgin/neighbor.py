"""Neighbour-sampled mini-batches (include/hgin.h A22) on libhgin.so.

NOT IN REFERENCE (the reference trains on whole graphs).  ``LinkPredictor.loss`` encodes the whole graph for every
optimizer step; ``NeighborSampler`` cuts the sampled L-hop neighbourhood of a batch's endpoints out of a resident graph
instead, relabelled to local rows, so that the encoder convolves only the edges the batch can reach:

    sampler = hgin.NeighborSampler(graph, fanouts=[10, 5], seed=0)
    sub = sampler.sample({"path": p_ids, "link": l_ids}, offset=step)
    z = model.encode(sub.graph.x_dict(), sub.graph.edge_index_dict())     # rows sub.local(type, ids) are the seeds'

The picks (Floyd's subset algorithm on Philox words), the test of sampled sources against the rows already in the batch
and the relabelled edge lists are HIP kernels (csrc/hgin_neighbor.hip); ``unique`` of a hop's candidates, the row gathers
``x[n_id]`` and the host reads of sizes are torch.  A batch costs one host read for the seed range check, one per hop for
the hop's edge counts, and the size read inside every ``torch.unique`` (one per type for the seeds and per hop).

Messages flow over whatever is in the sampler's graph.  Where the supervised positives of a batch are edges of it,
``sample_excluding`` (include/hgin.h A25) leaves them out of that batch's neighbourhood, at every hop and in every
relation that is given pairs (``hgin.link_neighbor_batch_excl`` passes the positives and their flips in the reverse
relation; ``LinkPredictor(exclude_targets=True)`` does so for every training batch):

    sub = sampler.sample_excluding(seeds, {REL_PL: pos, REL_LP: pos.flip(0)}, offset=step)

The pairs become sorted keys dst * 2^32 + src (one ``torch.sort`` per relation and batch); the pick kernels drop a row's
excluded positions and draw the fanout from what is left, so the graph and its CSRs are never rebuilt.  The alternative
that needs no per-batch work is ``hgin.link_split(..., disjoint=...)``, which sets a fixed share of the training edges
aside as supervision-only positives for the whole run.
"""
from __future__ import annotations

import ctypes
import numbers
from dataclasses import dataclass
from typing import Dict, List, Optional

import torch
from torch import Tensor

from . import _lib, ops

FANOUT_MAX = 128


def _fanouts(what: str, fanouts) -> List[int]:
    if not isinstance(fanouts, list):
        raise TypeError(f"{what}: fanouts must be a list of integers, got {type(fanouts).__name__}")
    if not fanouts:
        raise ValueError(f"{what}: fanouts must name at least one hop")
    out = []
    for f in fanouts:
        if isinstance(f, bool) or not isinstance(f, numbers.Integral):
            raise TypeError(f"{what}: a fanout must be an integer, got {type(f).__name__}")
        f = int(f)
        if f != -1 and not 1 <= f <= FANOUT_MAX:
            raise ValueError(f"{what}: a fanout must be -1 (every neighbour) or in [1, {FANOUT_MAX}], got {f}")
        out.append(f)
    return out


@dataclass
class SampledSubgraph:
    """What ``NeighborSampler.sample`` returns.  ``graph``: a ``HeteroGraph`` of the local rows (``x`` / ``y`` / ``batch``
    gathered, ``static_features`` off, a local int64 ``edge_index`` for every sampled relation); ``n_id`` {type: int64
    [n_local]}: the global id of every local row; ``e_id`` {relation: int64 [E_r]}: the original position of every local
    edge; ``n_seed`` {type: int}: the leading rows that are the batch's seeds (unique, ascending)."""

    graph: object
    n_id: Dict[str, Tensor]
    e_id: Dict[tuple, Tensor]
    n_seed: Dict[str, int]

    def _rows(self, node_type: str, ids: Tensor) -> Tensor:
        """Local rows of global ids known to be seeds: a binary search in the sorted seed block, no check, no sync."""
        seeds = self.n_id[node_type][:self.n_seed[node_type]]
        return torch.searchsorted(seeds, ids.contiguous())

    def local(self, node_type: str, ids: Tensor) -> Tensor:
        """Local rows (int64, the shape of ``ids``) of global ids that are seeds of the batch; IndexError for an id that
        is not (one host read)."""
        if node_type not in self.n_id:
            raise ValueError(f"SampledSubgraph.local: unknown node type {node_type!r}")
        if not isinstance(ids, Tensor) or ids.dtype not in (torch.int32, torch.int64):
            got = ids.dtype if isinstance(ids, Tensor) else type(ids).__name__
            raise TypeError(f"SampledSubgraph.local: ids must be an int32 or int64 tensor, got {got}")
        ids = ids.long()
        n = self.n_seed[node_type]
        if ids.numel() == 0:
            return torch.empty_like(ids)
        if n == 0:
            raise IndexError(f"SampledSubgraph.local: the batch has no {node_type!r} seeds")
        rows = self._rows(node_type, ids)
        seeds = self.n_id[node_type][:n]
        if bool((seeds[rows.clamp(max=n - 1)] != ids).any()):
            raise IndexError(f"SampledSubgraph.local: an id is not a {node_type!r} seed of this batch")
        return rows

    def local_edges(self, src_type: str, dst_type: str, edge_index: Tensor) -> Tensor:
        """The edges of the global int64 ``edge_index`` [2, M] (sources of ``src_type``, destinations of ``dst_type``)
        whose endpoints are both seeds of the batch, relabelled to local rows (int64 [2, M']; order kept): a binary
        search into the two sorted seed blocks plus an equality test, in torch; no value is read on the host."""
        for t in (src_type, dst_type):
            if t not in self.n_id:
                raise ValueError(f"SampledSubgraph.local_edges: unknown node type {t!r}")
        if not isinstance(edge_index, Tensor) or edge_index.dtype != torch.int64:
            got = edge_index.dtype if isinstance(edge_index, Tensor) else type(edge_index).__name__
            raise TypeError(f"SampledSubgraph.local_edges: edge_index must be an int64 tensor, got {got}")
        if edge_index.dim() != 2 or int(edge_index.size(0)) != 2:
            raise ValueError(f"SampledSubgraph.local_edges: edge_index must be [2, M], got {tuple(edge_index.shape)}")
        ns, nd = self.n_seed[src_type], self.n_seed[dst_type]
        if ns == 0 or nd == 0 or edge_index.size(1) == 0:
            return edge_index.new_empty((2, 0))
        s_seeds, d_seeds = self.n_id[src_type][:ns], self.n_id[dst_type][:nd]
        rs = torch.searchsorted(s_seeds, edge_index[0].contiguous()).clamp_(max=ns - 1)
        rd = torch.searchsorted(d_seeds, edge_index[1].contiguous()).clamp_(max=nd - 1)
        keep = (s_seeds[rs] == edge_index[0]) & (d_seeds[rd] == edge_index[1])
        return torch.stack([rs[keep], rd[keep]])


class NeighborSampler:
    """Samples the L-hop neighbourhood of a batch of seed nodes out of ``graph`` (include/hgin.h A22).

    ``fanouts`` = [f_1 .. f_L]: in-neighbours kept per expanded node and relation at each hop (1 .. 128, or -1 = all);
    ``relations``: the relations messages flow over (default: every key of ``graph.edge_index``, in that order; the slot
    of a relation in this list enters its Philox counter); ``seed``: the sampler's Philox key.  The CSRs come from
    ``ops.relation_graph`` (cached on the edge tensors).  A dense global -> local map per node type stays resident on the
    device between calls; it is clean again whenever ``sample`` returns or raises."""

    def __init__(self, graph, fanouts, relations=None, seed: int = 0):
        from .store import PaddedBatch
        what = "NeighborSampler"
        if isinstance(graph, PaddedBatch):
            raise ValueError(f"{what}: a PaddedBatch is not supported (its tensors are padded and refilled in place)")
        self.fanouts = _fanouts(what, fanouts)
        if isinstance(seed, bool) or not isinstance(seed, numbers.Integral):
            raise TypeError(f"{what}: seed must be an integer, got {type(seed).__name__}")
        self.seed = int(seed) & (2**64 - 1)
        if relations is None:
            relations = list(graph.edge_index.keys())
        elif not isinstance(relations, (list, tuple)):
            raise TypeError(f"{what}: relations must be a list of (src_type, name, dst_type), got "
                            f"{type(relations).__name__}")
        self.relations = [tuple(r) for r in relations]
        for r in self.relations:
            if r not in graph.edge_index:
                raise ValueError(f"{what}: the graph has no relation {r!r}")
            if r[0] not in graph.x or r[2] not in graph.x:
                raise ValueError(f"{what}: relation {r!r} names a node type the graph has no features for")
            e = graph.edge_index[r]
            if not isinstance(e, Tensor) or e.dtype != torch.int64:
                raise TypeError(f"{what}: edge_index of {r!r} must be an int64 tensor")
            if e.dim() != 2 or int(e.size(0)) != 2:
                raise ValueError(f"{what}: edge_index of {r!r} must be [2, E], got {tuple(e.shape)}")
        if len(set(self.relations)) != len(self.relations):
            raise ValueError(f"{what}: a relation is named twice")
        self.graph = graph
        self.types = list(graph.x.keys())
        self.num_nodes = {t: int(graph.x[t].size(0)) for t in self.types}
        for t, n in self.num_nodes.items():
            if n >= 2**31:
                raise ValueError(f"{what}: more than 2^31 {t!r} nodes")
        self._maps: Dict[str, Tensor] = {}

    # -------------------------------------------------------------------------------------------------
    def _check_seeds(self, seeds, offset, exclude=None, what="NeighborSampler.sample") -> Dict[str, Tensor]:
        if not isinstance(seeds, dict):
            raise TypeError(f"{what}: seeds must be a dict {{type: int64 ids}}, got {type(seeds).__name__}")
        if isinstance(offset, bool) or not isinstance(offset, numbers.Integral):
            raise TypeError(f"{what}: offset must be an integer, got {type(offset).__name__}")
        if not 0 <= int(offset) < 2**32:
            raise ValueError(f"{what}: offset (the batch number) must be in [0, 2^32), got {int(offset)}")
        out = {}
        for t, ids in seeds.items():
            if t not in self.num_nodes:
                raise ValueError(f"{what}: unknown node type {t!r}")
            if not isinstance(ids, Tensor) or ids.dtype != torch.int64:
                got = ids.dtype if isinstance(ids, Tensor) else type(ids).__name__
                raise TypeError(f"{what}: seeds of {t!r} must be an int64 tensor, got {got}")
            if ids.dim() != 1:
                raise ValueError(f"{what}: seeds of {t!r} must be one-dimensional, got {tuple(ids.shape)}")
            if ids.numel():
                out[t] = ids
        ranged = [(f"a {t!r} seed", ids, self.num_nodes[t]) for t, ids in out.items()]
        for r, e in (exclude or {}).items():   # the excluded pairs' ids join the one host read
            ranged += [(f"an excluded {r[0]!r} source of {r!r}", e[0], self.num_nodes[r[0]]),
                       (f"an excluded {r[2]!r} destination of {r!r}", e[1], self.num_nodes[r[2]])]
        devs = {v.device for _, v, _ in ranged}
        if len(devs) > 1:
            raise ValueError(f"{what}: seeds{' and excluded pairs' if exclude else ''} live on several devices "
                             f"{sorted(map(str, devs))}")
        if ranged:   # the one host read of the check
            lo_hi = torch.stack([torch.stack([v.amin(), v.amax()]) for _, v, _ in ranged]).tolist()
            for (name, _, n), (lo, hi) in zip(ranged, lo_hi):
                if lo < 0 or hi >= n:
                    raise IndexError(f"{what}: {name} is out of range [0, {n})")
        return out

    def _check_exclude(self, exclude, what) -> Dict[tuple, Tensor]:
        """{relation: int64 [2, M]} with M > 0 of ``exclude``, types and shapes checked (no value is read)."""
        if not isinstance(exclude, dict):
            raise TypeError(f"{what}: exclude must be a dict {{relation: int64 [2, M] pairs}}, got "
                            f"{type(exclude).__name__}")
        out = {}
        for r, e in exclude.items():
            if not isinstance(r, tuple) or r not in self.relations:
                raise ValueError(f"{what}: {r!r} is not a relation of this sampler")
            if not isinstance(e, Tensor) or e.dtype != torch.int64:
                got = e.dtype if isinstance(e, Tensor) else type(e).__name__
                raise TypeError(f"{what}: the excluded pairs of {r!r} must be an int64 tensor, got {got}")
            if e.dim() != 2 or int(e.size(0)) != 2:
                raise ValueError(f"{what}: the excluded pairs of {r!r} must be [2, M], got {tuple(e.shape)}")
            if e.size(1):
                out[r] = e
        return out

    def _device(self):
        for t in self.types:
            return self.graph.x[t].device
        raise ValueError("NeighborSampler: the graph has no node types")

    def _map(self, t: str, dev) -> Tensor:
        m = self._maps.get(t)
        if m is None or m.device != dev:
            m = self._maps[t] = torch.full((max(self.num_nodes[t], 1),), -1, dtype=torch.int32, device=dev)
        return m

    def _map_set(self, t: str, dev, ids: Tensor, base: int) -> None:
        if ids.numel():
            _lib.call("hgin_neighbor_map_set", ops._p(self._map(t, dev)), self.num_nodes[t], ops._p(ids),
                      int(ids.numel()), int(base), ops._stream(ids))

    def sample(self, seeds: Dict[str, Tensor], offset: int = 0) -> "SampledSubgraph":
        """The subgraph of include/hgin.h A22 around ``seeds`` = {type: int64 global ids} (repeats allowed, a type may
        be absent), for batch number ``offset`` (the second Philox counter word)."""
        return self._sample("NeighborSampler.sample", seeds, {}, offset)

    def sample_excluding(self, seeds: Dict[str, Tensor], exclude: Dict[tuple, Tensor],
                         offset: int = 0) -> "SampledSubgraph":
        """``sample`` without the edges of ``exclude`` = {relation: int64 [2, M]}, global (src, dst) pairs in that
        relation's own orientation (include/hgin.h A25): no edge of an excluded pair (no copy of a multi-edge) is in the
        subgraph, at any hop; a row's fanout is drawn from what is left of it.  A relation without an entry is sampled by
        the A22 entry points; an empty dict (or only empty entries) returns exactly what ``sample`` returns.  The keys
        dst * 2^32 + src are sorted on the device; the pairs' range check joins the seeds' one host read."""
        what = "NeighborSampler.sample_excluding"
        return self._sample(what, seeds, self._check_exclude(exclude, what), offset)

    def _sample(self, what: str, seeds, exclude: Dict[tuple, Tensor], offset) -> "SampledSubgraph":
        from .data import HeteroGraph
        seeds = self._check_seeds(seeds, offset, exclude, what)
        g = self.graph
        ops.require_device(*seeds.values(), *exclude.values(), *g.x.values(),
                           *[g.edge_index[r] for r in self.relations], what=what)
        dev = self._device()
        for ids in seeds.values():
            if ids.device != dev:
                raise ValueError(f"{what}: seeds are on {ids.device}, the graph on {dev}")
        for r, e in exclude.items():
            if e.device != dev:
                raise ValueError(f"{what}: the excluded pairs of {r!r} are on {e.device}, the graph on {dev}")
        offset = int(offset)
        # A25's keys, ascending: destination (the CSR row) in the high word, source in the low one
        excl = {r: torch.sort((e[1] << 32) | e[0]).values for r, e in exclude.items()}
        csr = {r: ops.relation_graph(g.edge_index[r], self.num_nodes[r[0]], self.num_nodes[r[2]]).csr
               for r in self.relations}
        empty = torch.empty(0, dtype=torch.int64, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        rows: Dict[str, List[Tensor]] = {t: [] for t in self.types}    # the blocks of n_id, in local-row order
        count = {t: 0 for t in self.types}
        edges: Dict[tuple, List[Tensor]] = {r: [] for r in self.relations}
        eids: Dict[tuple, List[Tensor]] = {r: [] for r in self.relations}
        try:
            frontier, front_base = {}, {}
            for t in self.types:
                u = torch.unique(seeds[t]) if t in seeds else empty
                self._map_set(t, dev, u, 0)
                rows[t].append(u)
                frontier[t], front_base[t], count[t] = u, 0, int(u.numel())
            n_seed = dict(count)
            for f in self.fanouts:
                jobs = []
                for slot, r in enumerate(self.relations):
                    fr = frontier[r[2]]
                    n = int(fr.numel())
                    if n == 0:
                        continue
                    off = torch.empty(n + 1, dtype=torch.int64, device=dev)
                    size = ctypes.c_size_t(0)
                    _lib.call("hgin_neighbor_sample_workspace_size", n, ctypes.byref(size))
                    ws = ops._workspace(size.value, dev)
                    if r in excl:
                        _lib.call("hgin_neighbor_sample_offsets_excl", ops._p(csr[r].rowptr), ops._p(csr[r].col),
                                  csr[r].n_rows, ops._p(fr), n, f, ops._p(excl[r]), int(excl[r].numel()), ops._p(off),
                                  ops._p(ws), size.value, stream)
                    else:
                        _lib.call("hgin_neighbor_sample_offsets", ops._p(csr[r].rowptr), csr[r].n_rows, ops._p(fr), n,
                                  f, ops._p(off), ops._p(ws), size.value, stream)
                    jobs.append((slot, r, fr, off))
                if not jobs:
                    break
                totals = torch.stack([j[3][-1] for j in jobs]).tolist()   # the hop's one host read
                cand: Dict[str, List[Tensor]] = {t: [] for t in self.types}
                drawn = []
                for (slot, r, fr, off), tot in zip(jobs, totals):
                    tot = int(tot)
                    if tot == 0:
                        continue
                    n = int(fr.numel())
                    src = torch.empty(tot, dtype=torch.int64, device=dev)
                    eid = torch.empty(tot, dtype=torch.int64, device=dev)
                    c = csr[r]
                    if r in excl:
                        _lib.call("hgin_neighbor_sample_excl", ops._p(c.rowptr), ops._p(c.col), ops._p(c.perm),
                                  c.n_rows, ops._p(fr), n, f, self.seed, offset, slot, ops._p(excl[r]),
                                  int(excl[r].numel()), ops._p(off), ops._p(src), ops._p(eid), tot, stream)
                    else:
                        _lib.call("hgin_neighbor_sample", ops._p(c.rowptr), ops._p(c.col), ops._p(c.perm), c.n_rows,
                                  ops._p(fr), n, f, self.seed, offset, slot, ops._p(off), ops._p(src), ops._p(eid),
                                  tot, stream)
                    new = torch.empty(tot, dtype=torch.int64, device=dev)
                    _lib.call("hgin_neighbor_fresh", ops._p(self._map(r[0], dev)), self.num_nodes[r[0]], ops._p(src),
                              tot, self.num_nodes[r[0]], ops._p(new), stream)
                    cand[r[0]].append(new)
                    drawn.append((r, fr, off, src, eid, tot))
                nxt, nxt_base = {}, {}
                for t in self.types:
                    u = empty
                    if cand[t]:
                        # the sentinel (= the node count, above every id) is appended so that it is always the last
                        # unique value and can be dropped without reading anything back
                        sent = torch.full((1,), self.num_nodes[t], dtype=torch.int64, device=dev)
                        u = torch.unique(torch.cat(cand[t] + [sent]))[:-1]
                    self._map_set(t, dev, u, count[t])
                    if u.numel():
                        rows[t].append(u)
                    nxt[t], nxt_base[t] = u, count[t]
                    count[t] += int(u.numel())
                for r, fr, off, src, eid, tot in drawn:
                    out = torch.empty((2, tot), dtype=torch.int64, device=dev)
                    _lib.call("hgin_neighbor_emit", ops._p(self._map(r[0], dev)), self.num_nodes[r[0]], ops._p(src),
                              ops._p(off), int(fr.numel()), front_base[r[2]], tot, ops._p(out), stream)
                    edges[r].append(out)
                    eids[r].append(eid)
                frontier, front_base = nxt, nxt_base
        finally:
            for t in self.types:
                for ids in rows[t]:
                    self._map_set(t, dev, ids, -1)

        n_id = {t: (torch.cat(rows[t]) if len(rows[t]) > 1 else rows[t][0]) for t in self.types}
        cat = lambda parts, shape: (torch.cat(parts, -1) if len(parts) > 1 else parts[0]) if parts else \
            torch.empty(shape, dtype=torch.int64, device=dev)   # noqa: E731
        edge_index = {r: cat(edges[r], (2, 0)) for r in self.relations}
        e_id = {r: cat(eids[r], (0,)) for r in self.relations}
        x = {t: g.x[t][n_id[t]] for t in self.types}
        y = g.y
        for t in self.types:   # the labels follow the node type they have one row for (the paths)
            if isinstance(y, Tensor) and y.dim() >= 1 and int(y.size(0)) == self.num_nodes[t] and \
                    (t == "path" or "path" not in self.num_nodes):
                y = g.y[n_id[t]]
                break
        batch = {t: b[n_id[t]] for t, b in g.batch.items() if t in n_id}
        sub = HeteroGraph(x, edge_index, y, batch)
        sub.static_features = False     # per-batch tensors: nothing to cache across steps
        return SampledSubgraph(sub, n_id, e_id, n_seed)
