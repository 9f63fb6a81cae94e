"""Neighbour-sampled mini-batches (include/hgin.h A22), host side: the numpy restatement of the sampling and subgraph
rules on the C oracle's Philox (``ref_picks`` / ``ref_sample``, which tests/test_gpu_neighbor.py pins the kernels to bit
for bit), the properties the rule is chosen for, its uniformity, the Python surface and the argument checks, all without
a device."""
import ctypes
import functools
import inspect
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

from oracle import c_oracle

NEW_SYMBOLS = ("hgin_neighbor_sample_workspace_size", "hgin_neighbor_sample_offsets", "hgin_neighbor_sample",
               "hgin_neighbor_fresh", "hgin_neighbor_map_set", "hgin_neighbor_emit")


@functools.lru_cache(maxsize=1 << 20)
def _block(v, offset, word3, seed):
    """philox4x32_10(counter = {lo32(v), offset, 2, word3}, key = {lo32(seed), hi32(seed)}) as four ints."""
    seed &= (1 << 64) - 1
    x = c_oracle.philox4x32_10([v & 0xFFFFFFFF, offset & 0xFFFFFFFF, 2, word3 & 0xFFFFFFFF],
                               [seed & 0xFFFFFFFF, seed >> 32])
    return tuple(int(w) for w in x)


def ref_picks_d(d, v, f, seed, offset, r_slot):
    """The ascending CSR positions picked for frontier node ``v`` whose row has ``d`` entries (include/hgin.h A22)."""
    if f == -1 or d <= f:
        return list(range(d))
    picked = set()
    for i in range(f):
        J = d - f + i
        w = _block(v, offset, r_slot * 64 + (i >> 2), seed)[i & 3]
        t = (w * (J + 1)) >> 32
        picked.add(J if t in picked else t)
    return sorted(picked)


def ref_picks(rowptr, v, f, seed, offset, r_slot):
    return ref_picks_d(int(rowptr[v + 1]) - int(rowptr[v]), v, f, seed, offset, r_slot)


def ref_csr(edge_index, n_dst):
    """(rowptr, col, perm) of the stable CSR by destination of an int64 [2, E] edge index (array or tensor)."""
    ei = np.asarray(edge_index.cpu().numpy() if isinstance(edge_index, torch.Tensor) else edge_index, dtype=np.int64)
    perm = np.argsort(ei[1], kind="stable")
    rowptr = np.zeros(n_dst + 1, dtype=np.int64)
    np.cumsum(np.bincount(ei[1], minlength=n_dst), out=rowptr[1:])
    return rowptr, ei[0][perm], perm


def ref_sample(graph, relations, fanouts, seeds, seed, offset):
    """(n_id {type: int64 array}, edges {relation: int64 [2, E_r]}, e_id {relation: int64 [E_r]}, n_seed {type: int}) of
    include/hgin.h A22 for a HeteroGraph of CPU tensors, ``seeds`` = {type: iterable of global ids}."""
    types = list(graph.x.keys())
    relations = [tuple(r) for r in relations]
    csr = {r: ref_csr(graph.edge_index[r], int(graph.x[r[2]].shape[0])) for r in relations}
    rows = {t: sorted(set(int(i) for i in np.asarray(seeds.get(t, ())).reshape(-1))) for t in types}
    local = {t: {g: i for i, g in enumerate(rows[t])} for t in types}
    n_seed = {t: len(rows[t]) for t in types}
    frontier = {t: list(rows[t]) for t in types}
    out = {r: ([], [], []) for r in relations}      # global src, local dst, e_id
    for f in fanouts:
        reached = {t: set() for t in types}
        for slot, r in enumerate(relations):
            rowptr, col, perm = csr[r]
            for v in frontier[r[2]]:
                for p in ref_picks(rowptr, v, f, seed, offset, slot):
                    s = int(col[rowptr[v] + p])
                    out[r][0].append(s)
                    out[r][1].append(local[r[2]][v])
                    out[r][2].append(int(perm[rowptr[v] + p]))
                    if s not in local[r[0]]:
                        reached[r[0]].add(s)
        frontier = {}
        for t in types:
            new = sorted(reached[t])
            for g in new:
                local[t][g] = len(rows[t])
                rows[t].append(g)
            frontier[t] = new
    n_id = {t: np.asarray(rows[t], dtype=np.int64) for t in types}
    edges = {r: np.asarray([[local[r[0]][s] for s in out[r][0]], out[r][1]], dtype=np.int64).reshape(2, -1)
             for r in relations}
    e_id = {r: np.asarray(out[r][2], dtype=np.int64) for r in relations}
    return n_id, edges, e_id, n_seed


# ---------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------
def test_counter_word_two_is_2():
    """Words 2 of the samplers' and the split rule's counters are 0 and 1; this stream's is 2."""
    zero = [int(v) for v in c_oracle.philox4x32_10([0, 0, 0, 0], [0, 0])]
    assert zero == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    two = [int(v) for v in c_oracle.philox4x32_10([0, 0, 2, 0], [0, 0])]
    assert _block(0, 0, 0, 0) == tuple(two) and two != zero
    assert two != [int(v) for v in c_oracle.philox4x32_10([0, 0, 1, 0], [0, 0])]
    # the first pick of d = 10, f = 1 is hi32(word 0 * 10) of exactly that block
    assert ref_picks_d(10, 0, 1, 0, 0, 0) == [(two[0] * 10) >> 32]
    # pick i >= 4 reads block r_slot * 64 + (i >> 2)
    five = ref_picks_d(1000, 3, 5, 9, 4, 2)
    w4 = _block(3, 4, 2 * 64 + 1, 9)[0]
    t4 = (w4 * 1000) >> 32
    assert t4 in five or 999 in five


@pytest.mark.parametrize("f", [1, 3, 5, 32, 128])
def test_picks_are_distinct_ascending_and_in_range(f):
    for d in (0, 1, f - 1, f, f + 1, 2 * f + 1, 300, 5000):
        if d < 0:
            continue
        for v in (0, 17, 2**31 - 1):
            p = ref_picks_d(d, v, f, 0xABCDEF0123, 3, 1)
            assert len(p) == min(d, f)
            assert p == sorted(set(p))
            assert all(0 <= q < d for q in p)
            if d <= f:
                assert p == list(range(d))
    assert ref_picks_d(300, 5, -1, 1, 2, 3) == list(range(300))


def test_picks_depend_only_on_seed_offset_slot_and_node():
    rowptr = np.array([0, 40, 40, 95, 400], dtype=np.int64)
    base = ref_picks(rowptr, 3, 5, 7, 2, 1)
    assert base == ref_picks_d(305, 3, 5, 7, 2, 1)
    assert base != ref_picks(rowptr, 3, 5, 7, 3, 1)       # offset
    assert base != ref_picks(rowptr, 3, 5, 7, 2, 2)       # r_slot
    assert base != ref_picks(rowptr, 3, 5, 8, 2, 1)       # seed
    assert base != ref_picks(rowptr, 3, 5, 7 + (1 << 32), 2, 1)   # the seed's high word is part of the key
    assert ref_picks(rowptr, 1, 5, 7, 2, 1) == []


def _tiny_graph():
    from hgin.data import CONFIGS, scaled_config, synthetic_graph
    return synthetic_graph(scaled_config(CONFIGS["cfg1"], 0.1), seed=3)


def test_a_nodes_edges_do_not_change_with_frontier_order_or_batch_content():
    from hgin.data import CONV_RELATIONS
    g = _tiny_graph()
    a = ref_sample(g, CONV_RELATIONS, [2], {"link": [3, 7, 11]}, 5, 1)
    b = ref_sample(g, CONV_RELATIONS, [2], {"link": [11, 3, 3, 20, 7], "path": [4]}, 5, 1)
    for r in CONV_RELATIONS:
        if r[2] != "link":
            continue
        for v in (3, 7, 11):
            ea = a[2][r][a[1][r][1] == list(a[0]["link"]).index(v)]
            eb = b[2][r][b[1][r][1] == list(b[0]["link"]).index(v)]
            assert np.array_equal(ea, eb)


def test_ref_sample_structure():
    """Seeds first and sorted, hop blocks sorted, no node twice, every edge's endpoints are local rows, e_id names the
    edge, an expanded node's in-edges are contiguous and in original order, hop-L nodes have no in-edges."""
    from hgin.data import CONV_RELATIONS
    g = _tiny_graph()
    seeds = {"path": [5, 1, 5, 30], "link": [2, 2, 9]}
    n_id, edges, e_id, n_seed = ref_sample(g, CONV_RELATIONS, [3, 2], seeds, 11, 4)
    assert n_seed == {"path": 3, "link": 2, "node": 0}
    assert list(n_id["path"][:3]) == [1, 5, 30] and list(n_id["link"][:2]) == [2, 9]
    for t in n_id:
        assert len(set(n_id[t].tolist())) == len(n_id[t])
    for r in CONV_RELATIONS:
        ei = g.edge_index[r].numpy()
        assert np.array_equal(n_id[r[0]][edges[r][0]], ei[0][e_id[r]])
        assert np.array_equal(n_id[r[2]][edges[r][1]], ei[1][e_id[r]])
        assert len(set(e_id[r].tolist())) == len(e_id[r])          # a node is expanded once per relation
        dst = edges[r][1]
        assert np.array_equal(dst, np.sort(dst, kind="stable"))     # hop-major + frontier order = local-row order
        for v in np.unique(dst):
            assert np.all(np.diff(e_id[r][dst == v]) > 0)           # original relative order inside a row
    # full fanout: every in-edge of every expanded node
    n_id, edges, e_id, n_seed = ref_sample(g, CONV_RELATIONS, [-1], {"link": [2]}, 0, 0)
    for r in CONV_RELATIONS:
        ei = g.edge_index[r].numpy()
        want = np.nonzero(ei[1] == 2)[0] if r[2] == "link" else np.zeros(0, dtype=np.int64)
        assert np.array_equal(e_id[r], want)


def test_uniformity_of_the_restatement():
    """d = 7, f = 3, offset = 0 .. 6999: every neighbour is picked 3000 times in expectation, sigma = sqrt(7000 * 3/7 *
    4/7) = 41.4; every count within 5 sigma = 207, and all 35 subsets occur.  With seed = 2024, v = 5, r_slot = 0 the
    restatement gives the counts [3040, 2926, 2997, 2969, 2952, 3051, 3065] (largest deviation 74) and subset
    frequencies between 164 and 232 (expected 200)."""
    counts = np.zeros(7, dtype=np.int64)
    subsets = {}
    for offset in range(7000):
        p = ref_picks_d(7, 5, 3, 2024, offset, 0)
        counts[p] += 1
        subsets[tuple(p)] = subsets.get(tuple(p), 0) + 1
    print(counts.tolist(), min(subsets.values()), max(subsets.values()))
    assert counts.sum() == 21000
    assert np.all(np.abs(counts - 3000) <= 207), counts
    assert set(subsets) == set(itertools.combinations(range(7), 3))


# ---------------------------------------------------------------------------------------------------
# surface
# ---------------------------------------------------------------------------------------------------
def test_python_surface():
    import hgin
    from hgin import linkpred, neighbor, train
    for name in ("NeighborSampler", "SampledSubgraph", "LinkBatch", "link_neighbor_batch", "link_minibatch_step"):
        assert name in hgin.__all__ and hasattr(hgin, name), name
    assert hgin.NeighborSampler is neighbor.NeighborSampler and hgin.link_neighbor_batch is linkpred.link_neighbor_batch
    sig = inspect.signature(train.link_train_step)
    assert list(sig.parameters) == ["model", "opt", "graph", "predictor", "step", "pos", "known"]
    sig = inspect.signature(neighbor.NeighborSampler.__init__)
    assert [(n, p.default) for n, p in sig.parameters.items()][2:] == [
        ("fanouts", inspect.Parameter.empty), ("relations", None), ("seed", 0)]
    sig = inspect.signature(neighbor.NeighborSampler.sample)
    assert [(n, p.default) for n, p in sig.parameters.items()][1:] == [("seeds", inspect.Parameter.empty), ("offset", 0)]
    sig = inspect.signature(linkpred.link_neighbor_batch)
    assert [(n, p.default) for n, p in sig.parameters.items()] == [
        ("sampler", inspect.Parameter.empty), ("relation", inspect.Parameter.empty), ("pos", inspect.Parameter.empty),
        ("neg_dst", None), ("offset", 0)]
    assert linkpred.LinkBatch._fields == ("sub", "pos", "neg_dst")
    sig = inspect.signature(linkpred.LinkPredictor.batch_loss)
    assert [(n, p.default) for n, p in sig.parameters.items()][1:] == [
        ("sampler", inspect.Parameter.empty), ("pos", inspect.Parameter.empty), ("step", 0), ("known", None)]
    sig = inspect.signature(train.link_minibatch_step)
    assert [(n, p.default) for n, p in sig.parameters.items()] == [
        ("model", inspect.Parameter.empty), ("opt", inspect.Parameter.empty), ("sampler", inspect.Parameter.empty),
        ("predictor", inspect.Parameter.empty), ("pos", inspect.Parameter.empty), ("step", 0), ("known", None)]
    fields = {f.name for f in neighbor.SampledSubgraph.__dataclass_fields__.values()}
    assert fields == {"graph", "n_id", "e_id", "n_seed"} and callable(neighbor.SampledSubgraph.local)


def test_abi_stays_16_and_the_header_section():
    from conftest import ROOT
    from hgin import _lib
    assert _lib.ABI_VERSION == 16
    assert _lib.lib().hgin_abi_version() == 16
    text = open(os.path.join(ROOT, "include", "hgin.h")).read()
    assert int(re.search(r"#define HGIN_ABI_VERSION (\d+)", text).group(1)) == 16
    a22 = text[text.index("---- A22"):]
    a22 = a22[:a22.index("---- F4")]
    assert text.index("---- A21") < text.index("---- A22")
    for name in NEW_SYMBOLS:
        assert name in _lib.exported_symbols() and hasattr(_lib.lib(), name), name
        assert re.search(r"\bint " + name + r"\(", a22), name
    for word in ("without a bump", "Floyd", "J = d - f + i", "(uint32)v, offset, 2, (uint32)(r_slot * 64 + (i >> 2))",
                 "hi32((uint64)w_i * (J + 1))", "ascending CSR position", "word 2 is", "hop-major",
                 "does not depend on execution order", "no workgroup waits on another"):
        assert word in a22, word


# ---------------------------------------------------------------------------------------------------
# validation: before any device is needed
# ---------------------------------------------------------------------------------------------------
def _graph():
    from hgin.data import CONFIGS, synthetic_graph
    return synthetic_graph(CONFIGS["cfg1"], seed=0)


def test_sampler_errors_on_cpu_tensors():
    import hgin
    from hgin.data import REL_PL, HeteroGraph
    from hgin.store import PaddedBatch
    g = _graph()
    for bad in ((10, 5), 10, None, "10"):
        with pytest.raises(TypeError):
            hgin.NeighborSampler(g, fanouts=bad)
    for bad in ([10.0], [True], ["3"]):
        with pytest.raises(TypeError):
            hgin.NeighborSampler(g, fanouts=bad)
    for bad in ([], [0], [129], [-2], [5, 0]):
        with pytest.raises(ValueError):
            hgin.NeighborSampler(g, fanouts=bad)
    with pytest.raises(ValueError, match="no relation"):
        hgin.NeighborSampler(g, fanouts=[2], relations=[("path", "likes", "link")])
    with pytest.raises(ValueError, match="twice"):
        hgin.NeighborSampler(g, fanouts=[2], relations=[REL_PL, REL_PL])
    with pytest.raises(TypeError):
        hgin.NeighborSampler(g, fanouts=[2], seed=0.5)
    with pytest.raises(ValueError, match="PaddedBatch"):
        hgin.NeighborSampler(object.__new__(PaddedBatch), fanouts=[2])
    bad = HeteroGraph(g.x, dict(g.edge_index), g.y, g.batch)
    bad.edge_index[REL_PL] = g.edge_index[REL_PL].to(torch.int32)
    with pytest.raises(TypeError):
        hgin.NeighborSampler(bad, fanouts=[2])
    s = hgin.NeighborSampler(g, fanouts=[10, 5])
    assert s.relations == list(g.edge_index.keys()) and s.fanouts == [10, 5] and s.seed == 0
    assert hgin.NeighborSampler(g, fanouts=[-1, 128], relations=[REL_PL], seed=-1).seed == 2**64 - 1


def test_seed_errors_on_cpu_tensors():
    import hgin
    s = hgin.NeighborSampler(_graph(), fanouts=[3, 2])
    ids = torch.tensor([0, 5, 5])
    with pytest.raises(TypeError):
        s.sample({"path": ids.to(torch.int32)})
    with pytest.raises(TypeError):
        s.sample({"path": ids.float()})
    with pytest.raises(TypeError):
        s.sample({"path": [0, 5]})
    with pytest.raises(TypeError):
        s.sample(ids)
    with pytest.raises(TypeError):
        s.sample({"path": ids}, offset=0.5)
    with pytest.raises(ValueError):
        s.sample({"path": ids}, offset=-1)
    with pytest.raises(ValueError):
        s.sample({"path": ids}, offset=2**32)
    with pytest.raises(ValueError, match="unknown node type"):
        s.sample({"host": ids})
    with pytest.raises(ValueError):
        s.sample({"path": ids.view(1, 3)})
    with pytest.raises(IndexError):
        s.sample({"path": torch.tensor([0, 600])})
    with pytest.raises(IndexError):
        s.sample({"path": ids, "link": torch.tensor([-1])})


def test_link_layer_errors_on_cpu_tensors():
    import hgin
    from hgin.data import CONFIGS, REL_PL
    g = _graph()
    cfg = CONFIGS["cfg1"]
    model = hgin.HetroGIN(**cfg.model_kwargs({"link": cfg.f_link, "path": cfg.f_path, "node": cfg.f_node}))
    s = hgin.NeighborSampler(g, fanouts=[3, 2])
    pos = g.edge_index[REL_PL][:, :8]
    with pytest.raises(ValueError, match="hard"):
        hgin.LinkPredictor(model, REL_PL, k=2, seed=0, hard=2).batch_loss(s, pos)
    with pytest.raises(ValueError, match="graph_local"):
        hgin.LinkPredictor(model, REL_PL, k=2, seed=0, graph_local=True).batch_loss(s, pos)
    pred = hgin.LinkPredictor(model, REL_PL, k=2, seed=0)
    with pytest.raises(TypeError):
        pred.batch_loss(g, pos)
    with pytest.raises(TypeError):
        pred.batch_loss(s, pos.to(torch.int32))
    with pytest.raises(ValueError):
        pred.batch_loss(s, pos[0])
    with pytest.raises(TypeError):
        hgin.link_neighbor_batch(s, REL_PL, pos.float())
    with pytest.raises(ValueError):
        hgin.link_neighbor_batch(s, REL_PL, pos, neg_dst=torch.zeros(7, 2, dtype=torch.int64))
    with pytest.raises(TypeError):
        hgin.link_neighbor_batch(s, REL_PL, pos, neg_dst=torch.zeros(8, 2))
    other = hgin.HetroGIN(**cfg.model_kwargs({"link": cfg.f_link, "path": cfg.f_path, "node": cfg.f_node}))
    with pytest.raises(ValueError, match="another model"):
        hgin.link_minibatch_step(other, None, s, pred, pos)


def test_valid_arguments_on_cpu_tensors_name_the_missing_device():
    import hgin
    from hgin.data import CONFIGS, REL_PL
    g = _graph()
    cfg = CONFIGS["cfg1"]
    s = hgin.NeighborSampler(g, fanouts=[3, 2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.sample({"path": torch.tensor([0, 5, 5]), "link": torch.tensor([7])}, offset=3)
    pos = g.edge_index[REL_PL][:, :8]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hgin.link_neighbor_batch(s, REL_PL, pos, neg_dst=torch.zeros(8, 2, dtype=torch.int64))
    model = hgin.HetroGIN(**cfg.model_kwargs({"link": cfg.f_link, "path": cfg.f_path, "node": cfg.f_node}))
    pred = hgin.LinkPredictor(model, REL_PL, k=2, seed=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pred.batch_loss(s, pos)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hgin.LinkPredictor(model, REL_PL, k=2, seed=0, filter_negatives=True).batch_loss(s, pos, step=2)


# ---------------------------------------------------------------------------------------------------
# C argument checks: HGIN_E_ARG / HGIN_E_WORKSPACE before any launch
# ---------------------------------------------------------------------------------------------------
_Q = ctypes.c_void_p(256)


def test_c_argument_errors_do_not_touch_the_device():
    from hgin import _lib
    lib = _lib.lib()
    err = lib.hgin_last_error

    size = ctypes.c_size_t(0)
    assert lib.hgin_neighbor_sample_workspace_size(10, None) == -1
    assert lib.hgin_neighbor_sample_workspace_size(-1, ctypes.byref(size)) == -1
    assert lib.hgin_neighbor_sample_workspace_size(1 << 31, ctypes.byref(size)) == -1
    assert lib.hgin_neighbor_sample_workspace_size(0, ctypes.byref(size)) == 0 and size.value == 256
    assert lib.hgin_neighbor_sample_workspace_size(256 * 40 + 1, ctypes.byref(size)) == 0
    assert size.value == 512 and size.value >= 8 * (41 + 1)

    def offsets(rowptr=_Q, n_rows=10, fr=_Q, n=4, f=5, off=_Q, ws=_Q, ws_bytes=1 << 20):
        return lib.hgin_neighbor_sample_offsets(rowptr, n_rows, fr, n, f, off, ws, ws_bytes, None)

    assert offsets(n_rows=-1) == -1 and b"n_rows = -1" in err()
    assert offsets(n_rows=1 << 31) == -1 and b"n_rows" in err()
    assert offsets(n=-1) == -1 and b"n_frontier = -1" in err()
    for f in (0, -2, 129):
        assert offsets(f=f) == -1 and b"f = " in err()
    assert offsets(off=None) == -1 and b"off NULL" in err()
    assert offsets(rowptr=None) == -1 and b"rowptr NULL" in err()
    assert offsets(fr=None) == -1 and b"frontier NULL" in err()
    assert offsets(ws=None) == -3 and b"workspace" in err()
    assert offsets(ws_bytes=8) == -3 and b"workspace" in err()

    def sample(rowptr=_Q, col=_Q, perm=_Q, n_rows=10, fr=_Q, n=4, f=5, slot=0, off=_Q, src=_Q, eid=_Q, n_out=8):
        return lib.hgin_neighbor_sample(rowptr, col, perm, n_rows, fr, n, f, 0, 0, slot, off, src, eid, n_out, None)

    assert sample(n_rows=-1) == -1 and b"n_rows = -1" in err()
    assert sample(n=-1) == -1 and b"n_frontier = -1" in err()
    for f in (0, -2, 129):
        assert sample(f=f) == -1 and b"f = " in err()
    assert sample(slot=-1) == -1 and b"r_slot = -1" in err()
    assert sample(slot=1 << 26) == -1 and b"r_slot" in err()
    assert sample(n_out=-1) == -1 and b"n_out = -1" in err()
    assert sample(n_out=21) == -1 and b"n_out = 21" in err()        # above n_frontier * f
    for name in ("rowptr", "col", "perm", "off"):
        assert sample(**{name: None}) == -1 and (name + " NULL").encode() in err()
    assert sample(fr=None) == -1 and b"frontier NULL" in err()
    assert sample(src=None) == -1 and b"out_src NULL" in err()
    assert sample(eid=None) == -1 and b"out_eid NULL" in err()
    assert sample(n=0, n_out=0, rowptr=None, col=None, perm=None, fr=None, off=None, src=None, eid=None) == 0
    assert sample(n_out=0, rowptr=None, col=None, perm=None, fr=None, off=None, src=None, eid=None) == 0

    assert lib.hgin_neighbor_fresh(_Q, -1, _Q, 4, 0, _Q, None) == -1 and b"n_nodes = -1" in err()
    assert lib.hgin_neighbor_fresh(_Q, 10, _Q, -1, 0, _Q, None) == -1 and b"n = -1" in err()
    assert lib.hgin_neighbor_fresh(None, 10, _Q, 4, 0, _Q, None) == -1 and b"map NULL" in err()
    assert lib.hgin_neighbor_fresh(_Q, 10, None, 4, 0, _Q, None) == -1 and b"src NULL" in err()
    assert lib.hgin_neighbor_fresh(_Q, 10, _Q, 4, 0, None, None) == -1 and b"out NULL" in err()
    assert lib.hgin_neighbor_fresh(None, 10, None, 0, 0, None, None) == 0

    assert lib.hgin_neighbor_map_set(_Q, 1 << 31, _Q, 4, 0, None) == -1 and b"n_nodes" in err()
    assert lib.hgin_neighbor_map_set(_Q, 10, _Q, -1, 0, None) == -1 and b"n = -1" in err()
    assert lib.hgin_neighbor_map_set(_Q, 10, _Q, 4, (1 << 31) - 2, None) == -1 and b"base + n" in err()
    assert lib.hgin_neighbor_map_set(None, 10, _Q, 4, 0, None) == -1 and b"map NULL" in err()
    assert lib.hgin_neighbor_map_set(_Q, 10, None, 4, -1, None) == -1 and b"ids NULL" in err()
    assert lib.hgin_neighbor_map_set(None, 10, None, 0, 0, None) == 0

    def emit(m=_Q, n_src=10, src=_Q, off=_Q, n=4, base=0, n_edges=8, out=_Q):
        return lib.hgin_neighbor_emit(m, n_src, src, off, n, base, n_edges, out, None)

    assert emit(n_src=-1) == -1 and b"n_src_nodes = -1" in err()
    assert emit(n=-1) == -1 and b"n_frontier = -1" in err()
    assert emit(n_edges=-1) == -1 and b"n_edges = -1" in err()
    assert emit(base=-1) == -1 and b"dst_base = -1" in err()
    assert emit(n=0) == -1 and b"empty frontier" in err()
    assert emit(m=None) == -1 and b"map_src NULL" in err()
    assert emit(src=None) == -1 and b"src NULL" in err()
    assert emit(off=None) == -1 and b"off NULL" in err()
    assert emit(out=None) == -1 and b"out_edge NULL" in err()
    assert emit(n_edges=0, m=None, src=None, off=None, out=None) == 0
