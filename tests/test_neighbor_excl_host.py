"""Neighbour sampling with an excluded set (include/hgin.h A25), host side: the numpy restatement of the rule on top of
A22's (``ref_picks_excl`` / ``ref_sample_excl``, which tests/test_gpu_neighbor_excl.py pins the kernels to bit for bit),
its properties and uniformity, the Python surface and every argument check, all without a device."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from test_neighbor_host import ref_csr, ref_picks, ref_picks_d, ref_sample

NEW_SYMBOLS = ("hgin_neighbor_sample_offsets_excl", "hgin_neighbor_sample_excl")


def ref_picks_excl(rowptr, col, v, f, seed, offset, slot, excl_set):
    """The ascending CSR positions picked for frontier node ``v`` when the positions whose (source, v) pair is in
    ``excl_set`` (a set of (src, dst) tuples) are excluded: A22's picks over the ranks of the free positions."""
    r0, d = int(rowptr[v]), int(rowptr[v + 1]) - int(rowptr[v])
    free = [p for p in range(d) if (int(col[r0 + p]), int(v)) not in excl_set]
    return [free[t] for t in ref_picks_d(len(free), v, f, seed, offset, slot)]


def ref_sample_excl(graph, relations, fanouts, seeds, seed, offset, exclude):
    """``ref_sample`` with ``exclude`` = {relation: set of (src, dst)} applied at every hop (include/hgin.h A25)."""
    types = list(graph.x.keys())
    relations = [tuple(r) for r in relations]
    csr = {r: ref_csr(graph.edge_index[r], int(graph.x[r[2]].shape[0])) for r in relations}
    rows = {t: sorted(set(int(i) for i in np.asarray(seeds.get(t, ())).reshape(-1))) for t in types}
    local = {t: {g: i for i, g in enumerate(rows[t])} for t in types}
    n_seed = {t: len(rows[t]) for t in types}
    frontier = {t: list(rows[t]) for t in types}
    out = {r: ([], [], []) for r in relations}
    for f in fanouts:
        reached = {t: set() for t in types}
        for slot, r in enumerate(relations):
            rowptr, col, perm = csr[r]
            for v in frontier[r[2]]:
                for p in ref_picks_excl(rowptr, col, v, f, seed, offset, slot, exclude.get(r, ())):
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


def pair_set(pairs):
    """{(src, dst)} of an int64 [2, M] tensor or array."""
    a = np.asarray(pairs.cpu().numpy() if isinstance(pairs, torch.Tensor) else pairs, dtype=np.int64)
    return set(zip(a[0].tolist(), a[1].tolist()))


# ---------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------
def _row(d, n_src=1000, seed=0, rows=3, v=1):
    """A CSR of ``rows`` rows of d distinct sources each; (rowptr, col)."""
    rng = np.random.default_rng(seed)
    col = np.concatenate([rng.permutation(n_src)[:d] for _ in range(rows)])
    return np.arange(rows + 1, dtype=np.int64) * d, col


def test_an_empty_exclusion_is_a22():
    rowptr, col = _row(40)
    for f in (1, 5, 39, 40, 41, -1):
        for v in range(3):
            assert ref_picks_excl(rowptr, col, v, f, 9, 3, 1, set()) == ref_picks(rowptr, v, f, 9, 3, 1)
    from hgin.data import CONFIGS, CONV_RELATIONS, scaled_config, synthetic_graph
    g = synthetic_graph(scaled_config(CONFIGS["cfg1"], 0.1), seed=3)
    seeds = {"path": [5, 1, 5, 30], "link": [2, 2, 9]}
    a = ref_sample(g, CONV_RELATIONS, [3, 2], seeds, 11, 4)
    b = ref_sample_excl(g, CONV_RELATIONS, [3, 2], seeds, 11, 4, {})
    for x, y in zip(a[:3], b[:3]):
        assert set(x) == set(y) and all(np.array_equal(x[k], y[k]) for k in x)
    assert a[3] == b[3]


def test_no_excluded_position_is_picked_and_the_rest_is_a22_over_the_free_ranks():
    rowptr, col = _row(40)
    v, r0 = 1, 40
    gone = {7, 8, 20, 39}
    excl = {(int(col[r0 + p]), v) for p in gone}
    free = [p for p in range(40) if p not in gone]
    for f in (1, 5, 35, 36, 37, -1):
        for offset in range(20):
            got = ref_picks_excl(rowptr, col, v, f, 4, offset, 2, excl)
            assert not set(got) & gone and got == sorted(set(got))
            assert len(got) == (36 if f == -1 else min(36, f))
            assert got == [free[t] for t in ref_picks_d(36, v, f, 4, offset, 2)]


def test_every_copy_of_a_repeated_pair_goes():
    rowptr = np.array([0, 6], dtype=np.int64)
    col = np.array([4, 9, 4, 2, 4, 7])
    assert ref_picks_excl(rowptr, col, 0, -1, 0, 0, 0, {(4, 0)}) == [1, 3, 5]
    for offset in range(30):
        got = ref_picks_excl(rowptr, col, 0, 2, 0, offset, 0, {(4, 0)})
        assert len(got) == 2 and set(got) <= {1, 3, 5}


def test_d_free_at_most_f_switches_the_row_from_floyd_to_copy():
    rowptr, col = _row(9, rows=1)
    f = 5
    assert len(ref_picks_excl(rowptr, col, 0, f, 1, 0, 0, set())) == 5                 # d = 9 > f: Floyd
    four = {(int(col[p]), 0) for p in (0, 3, 4, 8)}                                    # d' = 5 = f: copy
    assert ref_picks_excl(rowptr, col, 0, f, 1, 0, 0, four) == [1, 2, 5, 6, 7]
    three = {(int(col[p]), 0) for p in (0, 3, 8)}                                      # d' = 6 = f + 1: Floyd again
    seen = {tuple(ref_picks_excl(rowptr, col, 0, f, 1, o, 0, three)) for o in range(40)}
    assert len(seen) > 1 and all(len(s) == 5 and set(s) <= {1, 2, 4, 5, 6, 7} for s in seen)
    everything = {(int(c), 0) for c in col}                                            # d' = 0
    for ff in (1, 5, -1):
        assert ref_picks_excl(rowptr, col, 0, ff, 1, 0, 0, everything) == []


def test_picks_do_not_depend_on_keys_of_other_rows_or_of_non_edges():
    rowptr, col = _row(40)
    v = 1
    own = {(int(col[40 + 3]), v), (int(col[40 + 17]), v)}
    others = {(int(col[2]), 0), (int(col[85]), 2), (int(col[40 + 3]), 0), (int(col[40 + 3]), 2), (5, 77)}
    absent = next(u for u in range(1000) if u not in set(col[40:80].tolist()))
    for f in (5, -1):
        for offset in range(10):
            base = ref_picks_excl(rowptr, col, v, f, 2, offset, 0, own)
            assert base == ref_picks_excl(rowptr, col, v, f, 2, offset, 0, own | others | {(absent, v)})
    assert ref_picks_excl(rowptr, col, v, 5, 2, 0, 0, others) == ref_picks(rowptr, v, 5, 2, 0, 0)


def test_uniformity_over_the_free_positions():
    """d = 40, 10 positions excluded, f = 5, offsets 0 .. 3999: a free position is picked with probability f / d' =
    1 / 6, so 666.7 times in expectation with sigma = sqrt(4000 * 1/6 * 5/6) = 23.6; every free count lies within
    5 sigma = 117.9 of it and every excluded count is 0."""
    rowptr, col = _row(40, rows=1, seed=5)
    gone = [0, 3, 4, 11, 19, 20, 21, 30, 38, 39]
    excl = {(int(col[p]), 0) for p in gone}
    N, f, dp = 4000, 5, 30
    counts = np.zeros(40, dtype=np.int64)
    for offset in range(N):
        counts[ref_picks_excl(rowptr, col, 0, f, 2025, offset, 0, excl)] += 1
    q = f / dp
    sigma = math.sqrt(N * q * (1 - q))
    free = np.setdiff1d(np.arange(40), gone)
    print(counts.tolist(), "largest deviation", float(np.abs(counts[free] - N * q).max()), "5 sigma", 5 * sigma)
    assert counts.sum() == N * f
    assert np.all(counts[gone] == 0)
    assert np.all(np.abs(counts[free] - N * q) <= 5 * sigma), counts


# ---------------------------------------------------------------------------------------------------
# surface
# ---------------------------------------------------------------------------------------------------
def test_python_surface():
    import hgin
    from hgin import linkpred, neighbor
    assert "link_neighbor_batch_excl" in hgin.__all__
    assert hgin.link_neighbor_batch_excl is linkpred.link_neighbor_batch_excl
    sig = inspect.signature(linkpred.link_neighbor_batch_excl)
    assert [(n, p.default) for n, p in sig.parameters.items()] == [
        ("sampler", inspect.Parameter.empty), ("relation", inspect.Parameter.empty), ("pos", inspect.Parameter.empty),
        ("neg_dst", None), ("offset", 0), ("rev_relation", "auto")]
    sig = inspect.signature(neighbor.NeighborSampler.sample_excluding)
    assert [(n, p.default) for n, p in sig.parameters.items()][1:] == [
        ("seeds", inspect.Parameter.empty), ("exclude", inspect.Parameter.empty), ("offset", 0)]
    init = inspect.signature(linkpred.LinkPredictor.__init__).parameters
    assert init["exclude_targets"].default is False and init["rev_relation"].default == "auto"
    assert list(init)[-2:] == ["exclude_targets", "rev_relation"]


def test_abi_stays_16_and_the_header_section():
    from conftest import ROOT
    from hgin import _lib
    assert _lib.ABI_VERSION == 16
    assert _lib.lib().hgin_abi_version() == 16
    text = open(os.path.join(ROOT, "include", "hgin.h")).read()
    assert int(re.search(r"#define HGIN_ABI_VERSION (\d+)", text).group(1)) == 16
    assert text.index("---- A24") < text.index("---- A25") < text.index("---- F4 widening")
    a25 = text[text.index("---- A25"):]
    a25 = a25[:a25.index("---- F4")]
    for name in NEW_SYMBOLS:
        assert name in _lib._SIGS, name
        assert name in _lib.exported_symbols() and hasattr(_lib.lib(), name), name
        assert re.search(r"\bint " + name + r"\(", a25), name
    for word in ("without a bump", "v * 2^32 + u", "ascending, repeats allowed", "every copy of a multi-edge goes",
                 "J = d' - f + i", "CSR position q_t", "bit for bit", "no workgroup waits on another", "no atomics",
                 "wave-uniform"):
        assert word in a25, word


# ---------------------------------------------------------------------------------------------------
# validation: before any device is needed
# ---------------------------------------------------------------------------------------------------
def _graph():
    from hgin.data import CONFIGS, synthetic_graph
    return synthetic_graph(CONFIGS["cfg1"], seed=0)


def test_exclude_errors_on_cpu_tensors():
    import hgin
    from hgin.data import REL_LN, REL_LP, REL_PL
    g = _graph()
    s = hgin.NeighborSampler(g, fanouts=[3, 2])
    seeds = {"path": torch.tensor([0, 5, 5]), "link": torch.tensor([7])}
    pairs = g.edge_index[REL_PL][:, :6]
    for bad in (None, [pairs], pairs, ((REL_PL, pairs),)):
        with pytest.raises(TypeError, match="exclude must be a dict"):
            s.sample_excluding(seeds, bad)
    with pytest.raises(ValueError, match="not a relation"):
        s.sample_excluding(seeds, {("path", "likes", "link"): pairs})
    assert REL_LN in g.edge_index
    with pytest.raises(ValueError, match="not a relation"):     # a relation of the graph the sampler does not use
        hgin.NeighborSampler(g, fanouts=[3], relations=[REL_PL, REL_LP]).sample_excluding(seeds, {REL_LN: pairs})
    with pytest.raises(ValueError, match="not a relation"):
        s.sample_excluding(seeds, {"uses": pairs})
    for bad in (pairs.to(torch.int32), pairs.float(), pairs.tolist(), None):
        with pytest.raises(TypeError, match="int64"):
            s.sample_excluding(seeds, {REL_PL: bad})
    for bad in (pairs[0], pairs.t().contiguous(), pairs.reshape(2, 3, 2), torch.zeros(3, 0, dtype=torch.int64)):
        with pytest.raises(ValueError, match=r"\[2, M\]"):
            s.sample_excluding(seeds, {REL_PL: bad})
    n_path, n_link = g.x["path"].size(0), g.x["link"].size(0)
    for bad in ([[0, n_path], [1, 2]], [[0, 1], [n_link, 2]], [[-1, 1], [0, 2]], [[0, 1], [0, -2]]):
        with pytest.raises(IndexError, match="excluded"):
            s.sample_excluding(seeds, {REL_PL: torch.tensor(bad)})
    with pytest.raises(IndexError, match="excluded"):           # REL_LP's own orientation: (link, path)
        s.sample_excluding(seeds, {REL_LP: torch.tensor([[n_link], [0]])})
    # the seed checks are sample's
    with pytest.raises(TypeError):
        s.sample_excluding({"path": [0, 5]}, {REL_PL: pairs})
    with pytest.raises(ValueError):
        s.sample_excluding(seeds, {REL_PL: pairs}, offset=-1)
    with pytest.raises(IndexError, match="seed"):
        s.sample_excluding({"path": torch.tensor([0, 600])}, {REL_PL: pairs})
    for m in s._maps.values():
        assert bool((m == -1).all())


def test_valid_arguments_on_cpu_tensors_name_the_missing_device():
    import hgin
    from hgin.data import CONFIGS, REL_LP, REL_PL
    g = _graph()
    cfg = CONFIGS["cfg1"]
    s = hgin.NeighborSampler(g, fanouts=[3, 2])
    seeds = {"path": torch.tensor([0, 5, 5]), "link": torch.tensor([7])}
    pos = g.edge_index[REL_PL][:, :8]
    for exclude in ({}, {REL_PL: pos[:, :0]}, {REL_PL: pos, REL_LP: pos.flip(0)}):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            s.sample_excluding(seeds, exclude, offset=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hgin.link_neighbor_batch_excl(s, REL_PL, pos, neg_dst=torch.zeros(8, 2, dtype=torch.int64))
    model = hgin.HetroGIN(**cfg.model_kwargs({"link": cfg.f_link, "path": cfg.f_path, "node": cfg.f_node}))
    pred = hgin.LinkPredictor(model, REL_PL, k=2, seed=0, exclude_targets=True)
    assert pred.exclude_targets is True and pred.rev_relation == "auto"
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pred.batch_loss(s, pos)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pred.batch_full_loss(s, pos)


def test_link_batch_excl_errors_on_cpu_tensors():
    import hgin
    from hgin.data import REL_PL
    g = _graph()
    s = hgin.NeighborSampler(g, fanouts=[3, 2])
    pos = g.edge_index[REL_PL][:, :8]
    with pytest.raises(TypeError, match="NeighborSampler"):
        hgin.link_neighbor_batch_excl(g, REL_PL, pos)
    with pytest.raises(TypeError):
        hgin.link_neighbor_batch_excl(s, REL_PL, pos.float())
    with pytest.raises(ValueError):
        hgin.link_neighbor_batch_excl(s, REL_PL, pos[0])
    with pytest.raises(ValueError):
        hgin.link_neighbor_batch_excl(s, ("path", "link"), pos)
    with pytest.raises(ValueError):
        hgin.link_neighbor_batch_excl(s, REL_PL, pos, neg_dst=torch.zeros(7, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match="rev_relation"):
        hgin.link_neighbor_batch_excl(s, REL_PL, pos, rev_relation="reverse")
    with pytest.raises(ValueError, match="no relation"):
        hgin.link_neighbor_batch_excl(s, REL_PL, pos, rev_relation=("link", "likes", "path"))
    with pytest.raises(ValueError, match="does not run"):
        hgin.link_neighbor_batch_excl(s, REL_PL, pos, rev_relation=REL_PL)


class _Seen(Exception):
    pass


def _stub_sampler(edge_index, relations=None):
    """A NeighborSampler over a stub graph whose ``sample_excluding`` only reports the exclusion it was handed."""
    import hgin
    from hgin.data import HeteroGraph
    x = {"path": torch.zeros(20, 1), "link": torch.zeros(10, 1)}
    s = hgin.NeighborSampler(HeteroGraph(x, edge_index, torch.zeros(20), {}), fanouts=[2], relations=relations)

    def seen(seeds, exclude, offset=0):
        raise _Seen({r: e.clone() for r, e in exclude.items()})

    s.sample_excluding = seen
    return s


def test_rev_relation_resolution_on_a_stub_graph():
    import hgin
    pl, lp, lp2 = ("path", "uses", "link"), ("link", "includes", "path"), ("link", "serves", "path")
    e = torch.tensor([[0, 3, 3], [1, 1, 9]])
    pos = torch.tensor([[3, 0], [9, 1]])

    def excluded(sampler, **kw):
        with pytest.raises(_Seen) as info:
            hgin.link_neighbor_batch_excl(sampler, pl, pos, **kw)
        return info.value.args[0]

    both = _stub_sampler({pl: e, lp: e.flip(0)})
    got = excluded(both)
    assert list(got) == [pl, lp] and torch.equal(got[pl], pos) and torch.equal(got[lp], pos.flip(0))
    assert list(excluded(both, rev_relation=None)) == [pl]
    assert list(excluded(both, rev_relation=lp)) == [pl, lp]
    assert list(excluded(_stub_sampler({pl: e}))) == [pl]                             # no reverse relation: none
    # only the relations the sampler convolves over
    assert list(excluded(_stub_sampler({pl: e, lp: e.flip(0)}, relations=[lp]))) == [lp]
    assert list(excluded(_stub_sampler({pl: e, lp: e.flip(0)}, relations=[pl]))) == [pl]
    several = _stub_sampler({pl: e, lp: e.flip(0), lp2: e.flip(0)})
    with pytest.raises(ValueError, match="several relations"):
        hgin.link_neighbor_batch_excl(several, pl, pos)
    assert list(excluded(several, rev_relation=lp2)) == [pl, lp2]
    assert list(excluded(several, rev_relation=None)) == [pl]


def test_the_predictor_hands_its_rev_relation_on(monkeypatch):
    import hgin
    from hgin import ops
    monkeypatch.setattr(ops, "require_device", lambda *a, **k: None)     # the stub sampler launches nothing

    class _Model:
        def encode(self, x, e):
            raise AssertionError("not reached")

    pl, lp, lp2 = ("path", "uses", "link"), ("link", "includes", "path"), ("link", "serves", "path")
    e = torch.tensor([[0, 3, 3], [1, 1, 9]])
    pos = torch.tensor([[3, 0], [9, 1]])
    s = _stub_sampler({pl: e, lp: e.flip(0), lp2: e.flip(0)})
    for rev, want in ((lp2, [pl, lp2]), (None, [pl])):
        pred = hgin.LinkPredictor(_Model(), pl, k=2, seed=0, exclude_targets=True, rev_relation=rev)
        with pytest.raises(_Seen) as info:
            pred.batch_full_loss(s, pos)
        assert list(info.value.args[0]) == want
    with pytest.raises(ValueError, match="several relations"):
        hgin.LinkPredictor(_Model(), pl, k=2, seed=0, exclude_targets=True).batch_full_loss(s, pos)


# ---------------------------------------------------------------------------------------------------
# C argument checks: HGIN_E_ARG / HGIN_E_WORKSPACE before any launch
# ---------------------------------------------------------------------------------------------------
_Q = ctypes.c_void_p(256)


def test_c_argument_errors_do_not_touch_the_device():
    from hgin import _lib
    lib = _lib.lib()
    err = lib.hgin_last_error

    def offsets(rowptr=_Q, col=_Q, n_rows=10, fr=_Q, n=4, f=5, excl=_Q, n_excl=3, off=_Q, ws=_Q, ws_bytes=1 << 20):
        return lib.hgin_neighbor_sample_offsets_excl(rowptr, col, n_rows, fr, n, f, excl, n_excl, off, ws, ws_bytes,
                                                     None)

    assert offsets(n_rows=-1) == -1 and b"n_rows = -1" in err()
    assert offsets(n_rows=1 << 31) == -1 and b"n_rows" in err()
    assert offsets(n=-1) == -1 and b"n_frontier = -1" in err()
    for f in (0, -2, 129):
        assert offsets(f=f) == -1 and b"f = " in err()
    assert offsets(excl=None) == -1 and b"excl NULL" in err()
    assert offsets(n_excl=-1) == -1 and b"n_excl = -1" in err()
    assert offsets(n_excl=1 << 31) == -1 and b"n_excl" in err()
    assert offsets(off=None) == -1 and b"off NULL" in err()
    assert offsets(rowptr=None) == -1 and b"rowptr NULL" in err()
    assert offsets(fr=None) == -1 and b"frontier NULL" in err()
    assert offsets(ws=None) == -3 and b"workspace" in err()
    assert offsets(ws_bytes=8) == -3 and b"workspace" in err()

    def sample(rowptr=_Q, col=_Q, perm=_Q, n_rows=10, fr=_Q, n=4, f=5, slot=0, excl=_Q, n_excl=3, off=_Q, src=_Q,
               eid=_Q, n_out=8):
        return lib.hgin_neighbor_sample_excl(rowptr, col, perm, n_rows, fr, n, f, 0, 0, slot, excl, n_excl, off, src,
                                             eid, n_out, None)

    assert sample(n_rows=-1) == -1 and b"n_rows = -1" in err()
    assert sample(n=-1) == -1 and b"n_frontier = -1" in err()
    for f in (0, -2, 129):
        assert sample(f=f) == -1 and b"f = " in err()
    assert sample(slot=-1) == -1 and b"r_slot = -1" in err()
    assert sample(slot=1 << 26) == -1 and b"r_slot" in err()
    assert sample(excl=None) == -1 and b"excl NULL" in err()
    assert sample(n_excl=-1) == -1 and b"n_excl = -1" in err()
    assert sample(n_excl=1 << 31) == -1 and b"n_excl" in err()
    assert sample(n_out=-1) == -1 and b"n_out = -1" in err()
    assert sample(n_out=21) == -1 and b"n_out = 21" in err()        # above n_frontier * f
    for name in ("rowptr", "col", "perm", "off"):
        assert sample(**{name: None}) == -1 and (name + " NULL").encode() in err()
    assert sample(fr=None) == -1 and b"frontier NULL" in err()
    assert sample(src=None) == -1 and b"out_src NULL" in err()
    assert sample(eid=None) == -1 and b"out_eid NULL" in err()
    none = dict(rowptr=None, col=None, perm=None, fr=None, off=None, src=None, eid=None)
    assert sample(n=0, n_out=0, excl=None, n_excl=0, **none) == 0
    assert sample(n_out=0, excl=None, n_excl=0, **none) == 0
