"""Leakage-free edge splits on the GPU (include/hgin.h A21; ``hgin.link_split*``).

Parts: bit for bit tests/test_linksplit_host.py's numpy restatement (Philox words from the C oracle), counts equal to
its histogram.  Selection: exactly ``edge_index[:, mask]`` and ``nonzero(mask)`` (a stable compaction) at the tile edges,
past one scan pass, on a non-contiguous edge index, and repeatably.  ``link_split``: on graphs whose ``randint``
endpoints repeat pairs, no held-out pair is left in a graph that is encoded to score it — in either direction — which a
split by edge position fails on the very same input; the encoder's output on ``train_graph`` equals, bit for bit, its
output on a graph cut with host boolean masks of the restatement.  End to end: training on ``train_graph`` /
``train_pos`` and filtered ranking of ``val_pos`` on ``val_graph``.  Sizes come from ``hgin_link_split_geometry``."""
import copy
import functools
import math

import numpy as np
import pytest
import torch

from test_linksplit_host import ref_bounds, ref_parts

DEV = "cuda"
pytestmark = pytest.mark.gpu

SEEDS = (0, 2**40 + 3)
FRACTIONS = ((0.1, 0.2, 0.0), (0.1, 0.2, 0.3), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))   # val, test, disjoint
KEEPS = ((), (0,), (0, 1), (0, 1, 2), (2,), (3,), (0, 1, 2, 3))


@functools.lru_cache(maxsize=None)
def _geometry():
    from hgin import linksplit
    return linksplit.split_geometry()


def _sizes(which):
    T, _ = _geometry()
    small = (1, 63, 64, 65, 255, 256, 257)
    tiles = (T - 1, T, T + 1, 3 * T + 5)
    return small + tiles if which == "parts" else tiles


@functools.lru_cache(maxsize=None)
def _master():
    """int64 [2, 3 T + 5] on the host, endpoints drawn with replacement (pairs repeat); the cases take prefixes."""
    T, _ = _geometry()
    g = torch.Generator().manual_seed(4321)
    n = 3 * T + 5
    return torch.stack([torch.randint(0, 700, (n,), generator=g), torch.randint(0, 90, (n,), generator=g)])


@functools.lru_cache(maxsize=None)
def _master_ref(seed, swap, fr):
    return ref_parts(_master(), seed, ref_bounds(*fr), swap)


# ---------------------------------------------------------------------------------------------------
# parts
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i_size", range(11))
def test_parts_are_the_restatement_bit_for_bit(i_size):
    import hgin
    E = _sizes("parts")[i_size]
    ei = _master()[:, :E].contiguous().to(DEV)
    for seed in SEEDS:
        for swap in (False, True):
            for fr in FRACTIONS:
                part, counts = hgin.link_split_parts(ei, seed, fr[0], fr[1], fr[2], swap=swap)
                want = _master_ref(seed, swap, fr)[:E]
                assert part.dtype == torch.uint8 and tuple(part.shape) == (E,)
                assert counts.dtype == torch.int64 and counts.is_cuda and tuple(counts.shape) == (4,)
                assert np.array_equal(part.cpu().numpy(), want), (E, seed, swap, fr)
                assert counts.cpu().tolist() == np.bincount(want, minlength=4).tolist(), (E, seed, swap, fr)


def test_parts_of_the_flipped_relation_and_of_an_empty_one():
    import hgin
    T, _ = _geometry()
    ei = _master()[:, :T + 1].contiguous().to(DEV)
    fwd, c_fwd = hgin.link_split_parts(ei, 9, 0.1, 0.2, 0.3)
    rev, c_rev = hgin.link_split_parts(ei.flip(0).contiguous(), 9, 0.1, 0.2, 0.3, swap=True)
    assert torch.equal(fwd, rev) and torch.equal(c_fwd, c_rev)
    assert set(fwd.cpu().tolist()) == {0, 1, 2, 3}
    part, counts = hgin.link_split_parts(torch.empty(2, 0, dtype=torch.int64, device=DEV), 9, 0.1, 0.2)
    assert part.numel() == 0 and counts.cpu().tolist() == [0, 0, 0, 0]
    out, eid = hgin.link_split_select(torch.empty(2, 0, dtype=torch.int64, device=DEV), part, (0, 1))
    assert tuple(out.shape) == (2, 0) and tuple(eid.shape) == (0,)


# ---------------------------------------------------------------------------------------------------
# selection
# ---------------------------------------------------------------------------------------------------
def _codes(E, seed=77):
    g = torch.Generator().manual_seed(seed + E)
    return torch.randint(0, 4, (E,), generator=g).to(torch.uint8)


def _check_select(ei, part, keep):
    import hgin
    out, eid = hgin.link_split_select(ei, part, keep)
    mask = torch.zeros_like(part, dtype=torch.bool)
    for p in keep:
        mask |= part == p
    assert out.dtype == torch.int64 and eid.dtype == torch.int64 and out.is_contiguous()
    assert torch.equal(out, ei[:, mask]), keep
    assert torch.equal(eid, mask.nonzero().flatten()), keep
    return out, eid


@pytest.mark.parametrize("i_size", range(4))
def test_selection_is_a_stable_compaction(i_size):
    T, _ = _geometry()
    E = _sizes("select")[i_size]
    ei = _master()[:, :E].contiguous().to(DEV)
    part = _codes(E)
    if E > 2 * T:
        part[T:2 * T] = 3          # a whole tile that most selections skip
    part = part.to(DEV)
    for keep in KEEPS:
        out, eid = _check_select(ei, part, keep)
        again = _check_select(ei, part, keep)                     # a second run repeats the first
        assert torch.equal(out, again[0]) and torch.equal(eid, again[1])
    # the parts the kernel wrote (their counts ride along on the tensor) select like the codes above
    import hgin
    kpart, counts = hgin.link_split_parts(ei, 5, 0.1, 0.2, 0.3)
    sizes = [int(_check_select(ei, kpart, (p,))[1].numel()) for p in range(4)]
    assert sizes == counts.cpu().tolist() and sum(sizes) == E


def test_selection_past_one_scan_pass():
    T, W = _geometry()
    E = W * T + 1
    assert E <= 8 * 1024 * 1024 + 1
    g = torch.Generator(device=DEV).manual_seed(3)
    ei = torch.randint(0, 2**40, (2, E), generator=g, device=DEV, dtype=torch.int64)
    part = torch.randint(0, 4, (E,), generator=g, device=DEV, dtype=torch.int32).to(torch.uint8)
    part[-1] = 1                   # the one edge of the second pass is kept
    out, eid = _check_select(ei, part, (0, 1))
    assert int(eid[-1]) == E - 1 and W * T // 3 < int(eid.numel()) < 2 * W * T // 3


def test_selection_of_a_column_sliced_view():
    import hgin
    T, _ = _geometry()
    E = T + 1
    wide = _master()[:, :E + 7].contiguous().to(DEV)
    view = wide[:, 3:3 + E]
    assert not view.is_contiguous()
    part = _codes(E).to(DEV)
    for keep in ((0,), (1, 3)):
        a = hgin.link_split_select(view, part, keep)
        b = hgin.link_split_select(view.contiguous(), part, keep)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        _check_select(view, part, keep)
    pa, ca = hgin.link_split_parts(view, 3, 0.2, 0.2)
    pb, cb = hgin.link_split_parts(view.contiguous(), 3, 0.2, 0.2)
    assert torch.equal(pa, pb) and torch.equal(ca, cb)


def test_a_wrong_output_size_is_an_error_and_nothing_is_scattered():
    """n_out disagreeing with the scanned total returns an error before the scatter is launched."""
    import ctypes

    from hgin import HginError, _lib, ops
    T, _ = _geometry()
    E = T + 1
    ei = _master()[:, :E].contiguous().to(DEV)
    part = _codes(E).to(DEV)
    true_n = int((part == 2).sum())
    size = ctypes.c_size_t(0)
    _lib.call("hgin_link_split_select_workspace_size", E, ctypes.byref(size))
    ws = torch.empty(size.value, dtype=torch.uint8, device=DEV)
    for n_out in (true_n - 1, true_n + 1):
        out = torch.full((2, n_out), -1, dtype=torch.int64, device=DEV)
        eid = torch.full((n_out,), -1, dtype=torch.int64, device=DEV)
        with pytest.raises(HginError, match="hold"):
            _lib.call("hgin_link_split_select", ops._p(ei), ops._p(part), E, 1 << 2, ops._p(out), ops._p(eid), n_out,
                      ops._p(ws), size.value, ops._stream(ei))
        torch.cuda.synchronize()
        assert bool((out == -1).all()) and bool((eid == -1).all())


# ---------------------------------------------------------------------------------------------------
# link_split on graphs whose endpoint pairs repeat
# ---------------------------------------------------------------------------------------------------
VAL, TEST, SEED = 0.15, 0.15, 12


@functools.lru_cache(maxsize=None)
def _graphs(kind):
    from hgin.data import CONFIGS, component_graph, synthetic_graph
    cfg = CONFIGS["cfg1"]
    g = synthetic_graph(cfg, seed=0) if kind == "single" else component_graph(cfg, 4)
    return cfg, g, g.to(DEV)


def _pairs(ei, n_dst=None):
    ei = ei.cpu().numpy()
    return ei[0] * (1 << 32) + ei[1]


def _positional_split_leaks(ei):
    """A split by edge position (a shuffled 70 / 15 / 15 cut of the columns) of this edge index: whether a held-out
    pair is still among the training edges.  CPU only."""
    E = ei.shape[1]
    perm = np.random.default_rng(0).permutation(E)
    n_test, n_val = int(E * TEST), int(E * VAL)
    pairs = _pairs(ei)
    held, train = pairs[perm[:n_test + n_val]], pairs[perm[n_test + n_val:]]
    return bool(np.isin(held, train).any())


@pytest.mark.parametrize("kind", ["single", "components"])
@pytest.mark.parametrize("disjoint", [0.0, 0.3])
def test_link_split_holds_every_copy_of_a_pair_out_of_both_directions(kind, disjoint):
    import hgin
    from hgin.data import REL_LN, REL_LP, REL_NL, REL_PL
    cfg, g, gd = _graphs(kind)
    ei = g.edge_index[REL_PL]
    E = ei.shape[1]
    pairs = _pairs(ei)
    assert len(np.unique(pairs)) < E, "the generator no longer repeats a pair: pick another seed"
    # a split by position leaks on this very input: a copy of a held-out pair stays among the training edges
    assert _positional_split_leaks(ei)

    sp = hgin.link_split(gd, REL_PL, val=VAL, test=TEST, disjoint=disjoint, seed=SEED)
    assert sp.relation == REL_PL and sp.rev_relation == REL_LP and sp.known is gd.edge_index[REL_PL]
    want = ref_parts(ei, SEED, ref_bounds(VAL, TEST, disjoint))
    assert np.array_equal(sp.part.cpu().numpy(), want)
    assert list(sp.counts) == np.bincount(want, minlength=4).tolist() and sum(sp.counts) == E
    assert min(sp.counts[0], sp.counts[2], sp.counts[3]) > 0 and (sp.counts[1] > 0) == (disjoint > 0)

    # the four parts' eids are a permutation of range(E); every set is the relation's columns at its eids, in order
    eids = [sp.train_eid, sp.val_pos_eid, sp.test_pos_eid] + ([sp.train_pos_eid] if disjoint else [])
    assert torch.equal(torch.cat(eids).sort().values, torch.arange(E, device=DEV))
    for p, (pos, eid) in {0: (sp.train_graph.edge_index[REL_PL], sp.train_eid), 2: (sp.val_pos, sp.val_pos_eid),
                          3: (sp.test_pos, sp.test_pos_eid), 1: (sp.train_pos, sp.train_pos_eid)}.items():
        if p == 1 and not disjoint:
            assert pos is sp.train_graph.edge_index[REL_PL] and eid is sp.train_eid    # the cached CSR is shared
            continue
        assert torch.equal(eid.cpu(), torch.from_numpy(np.flatnonzero(want == p)))
        assert torch.equal(pos, gd.edge_index[REL_PL][:, eid])

    # the reverse relation loses the same pairs: it stays the exact flip of the forward one
    for graph, parts in ((sp.train_graph, (0,)), (sp.val_graph, (0, 1)), (sp.test_graph, (0, 1, 2))):
        fwd, rev = graph.edge_index[REL_PL], graph.edge_index[REL_LP]
        assert torch.equal(rev, fwd.flip(0))
        assert torch.equal(fwd.cpu(), ei[:, torch.from_numpy(np.isin(want, parts))])
    if not disjoint:
        assert sp.val_graph.edge_index[REL_PL] is sp.train_graph.edge_index[REL_PL]

    # leakage: no held-out pair is left, in either direction, in a graph that is encoded to score it
    def inside(pos, graph):
        fwd = np.isin(_pairs(pos), _pairs(graph.edge_index[REL_PL])).any()
        rev = np.isin(_pairs(pos.flip(0)), _pairs(graph.edge_index[REL_LP])).any()
        return bool(fwd or rev)

    assert not inside(sp.val_pos, sp.train_graph) and not inside(sp.test_pos, sp.train_graph)
    assert not inside(sp.test_pos, sp.val_graph) and not inside(sp.val_pos, sp.val_graph)
    assert not inside(sp.test_pos, sp.test_graph)
    if disjoint:
        assert not inside(sp.train_pos, sp.train_graph) and inside(sp.train_pos, sp.val_graph)
    assert inside(sp.val_pos, sp.test_graph)          # the test graph does carry the validation edges

    # everything else is shared by reference
    for graph in (sp.train_graph, sp.val_graph, sp.test_graph):
        assert list(graph.edge_index) == list(gd.edge_index)
        assert graph.edge_index[REL_LN] is gd.edge_index[REL_LN] and graph.edge_index[REL_NL] is gd.edge_index[REL_NL]
        assert graph.y is gd.y
        assert all(graph.x[t] is gd.x[t] and graph.batch[t] is gd.batch[t] for t in gd.x)


def test_rev_relation_none_leaves_the_reverse_relation_alone():
    import hgin
    from hgin.data import REL_LP, REL_PL
    _, _, gd = _graphs("single")
    sp = hgin.link_split(gd, REL_PL, rev_relation=None, val=VAL, test=TEST, seed=SEED)
    assert sp.rev_relation is None
    assert all(g.edge_index[REL_LP] is gd.edge_index[REL_LP] for g in (sp.train_graph, sp.val_graph, sp.test_graph))
    both = hgin.link_split(gd, REL_PL, rev_relation=REL_LP, val=VAL, test=TEST, seed=SEED)
    assert torch.equal(both.train_graph.edge_index[REL_PL], sp.train_graph.edge_index[REL_PL])
    assert int(both.train_graph.edge_index[REL_LP].size(1)) == sp.counts[0]


def _model(cfg):
    import hgin
    torch.manual_seed(1997)
    ic = {"link": cfg.f_link, "path": cfg.f_path, "node": cfg.f_node}
    return hgin.HetroGIN(**cfg.model_kwargs(ic)).to(DEV).train()


@pytest.mark.parametrize("kind", ["single", "components"])
def test_encode_on_the_train_graph_equals_encode_on_a_host_masked_graph(kind):
    import hgin
    from hgin.data import REL_LP, REL_PL, HeteroGraph
    cfg, g, gd = _graphs(kind)
    sp = hgin.link_split(gd, REL_PL, val=VAL, test=TEST, disjoint=0.3, seed=SEED)
    bounds = ref_bounds(VAL, TEST, 0.3)
    keep_f = torch.from_numpy(ref_parts(g.edge_index[REL_PL], SEED, bounds) == 0)
    keep_r = torch.from_numpy(ref_parts(g.edge_index[REL_LP], SEED, bounds, swap=True) == 0)
    ei = dict(gd.edge_index)
    ei[REL_PL] = g.edge_index[REL_PL][:, keep_f].contiguous().to(DEV)
    ei[REL_LP] = g.edge_index[REL_LP][:, keep_r].contiguous().to(DEV)
    host_cut = HeteroGraph(gd.x, ei, gd.y, gd.batch)
    model = _model(cfg).eval()
    with torch.no_grad():
        got = model.encode(sp.train_graph.x_dict(), sp.train_graph.edge_index_dict())
        want = model.encode(host_cut.x_dict(), host_cut.edge_index_dict())
        full = model.encode(gd.x_dict(), gd.edge_index_dict())
    assert sorted(got) == sorted(want)
    for t in want:
        assert torch.equal(got[t], want[t]), t
    assert not torch.equal(got["link"], full["link"])     # the held-out edges did carry messages before


# ---------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------
def _finite(metrics):
    return sorted(metrics) == ["auc", "hits@1", "hits@10", "hits@3", "mrr"] and \
        all(math.isfinite(float(v)) for v in metrics.values())


@pytest.mark.parametrize("kind,graph_local", [("single", False), ("components", True)])
def test_train_on_the_train_graph_and_rank_the_held_out_edges(kind, graph_local):
    import hgin
    from hgin.data import REL_PL
    cfg, _, gd = _graphs(kind)
    sp = hgin.link_split(gd, REL_PL, val=VAL, test=TEST, disjoint=0.3, seed=SEED)
    model = _model(cfg)
    pred = hgin.LinkPredictor(model, REL_PL, 3, 7, graph_local=graph_local)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    losses = [float(hgin.link_train_step(model, opt, sp.train_graph, pred, s, pos=sp.train_pos)) for s in range(3)]
    assert all(np.isfinite(losses)) and len(set(losses)) == 3
    filt = float(hgin.link_train_step(model, opt, sp.train_graph, pred, 3, pos=sp.train_pos, known=sp.known))
    assert math.isfinite(filt)
    assert _finite(pred.full_metrics(sp.val_graph, pos=sp.val_pos, known=sp.known))
    assert _finite(pred.full_metrics(sp.test_graph, pos=sp.test_pos, known=sp.known))


def test_link_train_step_without_pos_keeps_todays_loss_bits():
    import hgin
    from hgin.data import REL_PL
    cfg, _, gd = _graphs("single")
    a = _model(cfg)
    b = copy.deepcopy(a)
    want = hgin.LinkPredictor(a, REL_PL, 3, 7).loss(gd, step=2).detach()
    opt = torch.optim.Adam(b.parameters(), lr=1e-3)
    got = hgin.link_train_step(b, opt, gd, hgin.LinkPredictor(b, REL_PL, 3, 7), step=2)
    assert torch.equal(got, want)
    # and pos / known reach predictor.loss: the relation's own edges given explicitly are the same call
    c = copy.deepcopy(a)
    opt = torch.optim.Adam(c.parameters(), lr=1e-3)
    pos = gd.edge_index[REL_PL]
    assert torch.equal(hgin.link_train_step(c, opt, gd, hgin.LinkPredictor(c, REL_PL, 3, 7), step=2, pos=pos), want)
    d = copy.deepcopy(a)
    opt = torch.optim.Adam(d.parameters(), lr=1e-3)
    filt = hgin.link_train_step(d, opt, gd, hgin.LinkPredictor(d, REL_PL, 3, 7), step=2, known=pos)
    assert torch.equal(filt, hgin.LinkPredictor(a, REL_PL, 3, 7).loss(gd, step=2, known=pos).detach())
    assert not torch.equal(filt, want)
