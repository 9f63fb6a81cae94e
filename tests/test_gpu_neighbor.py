"""Neighbour-sampled mini-batches (include/hgin.h A22) on the device: the sampling kernels and the subgraph against the
numpy restatement of tests/test_neighbor_host.py bit for bit, the resident map's state, and the encode / step / training
equivalences of the link layer built on them."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from test_neighbor_host import ref_csr, ref_picks, ref_sample

DEV = "cuda"
pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789
FANOUTS = [1, 5, 32, 128, -1]
FRONTIERS = [1, 63, 64, 65, 257, 1100]
N_SRC, N_DST = 500, 1200


# ---------------------------------------------------------------------------------------------------
# one hop, one relation: the kernels themselves
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bipartite(f):
    """Destination rows whose degrees cycle through 0, 1, f - 1, f, f + 1, 300 (f = 5 for the all-neighbours case), in
    shuffled edge order; (edge_index cpu, (rowptr, col, perm) numpy, the device Csr)."""
    from hgin import ops
    fe = 5 if f == -1 else f
    degs = [0, 1, max(fe - 1, 0), fe, fe + 1, 300]
    g = torch.Generator().manual_seed(100 + fe)
    dst = torch.cat([torch.full((degs[v % 6],), v, dtype=torch.long) for v in range(N_DST)])
    src = torch.randint(0, N_SRC, (dst.numel(),), generator=g)
    order = torch.randperm(dst.numel(), generator=g)
    ei = torch.stack([src[order], dst[order]])
    csr = ops.build_csr(ei.to(DEV), 1, N_DST, N_SRC)
    ref = ref_csr(ei, N_DST)
    assert np.array_equal(csr.rowptr.cpu().numpy(), ref[0]) and np.array_equal(csr.col.cpu().numpy(), ref[1])
    assert np.array_equal(csr.perm.cpu().numpy(), ref[2])
    return ei, ref, csr


def _one_hop(csr, frontier, f, seed, offset, slot):
    """(off, src, eid) as numpy through hgin_neighbor_sample_offsets + hgin_neighbor_sample."""
    from hgin import _lib, ops
    n = int(frontier.numel())
    off = torch.full((n + 1,), -7, dtype=torch.int64, device=DEV)
    size = ctypes.c_size_t(0)
    _lib.call("hgin_neighbor_sample_workspace_size", n, ctypes.byref(size))
    ws = torch.empty(size.value, dtype=torch.uint8, device=DEV)
    _lib.call("hgin_neighbor_sample_offsets", ops._p(csr.rowptr), csr.n_rows, ops._p(frontier), n, f, ops._p(off),
              ops._p(ws), size.value, ops._stream(off))
    tot = int(off[-1])
    src = torch.full((tot,), -7, dtype=torch.int64, device=DEV)
    eid = torch.full((tot,), -7, dtype=torch.int64, device=DEV)
    _lib.call("hgin_neighbor_sample", ops._p(csr.rowptr), ops._p(csr.col), ops._p(csr.perm), csr.n_rows,
              ops._p(frontier), n, f, seed, offset, slot, ops._p(off), ops._p(src), ops._p(eid), tot, ops._stream(off))
    return off.cpu().numpy(), src.cpu().numpy(), eid.cpu().numpy()


def _ref_one_hop(ref, frontier, f, seed, offset, slot):
    rowptr, col, perm = ref
    off, src, eid = [0], [], []
    for v in frontier:
        for p in ref_picks(rowptr, int(v), f, seed, offset, slot):
            src.append(int(col[rowptr[v] + p]))
            eid.append(int(perm[rowptr[v] + p]))
        off.append(len(src))
    return np.asarray(off), np.asarray(src, dtype=np.int64), np.asarray(eid, dtype=np.int64)


@pytest.mark.parametrize("n", FRONTIERS)
@pytest.mark.parametrize("f", FANOUTS)
def test_one_hop_matches_the_restatement(f, n):
    """Every degree class (0, 1, f - 1, f, f + 1, 300) sits in every frontier of six or more nodes, in an order that is
    not the id order; frontiers of 1 .. 1100 nodes cover one lane group, one wave, one workgroup and several."""
    ei, ref, csr = _bipartite(f)
    g = torch.Generator().manual_seed(7 * n + (f & 0xFF))
    frontier = torch.randperm(N_DST, generator=g)[:n] if n > 1 else torch.tensor([5])   # node 5: degree 300
    for offset, slot in ((0, 0), (2**32 - 1, 3)):
        got = _one_hop(csr, frontier.to(DEV), f, SEED, offset, slot)
        want = _ref_one_hop(ref, frontier.numpy(), f, SEED, offset, slot)
        for a, b, what in zip(got, want, ("off", "src", "eid")):
            assert np.array_equal(a, b), (what, f, n, offset)
    if f != -1 and n >= 64:
        other = _one_hop(csr, frontier.to(DEV), f, SEED, 1, 0)
        assert not np.array_equal(other[2], _ref_one_hop(ref, frontier.numpy(), f, SEED, 0, 0)[2])


def test_empty_frontier_and_a_relation_without_edges():
    from hgin import ops
    _, ref, csr = _bipartite(5)
    off, src, eid = _one_hop(csr, torch.empty(0, dtype=torch.int64, device=DEV), 5, SEED, 0, 0)
    assert off.tolist() == [0] and src.size == 0 and eid.size == 0
    none = ops.build_csr(torch.empty((2, 0), dtype=torch.int64, device=DEV), 1, N_DST, N_SRC)
    frontier = torch.arange(0, 300, dtype=torch.int64, device=DEV)
    for f in (3, -1):
        off, src, eid = _one_hop(none, frontier, f, SEED, 0, 0)
        assert off.tolist() == [0] * 301 and src.size == 0


def test_fresh_map_set_and_emit():
    from hgin import _lib, ops
    m = torch.full((50,), -1, dtype=torch.int32, device=DEV)
    ids = torch.tensor([40, 3, 17], dtype=torch.int64, device=DEV)
    _lib.call("hgin_neighbor_map_set", ops._p(m), 50, ops._p(ids), 3, 10, ops._stream(m))
    want = torch.full((50,), -1, dtype=torch.int32)
    want[[40, 3, 17]] = torch.tensor([10, 11, 12], dtype=torch.int32)
    assert torch.equal(m.cpu(), want)
    src = torch.tensor([3, 4, 40, 40, 0, 17, 49], dtype=torch.int64, device=DEV)
    out = torch.empty(7, dtype=torch.int64, device=DEV)
    _lib.call("hgin_neighbor_fresh", ops._p(m), 50, ops._p(src), 7, 50, ops._p(out), ops._stream(m))
    assert out.tolist() == [50, 4, 50, 50, 0, 50, 49]
    # frontier rows of 2, 0, 0, 3, 1, 0 edges; sources that all have a row
    off = torch.tensor([0, 2, 2, 2, 5, 6, 6], dtype=torch.int64, device=DEV)
    esrc = torch.tensor([3, 40, 17, 17, 3, 40], dtype=torch.int64, device=DEV)
    edge = torch.empty((2, 6), dtype=torch.int64, device=DEV)
    _lib.call("hgin_neighbor_emit", ops._p(m), 50, ops._p(esrc), ops._p(off), 6, 100, 6, ops._p(edge), ops._stream(m))
    assert edge.tolist() == [[11, 10, 12, 12, 11, 10], [100, 100, 103, 103, 103, 104]]
    _lib.call("hgin_neighbor_map_set", ops._p(m), 50, ops._p(ids), 3, -1, ops._stream(m))
    assert bool((m == -1).all())


# ---------------------------------------------------------------------------------------------------
# the subgraph
# ---------------------------------------------------------------------------------------------------
HUB = 300     # extra in-edges planted on link 0


@functools.lru_cache(maxsize=None)
def _graphs(bf16=False):
    """cfg1 at 0.3 (180 paths, 90 links, 30 nodes, four conv relations) with a hub: link 0 gets HUB more path -> link
    edges (and their flips).  (cpu graph, device graph)."""
    from hgin.data import CONFIGS, REL_LP, REL_PL, HeteroGraph, scaled_config, synthetic_graph
    g = synthetic_graph(scaled_config(CONFIGS["cfg1"], 0.3), seed=4)
    gen = torch.Generator().manual_seed(9)
    extra = torch.stack([torch.randint(0, g.x["path"].size(0), (HUB,), generator=gen),
                         torch.zeros(HUB, dtype=torch.long)])
    where = torch.randperm(g.edge_index[REL_PL].size(1) + HUB, generator=gen)
    pl = torch.cat([g.edge_index[REL_PL], extra], 1)[:, where].contiguous()
    ei = dict(g.edge_index)
    ei[REL_PL], ei[REL_LP] = pl, pl.flip(0).contiguous()
    x = {t: (v.to(torch.bfloat16) if bf16 else v) for t, v in g.x.items()}
    batch = {t: torch.arange(v.size(0)) % 3 for t, v in g.x.items()}     # something to gather
    cpu = HeteroGraph(x, ei, g.y, batch)
    return cpu, cpu.to(DEV)


def _dev_seeds(seeds):
    return {t: torch.tensor(v, dtype=torch.int64, device=DEV) for t, v in seeds.items()}


def _assert_sub(sub, ref, cpu, relations):
    n_id, edges, e_id, n_seed = ref
    assert sub.n_seed == n_seed
    assert set(sub.n_id) == set(n_id)
    for t in n_id:
        assert np.array_equal(sub.n_id[t].cpu().numpy(), n_id[t]), t
        assert torch.equal(sub.graph.x[t].cpu(), cpu.x[t][torch.from_numpy(n_id[t])]), t
        assert sub.graph.x[t].dtype == cpu.x[t].dtype
        assert torch.equal(sub.graph.batch[t].cpu(), cpu.batch[t][torch.from_numpy(n_id[t])]), t
    assert torch.equal(sub.graph.y.cpu(), cpu.y[torch.from_numpy(n_id["path"])])
    assert list(sub.graph.edge_index) == list(relations) and list(sub.e_id) == list(relations)
    for r in relations:
        got = sub.graph.edge_index[r]
        assert got.dtype == torch.int64 and tuple(got.shape) == edges[r].shape, r
        assert np.array_equal(got.cpu().numpy(), edges[r]), r
        assert np.array_equal(sub.e_id[r].cpu().numpy(), e_id[r]), r
    assert sub.graph.static_features is False


SEEDS = {
    "two types with repeats": {"path": [5, 1, 5, 30, 179, 30], "link": [0, 2, 2, 9, 89]},
    "paths only": {"path": [7, 3]},
    "nodes and paths": {"node": [4, 4, 29], "path": [11]},
}
FANS = [[3], [3, 2], [3, 2, 1], [-1, 2], [128, 1, 5], [2, 2, 2]]


@pytest.mark.parametrize("fanouts", FANS, ids=lambda f: "-".join(map(str, f)))
@pytest.mark.parametrize("case", list(SEEDS))
def test_subgraph_matches_the_restatement(case, fanouts):
    import hgin
    cpu, dev = _graphs()
    rels = list(cpu.edge_index.keys())
    sampler = hgin.NeighborSampler(dev, fanouts=fanouts, seed=SEED)
    for offset in (0, 5):
        sub = sampler.sample(_dev_seeds(SEEDS[case]), offset=offset)
        ref = ref_sample(cpu, rels, fanouts, SEEDS[case], SEED, offset)
        _assert_sub(sub, ref, cpu, rels)
    for t, ids in SEEDS[case].items():
        want = np.searchsorted(ref[0][t][:ref[3][t]], np.asarray(ids))
        assert np.array_equal(sub.local(t, torch.tensor(ids, device=DEV)).cpu().numpy(), want)
        assert np.array_equal(ref[0][t][want], np.asarray(ids))
    absent = next(i for i in range(180) if i not in SEEDS[case].get("path", []))
    with pytest.raises(IndexError):
        sub.local("path", torch.tensor([absent], device=DEV))
    for m in sampler._maps.values():
        assert bool((m == -1).all())


def test_the_cases_the_subgraph_rule_is_about_occur():
    """On the reference: a link reached through two relations in one hop, a seed reached again at a later hop and not
    re-added, a seed type without seeds, an empty hop-2 frontier, the hub row cut to the fanout."""
    from hgin.data import REL_LN, REL_LP, REL_PL
    cpu, _ = _graphs()
    rels = list(cpu.edge_index.keys())
    n_id, edges, e_id, n_seed = ref_sample(cpu, rels, [3], SEEDS["nodes and paths"], SEED, 0)
    via_lp = set(edges[REL_LP][0].tolist())
    via_ln = set(edges[REL_LN][0].tolist())
    assert n_seed["link"] == 0 and via_lp | via_ln == set(range(len(n_id["link"])))
    both = ref_sample(cpu, rels, [-1], {"node": list(range(30)), "path": list(range(180))}, SEED, 0)
    assert set(both[1][REL_LP][0].tolist()) & set(both[1][REL_LN][0].tolist())
    n_id, edges, e_id, n_seed = ref_sample(cpu, rels, [3, 2, 1], SEEDS["two types with repeats"], SEED, 0)
    assert n_seed == {"path": 4, "link": 4, "node": 0}
    assert (edges[REL_PL][0] < n_seed["path"]).any() and len(set(n_id["path"].tolist())) == len(n_id["path"])
    hub_edges = (edges[REL_PL][1] == 0).sum()
    assert hub_edges == 3 and (cpu.edge_index[REL_PL][1] == 0).sum() > HUB
    # paths only: hop 1 reaches links alone, so the hop-2 frontiers of paths and nodes are empty
    n_id, edges, e_id, n_seed = ref_sample(cpu, rels, [3], SEEDS["paths only"], SEED, 0)
    assert len(n_id["path"]) == n_seed["path"] and len(n_id["node"]) == 0 and len(n_id["link"]) > 0


def test_bf16_features_and_a_relation_subset():
    import hgin
    from hgin.data import REL_LP, REL_PL
    cpu, dev = _graphs(True)
    rels = [REL_LP, REL_PL]
    sampler = hgin.NeighborSampler(dev, fanouts=[4, 2], relations=rels, seed=3)
    sub = sampler.sample(_dev_seeds(SEEDS["two types with repeats"]), offset=2)
    assert sub.graph.x["path"].dtype == torch.bfloat16
    _assert_sub(sub, ref_sample(cpu, rels, [4, 2], SEEDS["two types with repeats"], 3, 2), cpu, rels)


def test_state_is_clean_between_calls_and_after_an_error():
    import hgin
    cpu, dev = _graphs()
    rels = list(cpu.edge_index.keys())
    a, b = SEEDS["two types with repeats"], SEEDS["nodes and paths"]
    one = hgin.NeighborSampler(dev, fanouts=[3, 2], seed=1)
    s1, s2, s3 = one.sample(_dev_seeds(a), 0), one.sample(_dev_seeds(b), 1), one.sample(_dev_seeds(b), 1)
    f1 = hgin.NeighborSampler(dev, fanouts=[3, 2], seed=1).sample(_dev_seeds(a), 0)
    f2 = hgin.NeighborSampler(dev, fanouts=[3, 2], seed=1).sample(_dev_seeds(b), 1)
    for x, y in ((s1, f1), (s2, f2), (s3, f2)):
        for t in x.n_id:
            assert torch.equal(x.n_id[t], y.n_id[t])
        for r in rels:
            assert torch.equal(x.graph.edge_index[r], y.graph.edge_index[r]) and torch.equal(x.e_id[r], y.e_id[r])
    with pytest.raises(IndexError):
        one.sample({"path": torch.tensor([0, 180], device=DEV), "link": torch.tensor([1], device=DEV)}, 2)
    for m in one._maps.values():
        assert bool((m == -1).all())
    _assert_sub(one.sample(_dev_seeds(a), 0), ref_sample(cpu, rels, [3, 2], a, 1, 0), cpu, rels)


# ---------------------------------------------------------------------------------------------------
# the link layer
# ---------------------------------------------------------------------------------------------------
def _model(seed=1997):
    import hgin
    from hgin.data import CONFIGS
    cfg = CONFIGS["cfg1"]
    torch.manual_seed(seed)
    model = hgin.HetroGIN(**cfg.model_kwargs({"link": cfg.f_link, "path": cfg.f_path, "node": cfg.f_node}))
    return model.to(DEV), cfg.layers


@pytest.mark.parametrize("case", ["two types with repeats", "paths only"])
def test_encode_of_the_full_fanout_subgraph_matches_the_full_graph(case):
    """fanouts = [-1] * layers: the seeds' embeddings see their whole L-hop neighbourhood.  "paths only" leaves the
    relation link -> node without an edge (no node is ever expanded)."""
    import hgin
    from hgin.data import REL_LN
    _, dev = _graphs()
    model, layers = _model()
    sub = hgin.NeighborSampler(dev, fanouts=[-1] * layers, seed=0).sample(_dev_seeds(SEEDS[case]), 0)
    if case == "paths only":
        assert sub.graph.edge_index[REL_LN].size(1) == 0
    with torch.no_grad():
        z_full = model.encode(dev.x_dict(), dev.edge_index_dict())
        z_sub = model.encode(sub.graph.x_dict(), sub.graph.edge_index_dict())
    for t, n in sub.n_seed.items():
        if n == 0:
            continue
        want = z_full[t][sub.n_id[t][:n]].double()
        got = z_sub[t][:n].double()
        d, nz = float((got - want).norm()), float(want.norm())
        print(f"{case} / {t}: {n} seed rows, ||dz|| / ||z|| = {d / nz:.3g}, bit-equal: {torch.equal(got, want)}")
        assert nz > 0 and d <= 1e-5 * nz + 1e-9, (t, d, nz)


@pytest.mark.parametrize("objective", ["bce", "softmax"])
def test_batch_loss_of_all_positives_matches_the_full_graph_loss(objective):
    import hgin
    from hgin.data import REL_PL
    from hgin.linkpred import negative_edges
    _, dev = _graphs()
    model, layers = _model()
    pos = dev.edge_index[REL_PL]
    B, k, step = int(pos.size(1)), 3, 2
    n_dst = dev.x["link"].size(0)
    pred = hgin.LinkPredictor(model, REL_PL, k=k, seed=11, objective=objective)
    sampler = hgin.NeighborSampler(dev, fanouts=[-1] * layers, seed=5)

    model.zero_grad()
    full = pred.loss(dev, pos=pos, step=step)
    full.backward()
    g_full = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    model.zero_grad()
    got = pred.batch_loss(sampler, pos, step=step)
    got.backward()
    g_got = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}

    # the negatives are negative_edges' global destinations
    neg = negative_edges(pos, n_dst, k, 11, step * B * k)[1].view(B, k)
    batch = hgin.link_neighbor_batch(sampler, REL_PL, pos, neg, offset=step)
    assert torch.equal(batch.sub.n_id["link"][batch.neg_dst.long()], neg)
    assert torch.equal(batch.sub.n_id["path"][batch.pos[0]], pos[0])
    assert torch.equal(batch.sub.n_id["link"][batch.pos[1]], pos[1])
    assert batch.neg_dst.dtype == torch.int32 and batch.pos.dtype == torch.int64
    with torch.no_grad():
        z = model.encode(batch.sub.graph.x_dict(), batch.sub.graph.edge_index_dict())
        again = hgin.sampled_link_loss(z["path"], z["link"], batch.pos, 0, 11, 0, objective, neg_dst=batch.neg_dst)
    assert torch.equal(again, got.detach())

    got, full = float(got.detach()), float(full.detach())
    dl = abs(got - full)
    print(f"{objective}: loss {full:.6g}, |dloss| / |loss| = {dl / abs(full):.3g}")
    assert set(g_got) == set(g_full)
    for n, want in g_full.items():
        d, nz = float((g_got[n].double() - want.double()).norm()), float(want.double().norm())
        print(f"  {n}: ||dg|| / ||g|| = {d / max(nz, 1e-300):.3g} (||g|| = {nz:.3g})")
    assert dl <= 1e-5 * abs(full), (dl, full)
    for n, want in g_full.items():
        d, nz = float((g_got[n].double() - want.double()).norm()), float(want.double().norm())
        assert d <= 1e-5 * nz + 1e-9, (n, d, nz)


def test_filtered_batch_negatives_are_not_known_edges():
    import hgin
    from hgin.data import REL_PL
    from hgin.linkpred import negative_edges
    _, dev = _graphs()
    model, _ = _model()
    pos = dev.edge_index[REL_PL][:, 40:200].contiguous()
    B, k, step = int(pos.size(1)), 4, 3
    n_dst = int(dev.x["link"].size(0))
    known = dev.edge_index[REL_PL]
    neg = negative_edges(pos, n_dst, k, 21, step * B * k, known=known)[1].view(B, k)
    have = set((known[0] * n_dst + known[1]).tolist())
    assert not (set((pos[0].repeat_interleave(k) * n_dst + neg.reshape(-1)).tolist()) & have)
    # batch_loss draws exactly these: the loss equals the one built by hand from them, bit for bit
    pred = hgin.LinkPredictor(model, REL_PL, k=k, seed=21, filter_negatives=True)
    sampler = hgin.NeighborSampler(dev, fanouts=[3, 2], seed=5)
    with torch.no_grad():
        got = pred.batch_loss(sampler, pos, step=step)
        batch = hgin.link_neighbor_batch(sampler, REL_PL, pos, neg, offset=step)
        z = model.encode(batch.sub.graph.x_dict(), batch.sub.graph.edge_index_dict())
        want = hgin.sampled_link_loss(z["path"], z["link"], batch.pos, 0, 21, 0, neg_dst=batch.neg_dst)
    assert torch.equal(got, want)
    local_neg_global = batch.sub.n_id["link"][batch.neg_dst.long()]
    assert not (set((pos[0].repeat_interleave(k) * n_dst + local_neg_global.reshape(-1)).tolist()) & have)
    unfiltered = negative_edges(pos, n_dst, k, 21, step * B * k)[1]
    assert set((pos[0].repeat_interleave(k) * n_dst + unfiltered).tolist()) & have     # the filter had work to do


def test_five_minibatch_steps_are_reproducible():
    import hgin
    from hgin.data import REL_PL
    _, dev = _graphs()
    pos = dev.edge_index[REL_PL]
    runs = []
    for _ in range(2):
        model, _layers = _model(seed=5)
        before = [p.detach().clone() for p in model.parameters()]
        opt = torch.optim.Adam(model.parameters(), lr=1e-2)
        pred = hgin.LinkPredictor(model, REL_PL, k=3, seed=8)
        sampler = hgin.NeighborSampler(dev, fanouts=[3, 2], seed=2)
        losses = [hgin.link_minibatch_step(model, opt, sampler, pred, pos[:, 64 * s:64 * s + 64].contiguous(), s)
                  for s in range(5)]
        runs.append((torch.stack(losses), [p.detach().clone() for p in model.parameters()], before))
    (l1, p1, b1), (l2, p2, _) = runs
    assert bool(torch.isfinite(l1).all())
    assert torch.equal(l1, l2)
    assert all(torch.equal(a, b) for a, b in zip(p1, p2))
    assert any(not torch.equal(a, b) for a, b in zip(p1, b1))
