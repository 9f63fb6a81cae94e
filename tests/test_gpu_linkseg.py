"""Graph-local negatives and candidates of the link head on the GPU (include/hgin.h A19, ``segments=``).

Draws: bit for bit tests/test_linkseg_host.py's numpy restatement (Philox words from the C oracle), in the unfused
``negative_edges`` and in the fused forward's saved pairs.  Anchors: with one graph every segmented call equals the
unsegmented one bit for bit (loss, both gradients, sampled ranks, full ranks, top-K); with several graphs the segmented
loss equals the A18 call that is given the same destinations, bit for bit.  Loss and gradients against the float64
references of tests/test_linkpred_host.py / tests/test_linkobj_host.py on the reference draws and against the unfused
``link_loss(segments=)``, within tests/test_gpu_linkpred.py::_check's bounds (imported, not re-chosen).  Full ranks:
exact on integer embeddings against ``ref_seg_full_ranks``; on random floats one segmented call equals, bit for bit, the
unsegmented calls run per graph on the sliced tensors, and so does top-K (indices shifted, scores as bits).  Model
level: ``LinkPredictor(graph_local=True)`` on ``component_graph(cfg1, 4)``."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_linkobj import PARAMS
from test_gpu_linkpred import E, N_SRC, REL_PL, SEED, _check, _inputs
from test_linkobj_host import ref_obj_loss_and_grads
from test_linkpred_host import ref_loss_and_grads
from test_linkseg_host import ref_seg_draws, ref_seg_full_ranks

DEV = "cuda"
pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------
# loss and sampler: destination segments (1, 5, 53, 200), sources shuffled across the graphs
# ---------------------------------------------------------------------------------------------------
LOSS_SEGS = (1, 5, 53, 200)
KS, OFFS, FS = (1, 3, 5), (6, 2**32 + 1), (6, 128, 260)
OBJECTIVES = (("bce", 0.0), ("softmax", PARAMS["softmax"][-1]), ("bpr", 0.0), ("selfadv", PARAMS["selfadv"][-1]))
LOSS_CASES = [(o, p, k, off, F) for o, p in OBJECTIVES for k in KS for off in OFFS for F in FS]


def _obj_kw(objective, param):
    return {"softmax": dict(objective=objective, temperature=param), "selfadv": dict(objective=objective, alpha=param),
            "bpr": dict(objective=objective)}.get(objective, {})


@functools.lru_cache(maxsize=None)
def _loss_inputs(F):
    """(pos, zs, zd, src_seg, dst_ptr, LinkSegments on the device): 37 sources dealt to the four graphs in a shuffled
    order (30 of them own positives), every positive's destination drawn inside its source's graph."""
    from hgin import LinkSegments
    g = torch.Generator().manual_seed(977 + F)
    n_dst = sum(LOSS_SEGS)
    src_seg = torch.arange(N_SRC) % len(LOSS_SEGS)
    src_seg = src_seg[torch.randperm(N_SRC, generator=g)]
    ptr = torch.tensor((0,) + LOSS_SEGS).cumsum(0)
    src = torch.randint(0, 30, (E,), generator=g)
    gs = src_seg[src]
    dst = ptr[gs] + (torch.rand(E, generator=g, dtype=torch.float64) * (ptr[gs + 1] - ptr[gs])).long()
    pos = torch.stack([src, dst])
    assert int((gs == 0).sum()) >= 10 and len(set(gs.tolist())) == 4
    zs = torch.randn(N_SRC, F, generator=g) * 0.5
    zd = torch.randn(n_dst, F, generator=g) * 0.5
    batch_dst = torch.repeat_interleave(torch.arange(len(LOSS_SEGS)), torch.tensor(LOSS_SEGS))
    seg = LinkSegments(src_seg.to(DEV), batch_dst.to(DEV))
    assert seg.dst_ptr.cpu().tolist() == ptr.tolist()
    return pos, zs, zd, src_seg.numpy(), ptr.numpy(), seg


def _run(zs, zd, pos, k, off, objective="bce", param=0.0, **kw):
    """(loss, g_src, g_dst, negatives [2, E K]) of one fused forward + backward on the device."""
    from hgin.linkpred import _SampledLinkLossFn, sampled_link_loss
    a, b = zs.detach().clone().requires_grad_(True), zd.detach().clone().requires_grad_(True)
    loss = sampled_link_loss(a, b, pos, k, SEED, off, **_obj_kw(objective, param), **kw)
    assert isinstance(loss.grad_fn, _SampledLinkLossFn._backward_cls)
    coef, neg, sa, sb = loss.grad_fn.saved_tensors   # nothing else is saved
    assert sa.data_ptr() == a.data_ptr() and sb.data_ptr() == b.data_ptr()
    loss.backward()
    return loss.detach(), a.grad, b.grad, neg


@functools.lru_cache(maxsize=None)
def _draws(k, off, F):
    pos, _, _, src_seg, ptr, _ = _loss_inputs(F)
    return ref_seg_draws(SEED, off, pos[0].numpy(), k, src_seg, ptr)


@functools.lru_cache(maxsize=None)
def _loss_case(objective, param, k, off, F):
    pos, zs, zd, src_seg, ptr, seg = _loss_inputs(F)
    posd, zsd, zdd = pos.to(DEV), zs.to(DEV), zd.to(DEV)
    loss, g_src, g_dst, neg = _run(zsd, zdd, posd, k, off, objective, param, segments=seg)
    want = _draws(k, off, F)
    if objective == "bce":
        ref = ref_loss_and_grads(zs, zd, pos, want, k)
    else:
        ref = ref_obj_loss_and_grads(zs, zd, pos, want, k, objective, param)
    return dict(pos=pos, posd=posd, zs=zs, zd=zd, zsd=zsd, zdd=zdd, seg=seg, loss=loss, g_src=g_src, g_dst=g_dst,
                neg=neg, want=want, ref=ref, src_seg=src_seg, ptr=ptr)


@pytest.mark.parametrize("objective,param,k,off,F", LOSS_CASES)
def test_draws_are_the_reference_bit_for_bit_and_stay_in_the_graph(objective, param, k, off, F):
    from hgin.linkpred import negative_edges
    c = _loss_case(objective, param, k, off, F)
    neg = c["neg"].cpu()
    assert neg.dtype == torch.int64 and tuple(neg.shape) == (2, E * k)
    assert np.array_equal(neg[1].numpy(), c["want"].astype(np.int64))
    assert torch.equal(neg[0], c["pos"][0].repeat_interleave(k))
    assert torch.equal(negative_edges(c["posd"], sum(LOSS_SEGS), k, SEED, off, segments=c["seg"]).cpu(), neg)
    g = c["src_seg"][neg[0].numpy()]
    d = neg[1].numpy()
    assert (d >= c["ptr"][g]).all() and (d < c["ptr"][g + 1]).all()
    assert (g == 0).any() and (d[g == 0] == 0).all()      # the one-destination graph always yields that destination
    assert len(set(d[g == 3].tolist())) > 20              # and the large one is really sampled


@pytest.mark.parametrize("objective,param,k,off,F", LOSS_CASES)
def test_loss_and_gradients_vs_float64_reference_and_link_loss(objective, param, k, off, F):
    from hgin.linkpred import link_loss
    c = _loss_case(objective, param, k, off, F)
    assert c["loss"].dim() == 0 and c["loss"].dtype == torch.float32
    _check(c["loss"], c["g_src"], c["g_dst"], c["ref"], f"segmented {objective} vs float64")
    a, b = c["zsd"].clone().requires_grad_(True), c["zdd"].clone().requires_grad_(True)
    base = link_loss(a, b, c["posd"], k, SEED, off, segments=c["seg"], **_obj_kw(objective, param))
    base.backward()
    _check(c["loss"], c["g_src"], c["g_dst"], (base.detach().cpu(), a.grad.cpu(), b.grad.cpu()),
           f"segmented {objective} vs link_loss")


@pytest.mark.parametrize("objective,param,k,off,F", LOSS_CASES)
def test_the_a18_anchor_and_determinism_are_bitwise(objective, param, k, off, F):
    """A segmented draw carries the bits the same destination carries as a given negative (A18): (k, segments) equals
    (0, neg_dst = the draws), also with m extra given negatives behind the draws; and a second run repeats the first."""
    from hgin.linkpred import link_ranks
    c = _loss_case(objective, param, k, off, F)
    zsd, zdd, posd, seg = c["zsd"], c["zdd"], c["posd"], c["seg"]
    again = _run(zsd, zdd, posd, k, off, objective, param, segments=seg)
    draws = torch.as_tensor(c["want"].astype(np.int32)).view(E, k).to(DEV)
    given = _run(zsd, zdd, posd, 0, off, objective, param, neg_dst=draws)
    for got in (again, given):
        assert torch.equal(got[0], c["loss"]) and torch.equal(got[1], c["g_src"]) and torch.equal(got[2], c["g_dst"])
        assert torch.equal(got[3], c["neg"])
    if objective == "bce":   # the ranks have no objective
        assert all(torch.equal(x, y) for x, y in zip(link_ranks(zsd, zdd, posd, k, SEED, off, segments=seg),
                                                     link_ranks(zsd, zdd, posd, 0, SEED, off, neg_dst=draws)))
    m = 2
    g = torch.Generator().manual_seed(k + F)
    ptr = torch.as_tensor(c["ptr"])
    gs = torch.as_tensor(c["src_seg"])[c["pos"][0]]
    extra = (ptr[gs][:, None] + (torch.rand(E, m, generator=g, dtype=torch.float64)
                                 * (ptr[gs + 1] - ptr[gs])[:, None]).long()).to(torch.int32).to(DEV)
    both = _run(zsd, zdd, posd, k, off, objective, param, neg_dst=extra, segments=seg)
    flat = _run(zsd, zdd, posd, 0, off, objective, param, neg_dst=torch.cat([draws, extra], 1).contiguous())
    assert all(torch.equal(x, y) for x, y in zip(both, flat))
    if objective == "bce":
        assert all(torch.equal(x, y) for x, y in zip(
            link_ranks(zsd, zdd, posd, k, SEED, off, neg_dst=extra, segments=seg),
            link_ranks(zsd, zdd, posd, 0, SEED, off, neg_dst=torch.cat([draws, extra], 1).contiguous())))


@pytest.mark.parametrize("objective,param,k,off,F", LOSS_CASES)
def test_one_graph_is_the_unsegmented_call_bit_for_bit(objective, param, k, off, F):
    from hgin import LinkSegments
    from hgin.linkpred import link_full_ranks, link_ranks, link_topk, negative_edges
    n_dst = 53
    pos, zs, zd = _inputs(n_dst, F)
    posd, zsd, zdd = pos.to(DEV), zs.to(DEV), zd.to(DEV)
    one = LinkSegments(torch.zeros(N_SRC, dtype=torch.long, device=DEV), torch.zeros(n_dst, dtype=torch.long, device=DEV))
    assert one.n_graphs == 1 and one.dst_ptr.cpu().tolist() == [0, n_dst]
    seg = _run(zsd, zdd, posd, k, off, objective, param, segments=one)
    plain = _run(zsd, zdd, posd, k, off, objective, param)
    assert all(torch.equal(x, y) for x, y in zip(seg, plain))
    if objective != "bce":
        return
    assert torch.equal(negative_edges(posd, n_dst, k, SEED, off, segments=one), negative_edges(posd, n_dst, k, SEED, off))
    for fn, args in ((link_ranks, (zsd, zdd, posd, k, SEED, off)), (link_full_ranks, (zsd, zdd, posd)),
                     (link_full_ranks, (zsd, zdd, posd, posd)), (link_topk, (zsd, zdd, posd[0].contiguous(), 10)),
                     (link_topk, (zsd, zdd, posd[0].contiguous(), 128, posd))):
        assert all(torch.equal(x, y) for x, y in zip(fn(*args, segments=one), fn(*args))), fn.__name__


def test_launch_tags():
    from hgin import _lib
    from hgin.linkpred import link_full_ranks, link_ranks, link_topk, sampled_link_loss
    c = _loss_case("bce", 0.0, 3, 6, 128)
    zsd, zdd, posd, seg = c["zsd"], c["zdd"], c["posd"], c["seg"]
    given = torch.zeros(E, 2, dtype=torch.int32, device=DEV)
    with _lib.trace_launches() as t:
        sampled_link_loss(zsd, zdd, posd, 3, SEED, 6, segments=seg)
        sampled_link_loss(zsd, zdd, posd, 3, SEED, 6, objective="bpr", neg_dst=given, segments=seg)
        link_ranks(zsd, zdd, posd, 3, SEED, 6, segments=seg)
        sampled_link_loss(zsd, zdd, posd, 3, SEED, 6)
        link_full_ranks(zsd, zdd, posd, segments=seg)
        link_topk(zsd, zdd, posd[0].contiguous(), 5, segments=seg)
    assert t.kernels[:6] == ["k_link_fwd<4,32,ONE,LOSS,SEG>", "k_link_loss_sum", "k_link_fwd<4,32,ONE,BPR,GIVEN,SEG>",
                             "k_link_loss_sum", "k_link_fwd<4,32,ONE,RANK,SEG>", "k_link_fwd<4,32,ONE,LOSS>"]
    assert any(k.startswith("k_rank_sweep<4,SEG>") for k in t.kernels) and "k_rank_pairs<4,FILTER,SEG>" in t.kernels
    assert any(k.startswith("k_topk_sweep<4,SEG>") for k in t.kernels)


# ---------------------------------------------------------------------------------------------------
# full ranks and top-K: destination segments (1, 2, 31, 33, 257, 130): tile boundaries (128, 256, 384) inside graphs,
# a graph across two tiles, a one-destination graph (n_cand = 0)
# ---------------------------------------------------------------------------------------------------
RANK_SEGS = (1, 2, 31, 33, 257, 130)
RANK_N_SRC = 300
RANK_FS = (6, 64, 100)
KINDS = ("none", "pos", "superset")
TOPK_KS = (1, 10, 128)


def _make_graphs(segs, n_src, n_pos, order, seed, empty_graphs=0):
    """(pos, src_seg, ptr, n_graphs): sources dealt to the graphs round-robin in a shuffled order (``empty_graphs``
    further graphs own two sources each and no destination), positives spread over every graph with destinations,
    destination uniform inside the graph; ``order`` "sorted" (by graph) or "shuffled"."""
    g = torch.Generator().manual_seed(seed)
    G = len(segs)
    src_seg = (torch.arange(n_src) % G)[torch.randperm(n_src, generator=g)]
    for j in range(empty_graphs):
        src_seg[2 * j:2 * j + 2] = G + j
    ptr = torch.tensor((0,) + tuple(segs) + (0,) * empty_graphs).cumsum(0)
    gs = torch.sort(torch.cat([torch.arange(G), torch.randint(0, G, (n_pos - G,), generator=g)])).values
    by_graph = [torch.nonzero(src_seg == q).flatten() for q in range(G)]
    src = torch.stack([by_graph[int(q)][int(torch.randint(0, len(by_graph[int(q)]), (1,), generator=g))] for q in gs])
    dst = ptr[gs] + (torch.rand(n_pos, generator=g, dtype=torch.float64) * (ptr[gs + 1] - ptr[gs])).long()
    pos = torch.stack([src, dst])
    if order == "shuffled":
        pos = pos[:, torch.randperm(n_pos, generator=g)]
    return pos.contiguous(), src_seg, ptr, G + empty_graphs


def _known(kind, pos, n_src, n_dst, seed):
    """None, the positives, or a superset: the positives + random edges anywhere (most of them leave the source's
    graph) + a block of the positives again (duplicates)."""
    if kind == "none":
        return None
    if kind == "pos":
        return pos
    g = torch.Generator().manual_seed(seed)
    n = 4 * pos.size(1)
    extra = torch.stack([torch.randint(0, n_src, (n,), generator=g), torch.randint(0, n_dst, (n,), generator=g)])
    return torch.cat([pos, extra, pos[:, :50]], 1)[:, torch.randperm(pos.size(1) + n + 50, generator=g)].contiguous()


def _segments(src_seg, ptr, n_graphs):
    from hgin import LinkSegments
    batch_dst = torch.repeat_interleave(torch.arange(n_graphs), ptr[1:] - ptr[:-1])
    seg = LinkSegments(src_seg.to(DEV), batch_dst.to(DEV), n_graphs)
    assert seg.dst_ptr.cpu().tolist() == ptr.tolist()
    return seg


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("F", RANK_FS)
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
def test_full_ranks_exact_on_integer_embeddings(order, F, kind):
    from hgin.linkpred import link_full_ranks
    n_dst = sum(RANK_SEGS)
    pos, src_seg, ptr, G = _make_graphs(RANK_SEGS, RANK_N_SRC, E, order, 31 + F)
    g = torch.Generator().manual_seed(5 + F)
    zs = torch.randint(-2, 3, (RANK_N_SRC, F), generator=g).float()
    zd = torch.randint(-2, 3, (n_dst, F), generator=g).float()
    known = _known(kind, pos, RANK_N_SRC, n_dst, 77)
    seg = _segments(src_seg, ptr, G)
    got = link_full_ranks(zs.to(DEV), zd.to(DEV), pos.to(DEV), None if known is None else known.to(DEV), segments=seg)
    want = ref_seg_full_ranks(zs.numpy(), zd.numpy(), pos.numpy(), None if known is None else known.numpy(),
                              src_seg.numpy(), ptr.numpy())
    for name, a, b in zip(("n_greater", "n_equal", "n_cand"), got, want):
        assert a.dtype == torch.int32 and np.array_equal(a.cpu().numpy().astype(np.int64), b), (name, order, F, kind)
    # the case is a real one: ties, negative thresholds, a query without candidates, and (superset) known edges that
    # leave the graph, which the unsegmented reference would have subtracted
    thr = (zs[pos[0]] * zd[pos[1]]).sum(1)
    assert int(want[1].sum()) > 0 and bool((thr < 0).any()) and int((want[2] == 0).sum()) >= 1
    if kind == "superset":
        gk = src_seg[known[0]]
        cross = (known[1] < ptr[gk]) | (known[1] >= ptr[gk + 1])
        assert int(cross.sum()) > 100
        # subtracting every distinct known neighbour, in the graph or not, would give other candidate counts
        from test_linkrank_host import ref_full_ranks
        anywhere = n_dst - 1 - ref_full_ranks(zs.numpy(), zd.numpy(), pos.numpy(), known.numpy())[2]
        gq = src_seg[pos[0]]
        assert ((ptr[gq + 1] - ptr[gq]).numpy() - 1 - anywhere != want[2]).any()


def _per_graph(known, src_seg, ptr, q):
    """The known edges the unsegmented call on graph q's slice sees: destination inside the graph, shifted."""
    if known is None:
        return None
    lo, hi = int(ptr[q]), int(ptr[q + 1])
    keep = (known[1] >= lo) & (known[1] < hi)
    return torch.stack([known[0][keep], known[1][keep] - lo]).contiguous()


@functools.lru_cache(maxsize=None)
def _float_case(order, F, kind, segs=RANK_SEGS, n_src=RANK_N_SRC, n_pos=E):
    n_dst = sum(segs)
    pos, src_seg, ptr, G = _make_graphs(segs, n_src, n_pos, order, 41 + F, empty_graphs=1)
    g = torch.Generator().manual_seed(9 + F)
    zs = (torch.randn(n_src, F, generator=g) * 0.5).to(DEV)
    zd = (torch.randn(n_dst, F, generator=g) * 0.5).to(DEV)
    known = _known(kind, pos, n_src, n_dst, 78)
    return pos, src_seg, ptr, G, zs, zd, known, _segments(src_seg, ptr, G)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("F", RANK_FS)
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
def test_full_ranks_equal_the_per_graph_calls_bit_for_bit(order, F, kind):
    from hgin.linkpred import link_full_ranks
    pos, src_seg, ptr, G, zs, zd, known, seg = _float_case(order, F, kind)
    got = [t.cpu() for t in link_full_ranks(zs, zd, pos.to(DEV), None if known is None else known.to(DEV),
                                            segments=seg)]
    gq = src_seg[pos[0]]
    for q in range(len(RANK_SEGS)):
        mine = torch.nonzero(gq == q).flatten()
        lo, hi = int(ptr[q]), int(ptr[q + 1])
        kq = _per_graph(known, src_seg, ptr, q)
        sub = torch.stack([pos[0][mine], pos[1][mine] - lo]).contiguous()
        want = link_full_ranks(zs, zd[lo:hi], sub.to(DEV), None if kq is None else kq.to(DEV))
        for name, a, b in zip(("n_greater", "n_equal", "n_cand"), got, want):
            assert torch.equal(a[mine], b.cpu()), (name, q, order, F, kind)


@pytest.mark.parametrize("k", TOPK_KS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("F", RANK_FS)
def test_topk_equals_the_per_graph_calls_bit_for_bit(F, kind, k):
    """Queries: every source row once, in row order (so a block of 128 queries mixes every graph), among them the two
    sources of a graph without destinations, whose rows come back fully padded."""
    from hgin.linkpred import link_topk
    pos, src_seg, ptr, G, zs, zd, known, seg = _float_case("sorted", F, kind)
    src = torch.arange(RANK_N_SRC)
    idx, score = (t.cpu() for t in link_topk(zs, zd, src.to(DEV), k, None if known is None else known.to(DEV),
                                              segments=seg))
    assert idx.dtype == torch.int32 and score.dtype == torch.float32 and tuple(idx.shape) == (RANK_N_SRC, k)
    empty = torch.nonzero(src_seg == G - 1).flatten()
    assert len(empty) == 2 and bool((idx[empty] == -1).all()) and bool((score[empty] == -float("inf")).all())
    for q in range(len(RANK_SEGS)):
        mine = torch.nonzero(src_seg == q).flatten()
        lo, hi = int(ptr[q]), int(ptr[q + 1])
        kq = _per_graph(known, src_seg, ptr, q)
        want_idx, want_score = (t.cpu() for t in link_topk(zs, zd[lo:hi], mine.to(DEV), k,
                                                           None if kq is None else kq.to(DEV)))
        shifted = torch.where(want_idx >= 0, want_idx + lo, want_idx)
        assert torch.equal(idx[mine], shifted), (q, F, kind, k)
        assert torch.equal(score[mine].view(torch.int32), want_score.view(torch.int32)), (q, F, kind, k)
        if hi - lo < k:
            assert bool((idx[mine][:, hi - lo:] == -1).all())     # a small graph pads


BIG_SEGS = (700,) * 8


@pytest.mark.parametrize("order", ["sorted", "shuffled"])
def test_several_workgroups_splits_and_query_blocks(order):
    """8 graphs x 700 destinations (44 tiles, one per split), E = 1000 (8 query blocks), F = 128: sorted queries leave
    most of a block's splits with an empty slice, shuffled ones sweep everything.  Exact on integers, and top-K equal
    to the per-graph calls."""
    from hgin.linkpred import link_full_ranks, link_topk
    n_src, n_pos, F, n_dst = 500, 1000, 128, sum(BIG_SEGS)
    pos, src_seg, ptr, G = _make_graphs(BIG_SEGS, n_src, n_pos, order, 3)
    g = torch.Generator().manual_seed(4)
    zs = torch.randint(-2, 3, (n_src, F), generator=g).float()
    zd = torch.randint(-2, 3, (n_dst, F), generator=g).float()
    known = _known("superset", pos, n_src, n_dst, 79)
    seg = _segments(src_seg, ptr, G)
    zsd, zdd, posd, knownd = zs.to(DEV), zd.to(DEV), pos.to(DEV), known.to(DEV)
    got = link_full_ranks(zsd, zdd, posd, knownd, segments=seg)
    want = ref_seg_full_ranks(zs.numpy(), zd.numpy(), pos.numpy(), known.numpy(), src_seg.numpy(), ptr.numpy())
    for name, a, b in zip(("n_greater", "n_equal", "n_cand"), got, want):
        assert np.array_equal(a.cpu().numpy().astype(np.int64), b), (name, order)
    assert int(want[0].sum()) > 0 and int(want[1].sum()) > 0
    idx, score = (t.cpu() for t in link_topk(zsd, zdd, posd[0].contiguous(), 10, knownd, segments=seg))
    gq = src_seg[pos[0]]
    for q in range(G):
        mine = torch.nonzero(gq == q).flatten()
        lo, hi = int(ptr[q]), int(ptr[q + 1])
        kq = _per_graph(known, src_seg, ptr, q).to(DEV)
        want_idx, want_score = (t.cpu() for t in link_topk(zsd, zdd[lo:hi], pos[0][mine].contiguous().to(DEV), 10, kq))
        assert torch.equal(idx[mine], want_idx + lo) and torch.equal(score[mine], want_score), (q, order)


@pytest.mark.parametrize("F,m", [(6, 5), (64, 40)])
def test_hard_negatives_stay_in_the_graph(F, m):
    import hgin
    from hgin.linkpred import link_topk
    pos, src_seg, ptr, G, zs, zd, known, seg = _float_case("shuffled", F, "superset")
    seed, off = 4242, 2**32 + 3
    posd, knownd = pos.to(DEV), known.to(DEV)
    got = hgin.hard_negatives_seg(zs, zd, posd, m, seg, knownd, seed, off)
    assert got.dtype == torch.int32 and tuple(got.shape) == (E, m) and got.is_contiguous()
    got = got.cpu().numpy().astype(np.int64)
    gq = src_seg[pos[0]].numpy()
    lo, hi = ptr.numpy()[gq][:, None], ptr.numpy()[gq + 1][:, None]
    assert (got >= lo).all() and (got < hi).all()                       # every entry is in-graph
    mined = link_topk(zs, zd, posd[0].contiguous(), m, knownd, segments=seg)[0].cpu().numpy().astype(np.int64)
    pad = mined < 0
    assert pad.any() and (~pad).any()
    assert np.array_equal(got[~pad], mined[~pad])
    is_known = np.zeros((RANK_N_SRC, sum(RANK_SEGS)), dtype=bool)
    is_known[known[0].numpy(), known[1].numpy()] = True
    rows = np.repeat(pos[0].numpy()[:, None], m, 1)
    assert not is_known[rows[~pad], got[~pad]].any()                    # a mined entry is never a known edge
    # a graph of n destinations leaves at most n unknown ones: the small graphs pad, with the segmented stream
    assert pad[gq == 0].all() and pad[gq == 1][:, 2:].all()
    draws = ref_seg_draws(seed, off, pos[0].numpy(), m, src_seg.numpy(), ptr.numpy()).astype(np.int64).reshape(E, m)
    assert np.array_equal(got[pad], draws[pad])


# ---------------------------------------------------------------------------------------------------
# model level: component_graph(cfg1, 4)
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _components():
    import hgin
    from hgin.data import CONFIGS, component_graph
    cfg = CONFIGS["cfg1"]
    g = component_graph(cfg, 4)
    torch.manual_seed(1997)
    ic = {"link": cfg.f_link, "path": cfg.f_path, "node": cfg.f_node}
    model = hgin.HetroGIN(**cfg.model_kwargs(ic)).to(DEV).train()
    return cfg, g.to(DEV), model


def _recording(model):
    recorded, encode = [], model.encode

    def recording_encode(*args, **kw):
        z = encode(*args, **kw)
        recorded.append(z)
        return z

    model.encode = recording_encode
    return recorded, encode


def test_predictor_graph_local_equals_the_direct_calls_and_trains():
    import hgin
    from hgin.linkpred import link_full_metrics, link_metrics, link_topk, sampled_link_loss
    cfg, gd, model = _components()
    pos = gd.edge_index[REL_PL]
    n_e, k, seed = int(pos.size(1)), 3, 7
    seg = hgin.LinkSegments.of(gd, REL_PL)
    assert seg.n_graphs == 4 and seg.dst_ptr.cpu().tolist() == [0, 75, 150, 225, 300]
    recorded, encode = _recording(model)
    try:
        pred = hgin.LinkPredictor(model, REL_PL, k, seed, graph_local=True)
        plain = hgin.LinkPredictor(model, REL_PL, k, seed)
        loss = pred.loss(gd, step=2)
        zs, zd = recorded[-1]["path"].detach(), recorded[-1]["link"].detach()
        assert torch.equal(loss.detach(), sampled_link_loss(zs, zd, pos, k, seed, 2 * n_e * k, segments=seg))
        assert pred._segments[0] is gd and pred.loss(gd, step=3) is not None and pred._segments[0] is gd
        # graph_local = False on the same graph: today's call, bit for bit, and another loss than the graph-local one
        loss_plain = plain.loss(gd, step=2)
        zs, zd = recorded[-1]["path"].detach(), recorded[-1]["link"].detach()
        assert torch.equal(loss_plain.detach(), sampled_link_loss(zs, zd, pos, k, seed, 2 * n_e * k))
        assert not torch.equal(loss_plain.detach(), loss.detach())
        # evaluation and retrieval
        for fn, direct in ((pred.metrics, lambda zs, zd: link_metrics(zs, zd, pos, k, seed, segments=seg)),
                           (pred.full_metrics, lambda zs, zd: link_full_metrics(zs, zd, pos, pos, segments=seg)),
                           (plain.full_metrics, lambda zs, zd: link_full_metrics(zs, zd, pos, pos))):
            got = fn(gd)
            want = direct(recorded[-1]["path"].detach(), recorded[-1]["link"].detach())
            assert sorted(got) == sorted(want) and all(torch.equal(got[key], want[key]) for key in want)
        idx, score = pred.predict(gd, k=5)
        zs, zd = recorded[-1]["path"].detach(), recorded[-1]["link"].detach()
        src = torch.arange(zs.size(0), dtype=torch.long, device=DEV)
        want_idx, want_score = link_topk(zs, zd, src, 5, pos, segments=seg)
        assert torch.equal(idx, want_idx) and torch.equal(score, want_score)
        lo = seg.dst_ptr.long()[seg.src_seg.long()][:, None]
        hi = seg.dst_ptr.long()[seg.src_seg.long() + 1][:, None]
        assert bool(((idx >= lo) & (idx < hi)).all())           # only the source's own graph is proposed
        idx_plain, _ = plain.predict(gd, k=5)
        assert not bool(((idx_plain >= lo) & (idx_plain < hi)).all())
        # three training steps: finite, changing losses
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        losses = [float(hgin.link_train_step(model, opt, gd, pred, step=s)) for s in range(3)]
        assert all(np.isfinite(losses)) and len(set(losses)) == 3
        # mining through the predictor stays in the graph
        hard = hgin.LinkPredictor(model, REL_PL, 1, seed, hard=4, graph_local=True)
        mined = hard.mine(gd).long()
        gq = seg.src_seg.long()[pos[0]]
        assert bool(((mined >= seg.dst_ptr.long()[gq][:, None]) & (mined < seg.dst_ptr.long()[gq + 1][:, None])).all())
    finally:
        model.encode = encode
