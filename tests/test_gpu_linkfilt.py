"""Sampled negatives drawn from each source's non-neighbours on the GPU (include/hgin.h A20, ``known=``).

Shapes, positives, embeddings and the case grid are tests/test_gpu_linkseg.py's (destination segments (1, 5, 53, 200),
k in (1, 3, 5), offsets (6, 2^32 + 1), F in (6, 128, 260), four objectives); the known set is built here so that a
source without a free destination, a source whose in-window row is empty, a row of more than 64 in-window columns and
rows with columns on both sides of the window all occur (asserted).  Draws: bit for bit tests/test_linkfilt_host.py's
numpy restatement, in the fused forward's saved pairs and in ``negative_edges(known=)``, segmented and as one pool.
Anchors, bitwise: (k, known) equals the A18 call that is given the reference draws (also with two more given negatives
behind them, and for the ranks), an empty known set equals the call without one, a second run repeats the first.
Values: against the float64 references on the reference draws and against the unfused ``link_loss(known=)``, within
tests/test_gpu_linkpred.py::_check's bounds (imported, not re-chosen)."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_linkpred import E, N_SRC, REL_PL, SEED, _check, _inputs
from test_gpu_linkseg import LOSS_CASES, LOSS_SEGS, _loss_inputs, _obj_kw, _run
from test_linkfilt_host import known_csr_np, ref_filt_draws
from test_linkobj_host import ref_obj_loss_and_grads
from test_linkpred_host import ref_loss_and_grads
from test_linkseg_host import ref_seg_draws

DEV = "cuda"
pytestmark = pytest.mark.gpu
N_DST = sum(LOSS_SEGS)
DRAW_CASES = sorted({(k, off, F) for _, _, k, off, F in LOSS_CASES})


@functools.lru_cache(maxsize=None)
def _known(F):
    """(known int64 [2, M] on the host, rowptr, col, info): the positives of ``_loss_inputs(F)`` without those of one
    source, plus edges chosen so that the four kinds of row the filter has to handle all occur (asserted here)."""
    pos, _, _, src_seg, ptr, _ = _loss_inputs(F)
    owners = [[s for s in sorted(set(pos[0].tolist())) if src_seg[s] == g] for g in range(4)]
    assert all(len(o) >= 2 for o in owners)
    full, bare, both = owners[1][0], owners[2][0], owners[2][1]
    hub = owners[3][0]
    lo2, hi2, lo3 = int(ptr[2]), int(ptr[3]), int(ptr[3])
    keep = pos[0] != bare                                       # bare's own positives are not known ...
    extra = [(full, int(ptr[1]) + j) for j in range(5)]         # every destination of the second graph
    extra += [(bare, 0), (bare, 3), (bare, lo3 + 7)]            # ... and its known edges all leave its graph
    extra += [(both, 0), (both, 2), (both, hi2), (both, N_DST - 1)]   # columns below and above its window [6, 59)
    extra += [(hub, lo3 + 2 * j) for j in range(100)] + [(hub, 1), (hub, lo2 + 4)]   # > 64 in-window columns
    known = torch.cat([pos[:, keep], torch.tensor(extra).t()], 1)
    known = known[:, torch.randperm(known.size(1), generator=torch.Generator().manual_seed(F))].contiguous()
    rowptr, col = known_csr_np(known.numpy(), N_SRC, N_DST)

    def in_window(s):
        row = col[rowptr[s]:rowptr[s + 1]]
        g = src_seg[s]
        return row, row[(row >= ptr[g]) & (row < ptr[g + 1])]

    free = {s: int(ptr[src_seg[s] + 1] - ptr[src_seg[s]]) - len(in_window(s)[1]) for s in set(pos[0].tolist())}
    no_free = sorted(s for s, f in free.items() if f == 0)
    assert full in no_free and any(src_seg[s] == 0 for s in no_free)        # both kinds of f == 0
    assert len(in_window(bare)[0]) == 3 and len(in_window(bare)[1]) == 0    # an empty in-window row
    assert len(in_window(hub)[1]) > 64                                      # past one lane-staged group
    row, inside = in_window(both)
    assert (row < lo2).any() and (row >= hi2).any() and 0 < len(inside) < len(row)   # the clip has work on both sides
    assert any(f > 0 for f in free.values())
    return known, rowptr, col, dict(no_free=no_free, bare=bare, hub=hub)


def _known_mask(F):
    known = _known(F)[0]
    mask = np.zeros((N_SRC, N_DST), dtype=bool)
    mask[known[0].numpy(), known[1].numpy()] = True
    return mask


@functools.lru_cache(maxsize=None)
def _draws(k, off, F, segmented=True):
    pos, _, _, src_seg, ptr, _ = _loss_inputs(F)
    _, rowptr, col, _ = _known(F)
    if segmented:
        return ref_filt_draws(SEED, off, pos[0].numpy(), k, src_seg, ptr, rowptr, col)
    return ref_filt_draws(SEED, off, pos[0].numpy(), k, None, [0, N_DST], rowptr, col)


@functools.lru_cache(maxsize=None)
def _case(objective, param, k, off, F):
    pos, zs, zd, src_seg, ptr, seg = _loss_inputs(F)
    posd, zsd, zdd, knownd = pos.to(DEV), zs.to(DEV), zd.to(DEV), _known(F)[0].to(DEV)
    loss, g_src, g_dst, neg = _run(zsd, zdd, posd, k, off, objective, param, segments=seg, known=knownd)
    want = _draws(k, off, F)
    if objective == "bce":
        ref = ref_loss_and_grads(zs, zd, pos, want, k)
    else:
        ref = ref_obj_loss_and_grads(zs, zd, pos, want, k, objective, param)
    return dict(pos=pos, posd=posd, zs=zs, zd=zd, zsd=zsd, zdd=zdd, seg=seg, knownd=knownd, loss=loss, g_src=g_src,
                g_dst=g_dst, neg=neg, want=want, ref=ref, src_seg=src_seg, ptr=ptr)


@pytest.mark.parametrize("objective,param,k,off,F", LOSS_CASES)
def test_segmented_draws_are_the_reference_and_never_a_known_edge(objective, param, k, off, F):
    from hgin.linkpred import negative_edges
    c = _case(objective, param, k, off, F)
    neg = c["neg"].cpu()
    assert neg.dtype == torch.int64 and tuple(neg.shape) == (2, E * k)
    assert np.array_equal(neg[1].numpy(), c["want"].astype(np.int64))
    assert torch.equal(neg[0], c["pos"][0].repeat_interleave(k))
    if objective == "bce":   # the unfused sampler has no objective
        got = negative_edges(c["posd"], N_DST, k, SEED, off, segments=c["seg"], known=c["knownd"])
        assert torch.equal(got.cpu(), neg)
    s, d = neg[0].numpy(), neg[1].numpy()
    g = c["src_seg"][s]
    assert (d >= c["ptr"][g]).all() and (d < c["ptr"][g + 1]).all()          # draws stay in the source's graph
    is_known = _known_mask(F)[s, d]
    no_free = np.isin(s, _known(F)[3]["no_free"])
    assert no_free.any() and is_known[no_free].all()       # a window of neighbours only: the unfiltered draw
    assert (~no_free).any() and not is_known[~no_free].any()
    # the filter did something: the unfiltered draws of the same counters hit known edges of sources that have a choice
    plain = ref_seg_draws(SEED, off, c["pos"][0].numpy(), k, c["src_seg"], c["ptr"])
    assert _known_mask(F)[s, plain][~no_free].any()


@pytest.mark.parametrize("k,off,F", DRAW_CASES)
def test_one_pool_draws_are_the_reference_and_never_a_known_edge(k, off, F):
    from hgin.linkpred import negative_edges
    c = _case("bce", 0.0, k, off, F)
    want = _draws(k, off, F, segmented=False).astype(np.int64)
    neg = _run(c["zsd"], c["zdd"], c["posd"], k, off, known=c["knownd"])[3].cpu()
    assert np.array_equal(neg[1].numpy(), want) and torch.equal(neg[0], c["pos"][0].repeat_interleave(k))
    assert torch.equal(negative_edges(c["posd"], N_DST, k, SEED, off, known=c["knownd"]).cpu(), neg)
    assert not _known_mask(F)[neg[0].numpy(), want].any()      # 259 destinations: every source has a free one
    assert not np.array_equal(want, c["want"].astype(np.int64))


@pytest.mark.parametrize("objective,param,k,off,F", LOSS_CASES)
def test_loss_and_gradients_vs_float64_reference_and_link_loss(objective, param, k, off, F):
    from hgin.linkpred import link_loss
    c = _case(objective, param, k, off, F)
    assert c["loss"].dim() == 0 and c["loss"].dtype == torch.float32
    _check(c["loss"], c["g_src"], c["g_dst"], c["ref"], f"filtered {objective} vs float64")
    a, b = c["zsd"].clone().requires_grad_(True), c["zdd"].clone().requires_grad_(True)
    base = link_loss(a, b, c["posd"], k, SEED, off, segments=c["seg"], known=c["knownd"], **_obj_kw(objective, param))
    base.backward()
    _check(c["loss"], c["g_src"], c["g_dst"], (base.detach().cpu(), a.grad.cpu(), b.grad.cpu()),
           f"filtered {objective} vs link_loss")


@pytest.mark.parametrize("objective,param,k,off,F", LOSS_CASES)
def test_the_a18_anchor_and_determinism_are_bitwise(objective, param, k, off, F):
    """A filtered draw carries the bits the same destination carries as a given negative (A18): (k, known) equals
    (0, neg_dst = the reference draws), also with m = 2 extra given negatives behind the draws (which are not
    filtered: they are known edges here); and a second run repeats the first."""
    from hgin.linkpred import link_ranks
    c = _case(objective, param, k, off, F)
    zsd, zdd, posd, seg, knownd = c["zsd"], c["zdd"], c["posd"], c["seg"], c["knownd"]
    again = _run(zsd, zdd, posd, k, off, objective, param, segments=seg, known=knownd)
    draws = torch.as_tensor(c["want"].astype(np.int32)).view(E, k).to(DEV)
    given = _run(zsd, zdd, posd, 0, off, objective, param, neg_dst=draws)
    for got in (again, given):
        assert torch.equal(got[0], c["loss"]) and torch.equal(got[1], c["g_src"]) and torch.equal(got[2], c["g_dst"])
        assert torch.equal(got[3], c["neg"])
    extra = torch.stack([posd[1], posd[1].flip(0)], 1).to(torch.int32).contiguous()   # m = 2: the positive itself, another's
    both = _run(zsd, zdd, posd, k, off, objective, param, neg_dst=extra, segments=seg, known=knownd)
    flat = _run(zsd, zdd, posd, 0, off, objective, param, neg_dst=torch.cat([draws, extra], 1).contiguous())
    assert all(torch.equal(x, y) for x, y in zip(both, flat))
    if objective == "bce":   # the ranks have no objective
        assert all(torch.equal(x, y) for x, y in zip(link_ranks(zsd, zdd, posd, k, SEED, off, segments=seg, known=knownd),
                                                     link_ranks(zsd, zdd, posd, 0, SEED, off, neg_dst=draws)))
        assert all(torch.equal(x, y) for x, y in zip(
            link_ranks(zsd, zdd, posd, k, SEED, off, neg_dst=extra, segments=seg, known=knownd),
            link_ranks(zsd, zdd, posd, 0, SEED, off, neg_dst=torch.cat([draws, extra], 1).contiguous())))
        # one pool
        pool = torch.as_tensor(_draws(k, off, F, segmented=False).astype(np.int32)).view(E, k).to(DEV)
        assert all(torch.equal(x, y) for x, y in zip(_run(zsd, zdd, posd, k, off, known=knownd),
                                                     _run(zsd, zdd, posd, 0, off, neg_dst=pool)))
        assert all(torch.equal(x, y) for x, y in zip(link_ranks(zsd, zdd, posd, k, SEED, off, known=knownd),
                                                     link_ranks(zsd, zdd, posd, 0, SEED, off, neg_dst=pool)))


@pytest.mark.parametrize("objective,param,k,off,F", LOSS_CASES)
def test_an_empty_known_set_is_the_call_without_one_bit_for_bit(objective, param, k, off, F):
    from hgin.linkpred import link_metrics, link_ranks, negative_edges
    c = _case(objective, param, k, off, F)
    zsd, zdd, posd, seg = c["zsd"], c["zdd"], c["posd"], c["seg"]
    empty = torch.zeros(2, 0, dtype=torch.long, device=DEV)
    for kw in ({"segments": seg}, {}):
        with_empty = _run(zsd, zdd, posd, k, off, objective, param, known=empty, **kw)
        without = _run(zsd, zdd, posd, k, off, objective, param, **kw)
        assert all(torch.equal(x, y) for x, y in zip(with_empty, without)), kw
        if objective != "bce":
            continue
        assert all(torch.equal(x, y) for x, y in zip(link_ranks(zsd, zdd, posd, k, SEED, off, known=empty, **kw),
                                                     link_ranks(zsd, zdd, posd, k, SEED, off, **kw)))
        assert torch.equal(negative_edges(posd, N_DST, k, SEED, off, known=empty, **kw),
                           negative_edges(posd, N_DST, k, SEED, off, **kw))
        a, b = link_metrics(zsd, zdd, posd, k, SEED, off, known=empty, **kw), link_metrics(zsd, zdd, posd, k, SEED, off, **kw)
        assert sorted(a) == sorted(b) and all(torch.equal(a[key], b[key]) for key in b)
    # and the filtered metrics are the filtered ranks'
    if objective == "bce":
        from hgin.linkpred import metrics_from_ranks
        got = link_metrics(zsd, zdd, posd, k, SEED, off, segments=seg, known=c["knownd"])
        want = metrics_from_ranks(*link_ranks(zsd, zdd, posd, k, SEED, off, segments=seg, known=c["knownd"]), k)
        assert all(torch.equal(got[key], want[key]) for key in want)


def test_plain_inputs_without_segments_keep_todays_bits_with_an_empty_known_set():
    """tests/test_gpu_linkpred.py's own inputs (one pool of 53 destinations): known = [2, 0] changes nothing."""
    pos, zs, zd = _inputs(53, 128)
    posd, zsd, zdd = pos.to(DEV), zs.to(DEV), zd.to(DEV)
    empty = torch.zeros(2, 0, dtype=torch.long, device=DEV)
    assert all(torch.equal(x, y) for x, y in zip(_run(zsd, zdd, posd, 3, 6, known=empty), _run(zsd, zdd, posd, 3, 6)))


def test_past_one_pass_of_the_persistent_grid_with_the_widest_group():
    """F = 260 (the looped form, one positive per wave), k = 3, E = 20,000 positives > 4096 workgroups x 4 waves: a wave
    takes a second positive and must start it from a fresh row state.  Draws bit-equal to the reference."""
    from hgin.linkpred import sampled_link_loss
    F, k, off, n_pos = 260, 3, 6, 20_000
    _, zs, zd, src_seg, ptr, seg = _loss_inputs(F)
    known, rowptr, col, _ = _known(F)
    g = torch.Generator().manual_seed(20)
    src = torch.randint(0, 30, (n_pos,), generator=g)
    gs = torch.as_tensor(src_seg)[src]
    tptr = torch.as_tensor(ptr)
    dst = tptr[gs] + (torch.rand(n_pos, generator=g, dtype=torch.float64) * (tptr[gs + 1] - tptr[gs])).long()
    pos = torch.stack([src, dst])
    assert n_pos > 4096 * 4
    a, b = zs.to(DEV).requires_grad_(True), zd.to(DEV).requires_grad_(True)
    loss = sampled_link_loss(a, b, pos.to(DEV), k, SEED, off, segments=seg, known=known.to(DEV))
    neg = loss.grad_fn.saved_tensors[1].cpu()
    want = ref_filt_draws(SEED, off, src.numpy(), k, src_seg, ptr, rowptr, col)
    assert np.array_equal(neg[1].numpy(), want.astype(np.int64)) and torch.equal(neg[0], src.repeat_interleave(k))
    assert bool(torch.isfinite(loss))


def test_launch_tags():
    from hgin import _lib
    from hgin.linkpred import link_ranks, negative_edges, sampled_link_loss
    c = _case("bce", 0.0, 3, 6, 128)
    zsd, zdd, posd, seg, knownd = c["zsd"], c["zdd"], c["posd"], c["seg"], c["knownd"]
    given = torch.zeros(E, 2, dtype=torch.int32, device=DEV)
    with _lib.trace_launches() as t:
        sampled_link_loss(zsd, zdd, posd, 3, SEED, 6, segments=seg, known=knownd)
        sampled_link_loss(zsd, zdd, posd, 3, SEED, 6, objective="bpr", neg_dst=given, known=knownd)
        link_ranks(zsd, zdd, posd, 3, SEED, 6, known=knownd)
        sampled_link_loss(zsd, zdd, posd, 3, SEED, 6, segments=seg)
        sampled_link_loss(zsd, zdd, posd, 3, SEED, 6, neg_dst=given)
        sampled_link_loss(zsd, zdd, posd, 3, SEED, 6)
        link_ranks(zsd, zdd, posd, 3, SEED, 6)
        negative_edges(posd, N_DST, 3, SEED, 6, known=knownd)
    assert t.kernels == ["k_link_fwd<4,32,ONE,LOSS,SEG,FILT>", "k_link_loss_sum", "k_link_fwd<4,32,ONE,BPR,GIVEN,FILT>",
                         "k_link_loss_sum", "k_link_fwd<4,32,ONE,RANK,FILT>", "k_link_fwd<4,32,ONE,LOSS,SEG>",
                         "k_link_loss_sum", "k_link_fwd<4,32,ONE,LOSS,GIVEN>", "k_link_loss_sum",
                         "k_link_fwd<4,32,ONE,LOSS>", "k_link_loss_sum", "k_link_fwd<4,32,ONE,RANK>",
                         "k_neg_sample_filt"]


# ---------------------------------------------------------------------------------------------------
# model level: component_graph(cfg1, 4)
# ---------------------------------------------------------------------------------------------------
def test_predictor_filter_negatives_equals_the_direct_calls_and_trains():
    import hgin
    from hgin.data import CONFIGS, component_graph
    from hgin.linkpred import link_metrics, sampled_link_loss
    cfg = CONFIGS["cfg1"]
    gd = component_graph(cfg, 4).to(DEV)
    torch.manual_seed(1997)
    ic = {"link": cfg.f_link, "path": cfg.f_path, "node": cfg.f_node}
    model = hgin.HetroGIN(**cfg.model_kwargs(ic)).to(DEV).train()
    pos = gd.edge_index[REL_PL]
    n_e, k, seed = int(pos.size(1)), 3, 7
    seg = hgin.LinkSegments.of(gd, REL_PL)
    recorded, encode = [], model.encode

    def recording_encode(*args, **kw):
        z = encode(*args, **kw)
        recorded.append(z)
        return z

    model.encode = recording_encode
    try:
        pred = hgin.LinkPredictor(model, REL_PL, k, seed, graph_local=True, filter_negatives=True)
        unfiltered = hgin.LinkPredictor(model, REL_PL, k, seed, graph_local=True)
        loss = pred.loss(gd, step=2)
        zs, zd = recorded[-1]["path"].detach(), recorded[-1]["link"].detach()
        direct = sampled_link_loss(zs, zd, pos, k, seed, 2 * n_e * k, segments=seg, known=pos)
        assert torch.equal(loss.detach(), direct)
        assert not torch.equal(loss.detach(), unfiltered.loss(gd, step=2).detach())
        # no negative of the filtered step is an edge of the relation; the unfiltered step's draws hit some
        keys = pos[0] * seg.n_dst + pos[1]
        a, b = zs.clone().requires_grad_(True), zd.clone().requires_grad_(True)
        l_filt = sampled_link_loss(a, b, pos, k, seed, 2 * n_e * k, segments=seg, known=pos)
        l_plain = sampled_link_loss(a, b, pos, k, seed, 2 * n_e * k, segments=seg)
        neg, plain = l_filt.grad_fn.saved_tensors[1], l_plain.grad_fn.saved_tensors[1]
        assert not bool(torch.isin(neg[0] * seg.n_dst + neg[1], keys).any())
        assert bool(torch.isin(plain[0] * seg.n_dst + plain[1], keys).any())
        got = pred.metrics(gd)
        want = link_metrics(recorded[-1]["path"].detach(), recorded[-1]["link"].detach(), pos, k, seed, segments=seg,
                            known=pos)
        assert sorted(got) == sorted(want) and all(torch.equal(got[key], want[key]) for key in want)
        # a few training steps lower the loss of a fixed draw (step 0's negatives, before and after)
        before = float(pred.loss(gd, step=0))
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        losses = [float(hgin.link_train_step(model, opt, gd, pred, step=s)) for s in range(1, 6)]
        after = float(pred.loss(gd, step=0))
        print(f"filtered link steps: before {before:.6f}, steps {losses}, after {after:.6f}")
        assert all(np.isfinite(losses)) and after < before
    finally:
        model.encode = encode
