"""Top-K link retrieval (A16) on the MI355X against the float64 reference of tests/test_linktopk_host.py: exactly on
integer-valued embeddings (every fp32 product and sum is exact, ties are frequent) in every launch regime of the
sweep, short and empty lists, the extremes of the insertion path, random floats within the rounding bands, the same
score bits as ``link_full_ranks``, determinism and position independence, and ``LinkPredictor.predict``.

Geometry (csrc/hgin_linktopk.hip = the A15 sweep): 128 queries x 128 destinations per workgroup tile, a private list
per (query, split, wave row, lane half), 4 * splits lists merged per query."""
import numpy as np
import pytest
import torch

from test_gpu_linkrank import DEV, N_SRC, REL_PL, _float_inputs, _int_inputs, _superset
from test_gpu_linkrank_sweep import CASES, COPIES, SHAPES, TILE, _cdiv, _plan, _sliced
from test_linktopk_host import ref_topk, topk_candidate_mask

pytestmark = pytest.mark.gpu

KS = (1, 10, 128)


def _run(zs, zd, src, k, known, vec=None):
    """(idx int64 [Q, k], score float32 [Q, k]) as numpy, and the split count the library launched."""
    from hgin import _lib
    from hgin.linkpred import link_topk
    with _lib.trace_launches() as tr:
        idx, score = link_topk(zs.to(DEV) if not zs.is_cuda else zs, zd.to(DEV) if not zd.is_cuda else zd,
                               src.to(DEV), k, None if known is None else known.to(DEV))
    assert idx.dtype == torch.int32 and score.dtype == torch.float32 and idx.is_cuda and score.is_cuda
    assert tuple(idx.shape) == tuple(score.shape) == (src.numel(), k)
    assert not idx.requires_grad and not score.requires_grad
    tags = [t for t in tr.kernels if t.startswith("k_topk_sweep")]
    assert len(tags) == 1 and "splits=" in tags[0], tr.kernels
    if vec is not None:
        assert tags[0].startswith(f"k_topk_sweep<{vec}> splits="), tags
    return idx.cpu().numpy().astype(np.int64), score.cpu().numpy(), int(tags[0].split("splits=")[1])


def _assert_equal(got_idx, got_score, want_idx, want_val, tag):
    bad = np.nonzero((got_idx != want_idx).any(1) | (got_score.astype(np.float64) != want_val).any(1))[0]
    assert bad.size == 0, (tag, bad.size, bad[:3].tolist(), got_idx[bad[:3]].tolist(), want_idx[bad[:3]].tolist(),
                           got_score[bad[:3]].tolist(), want_val[bad[:3]].tolist())


# ---------------------------------------------------------------------------------------------------
# 1. exact, every regime
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["none", "superset"])
@pytest.mark.parametrize("shape,F,sliced", CASES)
def test_exact_in_every_regime(shape, F, sliced, kind):
    """The shapes of tests/test_gpu_linkrank_sweep.py (many splits of 3 tiles with a 9-row last tile; 6 splits of 2
    tiles; one split walking every tile), F = 8 / 64 / 100 through a column window at an odd offset, k = 1, 10, 128.
    One float64 reference at k = 129 serves the three k: a top-k list is a prefix of it, and its entry k tells
    whether a tie straddles the k-th place."""
    Q, n_dst, tps, splits = SHAPES[shape][:4]
    if sliced:
        pos, zs_w, zd_w, g = _int_inputs(Q, n_dst, F + 12, seed=5000 + F + Q)
        zs_d, zd_d, zs, zd = _sliced(zs_w, zd_w, 3, F)
    else:
        pos, zs, zd, g = _int_inputs(Q, n_dst, F, seed=5000 + F + Q)
        zs_d, zd_d = zs, zd
    src = pos[0].contiguous()
    known = None if kind == "none" else _superset(pos, N_SRC, n_dst, g)
    want_idx, want_val = ref_topk(zs.numpy(), zd.numpy(), src.numpy(), max(KS) + 1,
                                  None if known is None else known.numpy())
    plan = _plan(Q, n_dst)
    assert plan[2] == tps >= 2 and plan[3] == splits, plan
    for k in KS:
        got_idx, got_score, launched = _run(zs_d, zd_d, src, k, known, 1 if sliced else 4)
        assert launched == splits, ("the library's split count left the formula", launched, plan)
        _assert_equal(got_idx, got_score, want_idx[:, :k], want_val[:, :k], (shape, F, kind, k))
        straddle = float((want_val[:, k - 1] == want_val[:, k]).mean())
        print(f"{shape} F={F} {kind} k={k}: a tie straddles the k-th place for {straddle:.3f} of the queries")
        # integer scores of standard deviation 2 sqrt(F) <= 20 over at least 300 destinations: neighbours in the
        # sorted list are often closer than one unit, so equal (least often at the very top, where they are sparse)
        assert straddle > 0.05, (shape, F, kind, k, straddle)
    if known is not None:
        mask = topk_candidate_mask(src.numpy(), N_SRC, n_dst, known.numpy())
        assert int((mask.sum(1) < n_dst).sum()) > Q // 2   # the filter removed something for most queries


def test_hand_computed_case():
    from test_linkrank_host import KNOWN, ZD, ZS
    zs, zd, known = torch.tensor(ZS), torch.tensor(ZD), torch.tensor(KNOWN)
    idx, score, _ = _run(zs, zd, torch.tensor([0, 1, 2]), 2, None)
    assert idx.tolist() == [[0, 1], [2, 0], [3, 2]] and score.tolist() == [[2.0, 2.0], [3.0, 1.0], [1.0, 0.0]]
    idx, score, _ = _run(zs, zd, torch.tensor([2, 0, 0, 1]), 6, known)
    assert idx.tolist() == [[3, 0, 1, -1, -1, -1], [0, 1, 2, -1, -1, -1], [0, 1, 2, -1, -1, -1], [-1] * 6]
    ninf = float("-inf")
    assert score.tolist() == [[1.0, -2.0, -2.0] + [ninf] * 3, [2.0, 2.0, 0.0] + [ninf] * 3,
                              [2.0, 2.0, 0.0] + [ninf] * 3, [ninf] * 6]


# ---------------------------------------------------------------------------------------------------
# 2. short lists
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["none", "superset"])
def test_fewer_destinations_than_k(kind):
    pos, zs, zd, g = _int_inputs(211, 5, 8, seed=61)
    known = None if kind == "none" else _superset(pos, N_SRC, 5, g)
    src = pos[0].contiguous()
    got_idx, got_score, _ = _run(zs, zd, src, 10, known)
    want = ref_topk(zs.numpy(), zd.numpy(), src.numpy(), 10, None if known is None else known.numpy())
    _assert_equal(got_idx, got_score, *want, kind)
    assert bool((got_idx[:, 5:] == -1).all()) and bool(np.isneginf(got_score[:, 5:]).all())
    if known is None:
        assert bool((got_idx[:, :5] >= 0).all())
    else:
        assert int((got_idx[:, 4] == -1).sum()) > 100   # every query's own edge is known


@pytest.mark.parametrize("F,sliced", [(8, False), (100, True)])
def test_hub_sources_and_sources_without_known_edges(F, sliced):
    """Sources 290 / 291 know 600 of the 700 destinations (200 of them listed twice), source 292 every destination,
    sources 200 .. 263 none, the rest a few: at k = 128 the hubs return 100 entries and padding, 292 only padding."""
    Q, n_dst, k = 96, 700, 128
    width = F + 12 if sliced else F
    pos, zs_w, zd_w, g = _int_inputs(Q, n_dst, width, seed=78 + F)
    hub_a, hub_b, hub_all = 290, 291, 292
    src = pos[0].clone()
    src[:64] = torch.arange(200, 264)
    src[5], src[17], src[40] = hub_a, hub_b, hub_all
    src[64:] = torch.randint(0, 100, (32,), generator=g)
    src[70], src[71], src[90] = hub_a, hub_all, hub_b
    parts = []
    for hub in (hub_a, hub_b):
        dsts = torch.randperm(n_dst, generator=g)[:600]
        dsts = torch.cat([dsts, dsts[100:300]])
        parts.append(torch.stack([torch.full_like(dsts, hub), dsts]))
    parts.append(torch.stack([torch.full((n_dst,), hub_all), torch.arange(n_dst)]))
    parts.append(torch.stack([torch.randint(0, 100, (400,), generator=g),
                              torch.randint(0, n_dst, (400,), generator=g)]))
    known = torch.cat(parts, 1)[:, torch.randperm(sum(p.size(1) for p in parts), generator=g)]
    if sliced:
        zs_d, zd_d, zs, zd = _sliced(zs_w, zd_w, 3, F)
    else:
        zs_d, zd_d, zs, zd = zs_w, zd_w, zs_w, zd_w
    got_idx, got_score, _ = _run(zs_d, zd_d, src, k, known, 1 if sliced else 4)
    want = ref_topk(zs.numpy(), zd.numpy(), src.numpy(), k, known.numpy())
    _assert_equal(got_idx, got_score, *want, ("hubs", F))
    for q in (40, 71):
        assert bool((got_idx[q] == -1).all()) and bool(np.isneginf(got_score[q]).all())
    for q in (5, 17, 70, 90):
        assert bool((got_idx[q, :100] >= 0).all()) and bool((got_idx[q, 100:] == -1).all())
        assert bool(np.isneginf(got_score[q, 100:]).all())
    idle = [q for q in range(64) if q not in (5, 17, 40)]
    assert bool((got_idx[idle] >= 0).all())
    is_known = set(zip(known[0].tolist(), known[1].tolist()))
    returned = [(int(s), int(c)) for s, row in zip(src.tolist(), got_idx) for c in row if c >= 0]
    assert len(returned) > 64 * k and not any(p in is_known for p in returned)


# ---------------------------------------------------------------------------------------------------
# 3. the extremes of the insertion path
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("order", ["ascending", "descending", "constant"])
def test_insertion_path_extremes(order, k):
    """One-hot query rows (times 1, 2 or 3) against z_dst[:, 0] = the index (every tile brings new maxima: the cold
    path runs and shifts a whole list at every tile), the reverse (nothing is inserted once the lists are full) and a
    constant (all scores tied: indices 0 .. k - 1), over 134 splits of 3 tiles."""
    Q, n_dst, F = 300, 51209, 8
    assert _plan(Q, n_dst)[2:] == (3, 134)
    zs = torch.zeros(N_SRC, F)
    zs[:, 0] = (torch.arange(N_SRC) % 3 + 1).float()
    zd = torch.zeros(n_dst, F)
    c = torch.arange(n_dst).float()
    zd[:, 0] = {"ascending": c, "descending": float(n_dst) - c, "constant": torch.full_like(c, 7.0)}[order]
    zd[:, 1] = 1.0   # times the zeros of z_src
    src = torch.randperm(N_SRC, generator=torch.Generator().manual_seed(3))[:Q]
    got_idx, got_score, launched = _run(zs, zd, src, k, None, 4)
    assert launched == 134
    j = np.arange(k)
    want_idx = np.broadcast_to(n_dst - 1 - j if order == "ascending" else j, (Q, k))
    want_val = zs[src, 0].numpy().astype(np.float64)[:, None] * zd[:, 0].numpy().astype(np.float64)[want_idx]
    _assert_equal(got_idx, got_score, want_idx, want_val, (order, k))


# ---------------------------------------------------------------------------------------------------
# 4. floats against the float64 bands
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("F,sliced", [(64, False), (100, True)])
def test_random_floats_within_the_rounding_bands(F, sliced, filtered):
    """|fp32 score - float64 score| <= b[q, c] = 2 F 2^-24 sum_f |zs zd| for every accumulation order (the bound of
    ref_full_bands).  With B[q] = the largest b of the query's candidates and T[q] = the float64 k-th best score:
    a candidate with score64 - b > T + B must be returned (if it were not, the k returned ones would all have fp32
    scores >= its own, hence float64 scores > T: k + 1 candidates above the k-th best), and a returned candidate has
    score64 + b >= T - B (its fp32 score is at least the k-th largest fp32 score, which is at least T - B)."""
    k, n_dst = 10, 500
    pos, zs_w, zd_w, g = _float_inputs(F + 12 if sliced else F, seed=3024 + F)
    if sliced:
        zs_d, zd_d, zs, zd = _sliced(zs_w, zd_w, 3, F)
    else:
        zs_d, zd_d, zs, zd = zs_w, zd_w, zs_w, zd_w
    src = pos[0].contiguous()
    known = _superset(pos, N_SRC, n_dst, g) if filtered else None
    got_idx, got_score, _ = _run(zs_d, zd_d, src, k, known, 1 if sliced else 4)
    zs64, zd64 = zs.numpy().astype(np.float64), zd.numpy().astype(np.float64)
    s64 = zs64[src.numpy()] @ zd64.T
    b = 2.0 * F * 2.0 ** -24 * (np.abs(zs64[src.numpy()]) @ np.abs(zd64).T)
    mask = topk_candidate_mask(src.numpy(), N_SRC, n_dst, None if known is None else known.numpy())
    assert int(mask.sum(1).min()) > k   # every row is full
    _, want_val = ref_topk(zs64, zd64, src.numpy(), k, None if known is None else known.numpy())
    T = want_val[:, k - 1:k]
    B = np.where(mask, b, 0.0).max(1, keepdims=True)
    rows = np.arange(src.numel())[:, None]
    returned = np.zeros_like(mask)
    assert bool((got_idx >= 0).all()) and bool((got_idx < n_dst).all())
    returned[rows, got_idx] = True
    assert bool((returned.sum(1) == k).all()), "duplicates"
    assert not bool((returned & ~mask).any()), "a known edge was returned"
    must = mask & (s64 - b > T + B)
    assert not bool((must & ~returned).any()), np.nonzero((must & ~returned).any(1))[0][:5].tolist()
    print("clearly inside per query:", float(must.sum(1).mean()), "of", k)
    assert float(must.sum(1).mean()) > k - 2   # informative: the bands leave most of the top k determined
    assert bool((s64[rows, got_idx] + b[rows, got_idx] >= T - B).all())
    assert bool((np.abs(got_score.astype(np.float64) - s64[rows, got_idx]) <= b[rows, got_idx]).all())
    ds, di = np.diff(got_score, axis=1), np.diff(got_idx, axis=1)
    assert bool((ds <= 0).all()) and bool((di[ds == 0] > 0).all())


# ---------------------------------------------------------------------------------------------------
# 5. the same bits as the rank kernels
# ---------------------------------------------------------------------------------------------------
def _full_ranks(zs, zd, pos):
    from hgin.linkpred import link_full_ranks
    return [t.cpu().numpy().astype(np.int64) for t in link_full_ranks(zs.to(DEV), zd.to(DEV), pos.to(DEV))]


def test_consistent_with_link_full_ranks_on_floats():
    """Unfiltered, random floats, k = 10; half of the positives are destinations near the k-th place of their source
    (float64 ranks 0 .. 19), half are random.  n_greater / n_equal of (s, d) decide whether and where d appears; and
    every returned (s, top_idx[q, j]) asked back as a positive must sit at a place the counts allow, which fails if
    top_score were not the threshold the rank kernels compute for that pair."""
    k, n_dst, Q = 10, 1200, 400
    g = torch.Generator().manual_seed(515)
    zs, zd = torch.randn(N_SRC, 64, generator=g) * 0.5, torch.randn(n_dst, 64, generator=g) * 0.5
    src = torch.randint(0, N_SRC, (Q,), generator=g)
    near, _ = ref_topk(zs.numpy(), zd.numpy(), src.numpy(), 20, None)
    d = torch.randint(0, n_dst, (Q,), generator=g)
    d[:Q // 2] = torch.from_numpy(near[np.arange(Q // 2), np.arange(Q // 2) % 20])
    got_idx, got_score, _ = _run(zs, zd, src, k, None, 4)
    n_gt, n_eq, _ = _full_ranks(zs, zd, torch.stack([src, d]))
    where = [np.nonzero(row == int(c))[0] for row, c in zip(got_idx, d)]
    present = np.array([w.size > 0 for w in where])
    assert bool(present[n_gt + n_eq < k].all()) and not bool(present[n_gt >= k].any())
    assert 50 < int(present.sum()) < Q - 50
    p = np.array([w[0] if w.size else -1 for w in where])
    assert bool(((n_gt <= p) & (p <= n_gt + n_eq))[present].all())
    back = torch.stack([src.repeat_interleave(k), torch.from_numpy(got_idx.reshape(-1))])
    b_gt, b_eq, _ = _full_ranks(zs, zd, back)
    place = np.tile(np.arange(k), Q)
    assert bool(((b_gt <= place) & (place <= b_gt + b_eq)).all())


def test_copies_of_a_row_come_out_together_with_equal_bits():
    """Eight copies of destination row 600 in eight other tiles; row 600 is 3 z_src[s0], far above every other score of
    s0: the nine equal rows lead s0's list in index order with bit-equal scores, whichever workgroup scored them."""
    n_dst, k = 1200, 10
    g = torch.Generator().manual_seed(516)
    zs, zd = torch.randn(N_SRC, 64, generator=g) * 0.5, torch.randn(n_dst, 64, generator=g) * 0.5
    s0 = 17
    zd[600] = 3.0 * zs[s0]
    zd[COPIES] = zd[600].clone()
    nine = sorted(COPIES + [600])
    for Q in (40, 65500):   # ten splits of one tile; one split walking the ten tiles
        src = torch.randint(0, N_SRC, (Q,), generator=g)
        src[0] = src[Q - 1] = s0
        got_idx, got_score, launched = _run(zs, zd, src, k, None, 4)
        assert launched == _plan(Q, n_dst)[3] == (10 if Q == 40 else 1)
        for q in (0, Q - 1):
            assert got_idx[q, :9].tolist() == nine
            assert np.unique(got_score[q, :9].view(np.int32)).size == 1 and got_score[q, 9] < got_score[q, 8]
    n_gt, n_eq, _ = _full_ranks(zs, zd, torch.tensor([[s0], [600]]))
    assert n_gt[0] == 0 and n_eq[0] == 8


# ---------------------------------------------------------------------------------------------------
# 6. determinism and position independence
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filtered", [False, True])
def test_repeatable_and_independent_of_the_query_position(filtered):
    Q, n_dst, k = 65500, 1200, 10
    g = torch.Generator().manual_seed(97)
    zs, zd = torch.randn(N_SRC, 64, generator=g) * 0.5, torch.randn(n_dst, 64, generator=g) * 0.5
    src = torch.randint(0, N_SRC, (Q,), generator=g)
    src[40000] = src[0]   # the same source again, in query block 312
    assert 40000 // TILE == 312
    known = None
    if filtered:
        known = torch.stack([torch.randint(0, N_SRC, (30000,), generator=g),
                             torch.randint(0, n_dst, (30000,), generator=g)])
    a_idx, a_score, _ = _run(zs, zd, src, k, known, 4)
    b_idx, b_score, _ = _run(zs, zd, src, k, known, 4)
    assert np.array_equal(a_idx, b_idx) and np.array_equal(a_score.view(np.int32), b_score.view(np.int32))
    assert np.array_equal(a_idx[0], a_idx[40000])
    assert np.array_equal(a_score[0].view(np.int32), a_score[40000].view(np.int32))
    perm = torch.randperm(Q, generator=g)
    p_idx, p_score, _ = _run(zs, zd, src[perm], k, known, 4)
    assert np.array_equal(p_idx, a_idx[perm.numpy()])
    assert np.array_equal(p_score.view(np.int32), a_score[perm.numpy()].view(np.int32))
    # few queries, many splits: the same rows again (the result does not depend on how the destinations are split)
    f_idx, f_score, launched = _run(zs, zd, src[:300], k, known, 4)
    assert launched == _cdiv(n_dst, TILE)
    assert np.array_equal(f_idx, a_idx[:300]) and np.array_equal(f_score.view(np.int32), a_score[:300].view(np.int32))


def test_src_out_of_range_is_an_index_error():
    from hgin.linkpred import link_topk
    z = torch.zeros(5, 8, device=DEV)
    for bad in (-1, 5):
        with pytest.raises(IndexError, match="src index out of range"):
            link_topk(z, z, torch.tensor([0, bad, 1], device=DEV), 2)


# ---------------------------------------------------------------------------------------------------
# 7. model level (cfg1 synthetic graph)
# ---------------------------------------------------------------------------------------------------
def test_link_predictor_predict():
    import hgin
    from hgin.data import CONFIGS, synthetic_graph
    from hgin.linkpred import link_topk
    cfg = CONFIGS["cfg1"]
    g = synthetic_graph(cfg, seed=0)
    torch.manual_seed(1997)
    model = hgin.HetroGIN(**cfg.model_kwargs({"link": cfg.f_link, "path": cfg.f_path, "node": cfg.f_node}))
    model = model.to(DEV).train()
    gd = g.to(DEV)
    pred = hgin.LinkPredictor(model, REL_PL, 3, 7)
    idx, score = pred.predict(gd)
    assert model.training                      # restored
    assert tuple(idx.shape) == tuple(score.shape) == (cfg.n_path, 10)
    assert not idx.requires_grad and not score.requires_grad and score.grad_fn is None
    model.eval()
    idx_eval, score_eval = pred.predict(gd)
    assert not model.training
    assert torch.equal(idx, idx_eval) and torch.equal(score, score_eval)

    with torch.no_grad():
        z = model.encode(gd.x_dict(), gd.edge_index_dict())
    edges = gd.edge_index[REL_PL]
    every = torch.arange(cfg.n_path, device=DEV)
    same_idx, same_score = link_topk(z["path"], z["link"], every, 10, edges)
    assert torch.equal(idx, same_idx) and torch.equal(score, same_score)
    existing = set(zip(edges[0].tolist(), edges[1].tolist()))
    proposed = [(s, int(c)) for s, row in enumerate(idx.cpu().tolist()) for c in row if c >= 0]
    assert len(proposed) == cfg.n_path * 10 and not any(p in existing for p in proposed)
    # the unfiltered call does propose existing edges here, so the default filter did something
    unf_idx, _ = link_topk(z["path"], z["link"], every, 10)
    assert any((s, int(c)) in existing for s, row in enumerate(unf_idx.cpu().tolist()) for c in row)

    some = torch.tensor([5, 0, 5, 17], device=DEV)
    sub_idx, sub_score = pred.predict(gd, src=some, k=4, known=edges[:, :100])
    want_idx, want_score = link_topk(z["path"], z["link"], some, 4, edges[:, :100])
    assert torch.equal(sub_idx, want_idx) and torch.equal(sub_score, want_score)
    assert torch.equal(sub_idx[0], sub_idx[2])
