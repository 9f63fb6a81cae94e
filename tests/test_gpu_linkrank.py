"""Full-candidate filtered link ranking (A15) on the MI355X: the three counts against the float64 reference of
tests/test_linkrank_host.py — exactly on integer-valued embeddings (every fp32 product and sum is exact), within the
rounding band on random floats —, repeatability, and LinkPredictor.full_metrics on a small synthetic graph.

Tile geometry the shapes are chosen around (csrc/hgin_linkrank.hip): 128 queries x 128 destinations per workgroup
tile, 32 x 32 MFMA blocks, 32 features per LDS stage, 8 features per K block, 16-byte loads only when F, the strides
and the bases allow them."""
import numpy as np
import pytest
import torch

from test_linkrank_host import ref_full_bands, ref_full_metrics, ref_full_ranks

DEV = "cuda"
pytestmark = pytest.mark.gpu

N_SRC = 300
REL_PL = ("path", "uses", "link")


def _int_inputs(E, n_dst, F, seed, n_src=N_SRC):
    g = torch.Generator().manual_seed(seed)
    pos = torch.stack([torch.randint(0, n_src, (E,), generator=g), torch.randint(0, n_dst, (E,), generator=g)])
    zs = torch.randint(-2, 3, (n_src, F), generator=g).float()
    zd = torch.randint(-2, 3, (n_dst, F), generator=g).float()
    return pos, zs, zd, g


def _superset(pos, n_src, n_dst, g):
    """pos + its first half again + random extra edges (most from sources no query uses, some repeated)."""
    extra = torch.stack([torch.randint(0, n_src, (150,), generator=g), torch.randint(0, n_dst, (150,), generator=g)])
    return torch.cat([pos, pos[:, : max(1, pos.size(1) // 2)], extra, extra[:, :40]], 1)


def _known(kind, pos, n_src, n_dst, g):
    return None if kind == "none" else (pos.clone() if kind == "pos" else _superset(pos, n_src, n_dst, g))


def _run(zs, zd, pos, known):
    from hgin.linkpred import link_full_ranks
    out = link_full_ranks(zs.to(DEV) if not zs.is_cuda else zs, zd.to(DEV) if not zd.is_cuda else zd, pos.to(DEV),
                          None if known is None else known.to(DEV))
    assert all(t.dtype == torch.int32 and t.is_cuda and tuple(t.shape) == (pos.size(1),) for t in out)
    return [t.cpu().numpy().astype(np.int64) for t in out]


def _assert_exact(got, zs, zd, pos, known, tag):
    want = ref_full_ranks(zs.numpy(), zd.numpy(), pos.numpy(), None if known is None else known.numpy())
    for name, a, b in zip(("n_greater", "n_equal", "n_cand"), got, want):
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, (tag, name, bad[:5].tolist(), a[bad[:5]].tolist(), b[bad[:5]].tolist())


@pytest.mark.parametrize("kind", ["none", "pos", "superset"])
@pytest.mark.parametrize("F", [1, 6, 8, 64, 100, 128, 260, 520])
def test_exact_grid(F, kind):
    ties = negative = 0
    for n_dst in (1, 2, 31, 33, 257):
        for E in (1, 33, 211):
            pos, zs, zd, g = _int_inputs(E, n_dst, F, seed=1000 * F + 10 * n_dst + E)
            known = _known(kind, pos, N_SRC, n_dst, g)
            got = _run(zs, zd, pos, known)
            _assert_exact(got, zs, zd, pos, known, (n_dst, E, F, kind))
            if n_dst == 1:
                assert not got[0].any() and not got[1].any() and not got[2].any()
            ties += int(got[1].sum())
            negative += int(((zs[pos[0]] * zd[pos[1]]).sum(1) < 0).sum())
    assert ties > 0 and negative > 0   # the grid does exercise ties and negative thresholds


def test_hand_computed_case():
    """A duplicate destination row, negative thresholds, a duplicated known edge, a source connected to everything."""
    from test_linkrank_host import KNOWN, POS, ZD, ZS
    zs, zd, pos, known = torch.tensor(ZS), torch.tensor(ZD), torch.tensor(POS), torch.tensor(KNOWN)
    gt, eq, nc = _run(zs, zd, pos, None)
    assert gt.tolist() == [0, 3, 2, 0] and eq.tolist() == [1, 0, 1, 0] and nc.tolist() == [3, 3, 3, 3]
    gt, eq, nc = _run(zs, zd, pos, known)
    assert gt.tolist() == [0, 0, 1, 0] and eq.tolist() == [1, 0, 1, 0] and nc.tolist() == [2, 0, 2, 0]


@pytest.mark.parametrize("kind", ["none", "superset"])
def test_exact_several_workgroups_and_query_blocks(kind):
    pos, zs, zd, g = _int_inputs(1000, 5000, 128, seed=7)
    known = _known(kind, pos, N_SRC, 5000, g)
    _assert_exact(_run(zs, zd, pos, known), zs, zd, pos, known, kind)


@pytest.mark.parametrize("offset,F", [(4, 64), (3, 64), (4, 30), (1, 129)])
def test_exact_on_column_slices_of_wider_tensors(offset, F):
    """Row strides larger than F; offset 4 keeps the rows 16-byte aligned (the vector loads where F % 4 == 0), the
    others do not."""
    from hgin import _lib
    pos, zs_w, zd_w, g = _int_inputs(211, 257, F + 12, seed=31 + offset + F)
    zs_d, zd_d = zs_w.to(DEV)[:, offset:offset + F], zd_w.to(DEV)[:, offset:offset + F]
    assert zs_d.stride(0) == F + 12 and not zs_d.is_contiguous()
    zs, zd = zs_w[:, offset:offset + F].contiguous(), zd_w[:, offset:offset + F].contiguous()
    known = _superset(pos, N_SRC, 257, g)
    with _lib.trace_launches() as tr:
        got = _run(zs_d, zd_d, pos, known)
    vec = 4 if (offset % 4 == 0 and F % 4 == 0) else 1
    assert [t.split(" ")[0] for t in tr.kernels if t.startswith("k_rank")] == [
        f"k_rank_pairs<{vec},THR>", f"k_rank_sweep<{vec}>", f"k_rank_pairs<{vec},FILTER>"]
    _assert_exact(got, zs, zd, pos, known, (offset, F))


def test_exact_with_every_destination_in_the_last_partial_tile():
    pos, zs, zd, g = _int_inputs(211, 300, 64, seed=5)
    pos[1] = torch.randint(256, 300, (211,), generator=g)
    for known in (None, _superset(pos, N_SRC, 300, g)):
        _assert_exact(_run(zs, zd, pos, known), zs, zd, pos, known, known is None)


COPIES = [5, 130, 260, 390, 515, 777, 1000, 1199]   # eight different 128-destination tiles


@pytest.mark.parametrize("integer", [True, False])
def test_copies_of_the_positive_row_are_ties_in_every_tile(integer):
    """Eight rows of z_dst are copies of query 0's destination row: all eight land in n_equal, none in n_greater
    (threshold and candidates share one arithmetic).  On floats this holds only if the scores are bit-identical."""
    pos, zs, zd, g = _int_inputs(40, 1200, 64, seed=11)
    if not integer:
        zs, zd = torch.randn(N_SRC, 64, generator=g) * 0.5, torch.randn(1200, 64, generator=g) * 0.5
    pos[1, 0] = 600
    zd[COPIES] = zd[600].clone()
    got = _run(zs, zd, pos, None)
    if integer:
        _assert_exact(got, zs, zd, pos, None, "copies")
        assert got[1][0] >= 8
    else:
        assert got[1][0] == 8
        lo, hi, _, _, _ = ref_full_bands(zs.numpy(), zd.numpy(), pos.numpy(), None)
        assert lo[0] <= got[0][0] <= hi[0] - 8   # the copies are inside the band and must not count as greater


def _float_inputs(F, seed):
    g = torch.Generator().manual_seed(seed)
    E, n_dst = 64, 500
    pos = torch.stack([torch.randint(0, N_SRC, (E,), generator=g), torch.randint(0, n_dst, (E,), generator=g)])
    zs, zd = torch.randn(N_SRC, F, generator=g) * 0.5, torch.randn(n_dst, F, generator=g) * 0.5
    return pos, zs, zd, g


def _assert_in_bands(got, zs, zd, pos, known, informative=True):
    lo, hi, ge_lo, ge_hi, nc = ref_full_bands(zs.numpy(), zd.numpy(), pos.numpy(),
                                              None if known is None else known.numpy())
    gt, eq, cand = got
    print("band widths: n_greater", int((hi - lo).sum()), "coinciding queries", float((lo == hi).mean()))
    assert np.array_equal(cand, nc)
    assert bool(((lo <= gt) & (gt <= hi)).all()), np.nonzero((gt < lo) | (gt > hi))[0][:5].tolist()
    assert bool(((ge_lo <= gt + eq) & (gt + eq <= ge_hi)).all())
    if informative:
        assert float(((lo == hi) & (ge_lo == ge_hi)).mean()) >= 0.9, "uninformative: the bands are open"


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("F", [64, 256])
def test_random_floats_within_the_rounding_band(F, filtered):
    pos, zs, zd, g = _float_inputs(F, seed=2024 + F)
    known = _superset(pos, N_SRC, 500, g) if filtered else None
    _assert_in_bands(_run(zs, zd, pos, known), zs, zd, pos, known)


def test_repeatable_and_equal_for_a_repeated_query():
    pos, zs, zd, g = _float_inputs(64, seed=99)
    pos = torch.cat([pos, pos[:, 3:4], pos[:, :40], pos[:, :40], pos[:, 3:4]], 1)   # 146 queries: two query blocks
    known = _superset(pos, N_SRC, 500, g)
    a, b = _run(zs, zd, pos, known), _run(zs, zd, pos, known)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    for x in a:
        assert x[3] == x[64] == x[145] and np.array_equal(x[:40], x[65:105]) and np.array_equal(x[:40], x[105:145])


# ---------------------------------------------------------------------------------------------------
# model level (cfg1 synthetic graph)
# ---------------------------------------------------------------------------------------------------
def _metric_bounds(lo, hi, ge_lo, ge_hi, nc):
    """Each metric at the two ends of the band (rank = 1 + (n_greater + (n_greater + n_equal)) / 2 is monotone)."""
    best = ref_full_metrics(lo, ge_lo - lo, nc)
    worst = ref_full_metrics(hi, ge_hi - hi, nc)
    return best, worst


def test_link_predictor_full_metrics():
    import hgin
    from hgin.data import CONFIGS, synthetic_graph
    from hgin.linkpred import full_metrics_from_ranks, link_full_metrics, link_full_ranks
    cfg = CONFIGS["cfg1"]
    g = synthetic_graph(cfg, seed=0)
    torch.manual_seed(1997)
    model = hgin.HetroGIN(**cfg.model_kwargs({"link": cfg.f_link, "path": cfg.f_path, "node": cfg.f_node}))
    model = model.to(DEV).train()
    gd = g.to(DEV)
    pred = hgin.LinkPredictor(model, REL_PL, 3, 7)
    got = pred.full_metrics(gd)
    assert model.training                      # restored
    model.eval()
    got_eval = pred.full_metrics(gd)
    assert not model.training
    assert sorted(got) == ["auc", "hits@1", "hits@10", "hits@3", "mrr"]
    assert all(v.is_cuda and v.dtype == torch.float64 and v.dim() == 0 for v in got.values())
    assert all(float(got[k]) == float(got_eval[k]) for k in got)

    with torch.no_grad():
        z = model.encode(gd.x_dict(), gd.edge_index_dict())
    zs, zd, pos = z["path"], z["link"], g.edge_index[REL_PL]
    counts = link_full_ranks(zs, zd, pos.to(DEV), pos.to(DEV))
    same = full_metrics_from_ranks(*counts)
    assert all(float(got[k]) == float(same[k]) for k in got)
    bands = ref_full_bands(zs.cpu().numpy(), zd.cpu().numpy(), pos.numpy(), pos.numpy())
    _assert_in_bands([t.cpu().numpy().astype(np.int64) for t in counts], zs.cpu(), zd.cpu(), pos, pos,
                     informative=False)
    best, worst = _metric_bounds(*bands)
    for k in got:
        assert worst[k] - 1e-12 <= float(got[k]) <= best[k] + 1e-12, (k, worst[k], float(got[k]), best[k])

    # sources have several edges here (2000 positives over 600 paths): the filter changes the result
    unf = link_full_metrics(zs, zd, pos.to(DEV), None)
    assert float(unf["mrr"]) < float(got["mrr"]) and float(unf["hits@10"]) <= float(got["hits@10"])
    n_cand = counts[2].cpu()
    assert int(n_cand.max()) <= cfg.n_link - 1 and int(n_cand.min()) < cfg.n_link - 2
