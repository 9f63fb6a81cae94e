"""HetroGAT host-side checks (no GPU): the oracle's GATConv relation restatement reproduces the reference-executed
fixtures bit for bit (attention and aggregate), and the drop-in's constructor matches the reference's parameter
names, order and constructor-time initial values under train.py's seed (the lazy (-1, -1) projections materialise at
the first forward, on the device: checked in tests/test_gpu_gat.py).  Also the oracle's edge-list-as-given form
(``adjust_self_loops=False``) against a softmax written out row by row, and the case builders of tests/gat_cases.py:
their degrees, and that torch's own fp32 evaluation of the reference stays within a quarter of every tolerance the GPU
tests (tests/test_gpu_gat_degrees.py, tests/test_gpu_gat_wsum.py) apply on the same inputs."""
import pytest
import torch

import gat_cases as gc
from conftest import load_fixture

CASES = ["gat_cfg1_h16", "gat_w16_h4"]


def _kwargs(fx):
    m = fx["meta"]
    ic = {"link": fx["in.x.link"].shape[1], "path": fx["in.x.path"].shape[1], "node": fx["in.x.node"].shape[1]}
    return dict(input_channels=ic, node_embedding_size=m["hidden"], message_passing_layers=m["layers"], dropout=0.0,
                heads=m["heads"], concat_path=m["concat_path"], bl_features=m["bl_features"],
                divided_features=m["divided_features"], global_feats=False, mlp_layers=list(m["mlp_layers"]),
                act="torch.nn.PReLU()", mlp_head_act=None, mlp_bn=False)


def _sliced(fx):
    """models.py:482-493 feature slicing of the fixture inputs."""
    m = fx["meta"]
    x = {t: fx[f"in.x.{t}"] for t in ("path", "link", "node")}
    if not m["divided_features"]:
        x["path"] = torch.cat([x["path"][:, 0:3], x["path"][:, 6].reshape(-1, 1)], axis=1)
        x["link"] = torch.cat([x["link"][:, 0:3], x["link"][:, 4:7]], axis=1)
        if not m["bl_features"]:
            x["path"], x["link"] = x["path"][:, 0:3], x["link"][:, 0:3]
    elif not m["bl_features"]:
        x["path"], x["link"] = x["path"][:, 0:6], x["link"][:, 0:3]
    return x


@pytest.mark.parametrize("case", CASES)
def test_oracle_gat_relation_matches_reference(case):
    from oracle.pyg_cpu import gat_relation
    fx = load_fixture(case)
    x = _sliced(fx)
    H = fx["meta"]["heads"]
    for key in ("path__uses__link", "link__includes__path", "link__connects__node", "node__has__link"):
        src, _, dst = key.split("__")
        pre = f"sd.convs.0.convs.{key}."
        xs = torch.nn.functional.linear(x[src], fx[pre + "lin_src.weight"]).view(x[src].size(0), H, -1)
        xd = torch.nn.functional.linear(x[dst], fx[pre + "lin_dst.weight"]).view(x[dst].size(0), H, -1)
        alpha, agg = gat_relation(xs, xd, fx[f"in.ei.{key}"], fx[pre + "att_src"], fx[pre + "att_dst"])
        assert torch.equal(alpha, fx[f"alpha.0.{key}"]), key
        assert torch.equal(agg, fx[f"agg.0.{key}"]), key


def test_constructor_matches_reference_initialisation():
    from hgin import HetroGAT
    fx = load_fixture("gat_cfg1_h16")
    torch.manual_seed(fx["meta"]["seed_model"])
    kw = _kwargs(fx)
    ic = dict(kw["input_channels"])
    model = HetroGAT(**kw)
    assert kw["input_channels"] == ic          # HetroGAT reads input_channels; it does not mutate it (models.py:396)
    assert [n for n, _ in model.named_parameters()] == fx["meta"]["param_names_before_forward"]
    sd = model.state_dict()
    for k, v in sd.items():
        if k.endswith("lin_src.weight") or k.endswith("lin_dst.weight"):
            assert isinstance(v, torch.nn.parameter.UninitializedParameter), k   # lazy until the first forward
            continue
        assert torch.equal(v, fx["sd." + k]), k   # constructor-time RNG draws in the reference's order


def test_captured_padded_steps_refuse_gat_self_loops():
    """The captured padded steps (hgin/graphs.py) refuse HetroGAT: GATConv's bipartite self loops (i, i) for
    i < min(N_src, N_dst) would be counted on the padded capacities, giving real rows a loop from a padding source row;
    HetroGIN passes the same check (the fused step takes HetroGAT on real row counts)."""
    from hgin import HetroGAT, HetroGIN
    from hgin.graphs import _check_no_bipartite_loops
    fx = load_fixture("gat_cfg1_h16")
    kw = _kwargs(fx)
    with pytest.raises(ValueError, match="self loops"):
        _check_no_bipartite_loops(HetroGAT(**kw))
    gin_kw = {k: v for k, v in kw.items() if k != "heads"}
    _check_no_bipartite_loops(HetroGIN(**gin_kw))


def test_oracle_gat_relation_as_given_equals_dense_softmax():
    """gat_relation(adjust_self_loops=False) takes the edge list exactly as passed (coincident indices kept, nothing
    added): equal to a softmax written out per destination row over its edges in edge-list order, on 5 destinations of
    which row 2 has no edge (all-zero aggregate, finite everywhere); the default still adjusts."""
    from oracle.pyg_cpu import gat_relation
    gen = torch.Generator().manual_seed(5)
    H, C, ns, nd = 2, 3, 4, 5
    ei = torch.tensor([[0, 1, 1, 3, 2, 0, 3, 3, 1],
                       [0, 0, 1, 1, 1, 3, 3, 4, 3]])        # (0, 0), (1, 1), (3, 3): kept as they are; (1 -> 3) once
    xs = torch.randn(ns, H, C, generator=gen, dtype=torch.float64)
    xd = torch.randn(nd, H, C, generator=gen, dtype=torch.float64)
    att_s = torch.randn(1, H, C, generator=gen, dtype=torch.float64)
    att_d = torch.randn(1, H, C, generator=gen, dtype=torch.float64)
    alpha, agg = gat_relation(xs, xd, ei, att_s, att_d, adjust_self_loops=False)
    assert alpha.shape == (ei.size(1), H) and agg.shape == (nd, H, C)
    assert torch.isfinite(alpha).all() and torch.isfinite(agg).all()
    a_s, a_d = (xs * att_s).sum(-1), (xd * att_d).sum(-1)
    for i in range(nd):
        ks = [k for k in range(ei.size(1)) if int(ei[1, k]) == i]
        if not ks:
            assert i == 2 and torch.equal(agg[i], torch.zeros(H, C, dtype=torch.float64))
            continue
        for h in range(H):
            e = torch.stack([torch.nn.functional.leaky_relu(a_s[ei[0, k], h] + a_d[i, h], 0.2) for k in ks])
            w = torch.softmax(e, 0)
            assert torch.allclose(alpha[ks, h], w, rtol=1e-14, atol=0)
            want = sum(w[t] * xs[ei[0, k], h] for t, k in enumerate(ks))
            assert torch.allclose(agg[i, h], want, rtol=1e-13, atol=1e-15)
    # float64 and float32 alike: an empty row leaks neither -inf nor NaN
    _, agg32 = gat_relation(xs.float(), xd.float(), ei, att_s.float(), att_d.float(), adjust_self_loops=False)
    assert torch.isfinite(agg32).all() and not agg32[2].any()
    # the default is today's behaviour: (i, i) removed, then added for i < min(N_src, N_dst)
    alpha_adj, _ = gat_relation(xs, xd, ei, att_s, att_d)
    assert alpha_adj.size(0) == ei.size(1) - 3 + min(ns, nd)


def _quarter(r, what):
    assert r and all(v <= 0.25 for v in r.values()), (what, r)


def test_degree_ladder_builder():
    case = gc.degree_ladder(seed=3)
    assert case.n_src == 600 and case.n_dst == 29 and case.edge_index.size(1) == 1436
    assert case.in_degree.tolist() == gc.LADDER_DEGREES                      # row by row, hence the multiset
    assert gc.LADDER_DEGREES[0] == 0 and gc.LADDER_DEGREES[-1] == 0 and max(gc.LADDER_DEGREES) == 257
    out = case.out_degree
    assert not out[-gc.N_IDLE:].any() and int((out == 0).sum()) >= gc.N_IDLE
    assert int(out[gc.HUB]) > 64 and abs(int(out[gc.HUB]) - 350) <= 10
    assert torch.equal(gc.degree_ladder(seed=3).edge_index, case.edge_index)     # deterministic from the seed
    assert not torch.equal(gc.degree_ladder(seed=4).edge_index, case.edge_index)
    assert not torch.equal(case.edge_index[1], case.edge_index[1].sort().values)  # shuffled
    used, _, _ = gc.ladder_case(16, 8)
    assert used.in_degree.tolist() == gc.LADDER_DEGREES and int(used.out_degree[gc.HUB]) > 64


def test_short_rows_builder():
    case = gc.short_rows(seed=3)
    assert case.n_dst == 515 and case.n_src == 300
    assert case.in_degree.tolist() == [i % 10 for i in range(515)]
    assert int((case.in_degree == 0).sum()) == 52
    assert not case.out_degree[-gc.N_IDLE:].any()
    assert torch.equal(gc.short_rows(seed=3).edge_index, case.edge_index)


@pytest.mark.parametrize("H,C,G", gc.SHAPES_OPERANDS)
def test_ordered_rows_builder(H, C, G):
    """The orders the GPU test relies on, the size of the logits, and the quarter condition (g_x_d / g_att_dst in the
    conditioned measure of gat_cases.ratios)."""
    case, inp, ref = gc.ordered_case(H, C)
    assert case.n_dst == 6 and case.in_degree.tolist() == [gc.ORDERED_DEG] * 6
    assert not case.out_degree[-gc.N_IDLE:].any()
    a_s = (inp["xs"].double().view(-1, H, C) * inp["att_s"].double()).sum(-1)[:, 0]
    a_d = (inp["xd"].double().view(-1, H, C) * inp["att_d"].double()).sum(-1)[:, 0]
    j, i = case.edge_index
    e = [torch.nn.functional.leaky_relu(a_s[j[i == r]] + a_d[r], 0.2) for r in range(6)]
    assert bool((e[0][1:] > e[0][:-1]).all()) and bool((e[1][1:] < e[1][:-1]).all())
    assert int(e[2].argmax()) == gc.ORDERED_PEAK
    assert float(ref["max_logit"]) >= 20.0 and float(ref["alpha"].min()) <= 1e-10
    _quarter(gc.fp32_ratios(case, inp, ref, H, C, conditioned=True), "ordered")
    # the written-out g_a_d is autograd's: g_x_d = g_a_d att_dst
    want = (ref["g_ad"].unsqueeze(-1) * inp["att_d"].double()).reshape(6, H * C)
    bound = (ref["g_ad_cond"].unsqueeze(-1) * inp["att_d"].double().abs()).reshape(6, H * C)
    assert bool(((ref["g_xd"] - want).abs() <= 1e-10 * bound + 1e-300).all())


@pytest.mark.parametrize("H,C,G", gc.SHAPES)
def test_ladder_inputs_quarter_condition(H, C, G):
    case, inp, ref = gc.ladder_case(H, C)
    r = gc.fp32_ratios(case, inp, ref, H, C)
    assert set(r) == {"out", "alpha", "alpha_sum"} | set(gc.GRADS)
    _quarter(r, "ladder")
    empty = case.in_degree == 0
    assert torch.equal(ref["out"][empty], inp["bias"].double().expand(int(empty.sum()), -1))
    assert not ref["g_xs"][case.out_degree == 0].any()
    if (H, C, G) in gc.SHAPES_OPERANDS:
        for variant in (dict(use_xd=False), dict(use_bias=False), dict(use_accum=True)):
            case, inp, ref = gc.ladder_case(H, C, **{**dict(use_xd=True, use_bias=True, use_accum=False), **variant})
            _quarter(gc.fp32_ratios(case, inp, ref, H, C, **variant), variant)


@pytest.mark.parametrize("H,C,G", gc.SHAPES_SHORT)
def test_short_rows_inputs_quarter_condition(H, C, G):
    case, inp, ref = gc.short_case(H, C)
    _quarter(gc.fp32_ratios(case, inp, ref, H, C), "short_rows")


@pytest.mark.parametrize("n,H,C", gc.WSUM_CASES)
def test_wsum_inputs_quarter_condition(n, H, C):
    for weighted in (False, True):
        assert gc.wsum_fp32_ratio(n, H, C, weighted) <= 0.25, (n, H, C, weighted)
