"""Host side of the fused small-batch step's shape tests (tests/smallbatch_cases.py): the adversarial graphs have
exactly the rows and degrees they claim, their collation equals oracle/collate_np.py's, the float64 oracle gives every
case a finite non-zero loss and every live parameter a non-zero gradient (so that a norm-relative tolerance is never
vacuous), and the Python mirror of the staging arithmetic says which cases reach a second staging block — and that the
sizes tests/test_gpu_smallbatch.py runs never do.  The GPU half is tests/test_gpu_smallbatch_edges.py."""
import math

import pytest
import torch

import smallbatch_cases as sc
from hgin.data import REL_LN, REL_LP, REL_NL, REL_PL

# the model shapes of tests/test_gpu_smallbatch_edges.py's staging sweep (C.1): (hidden, layers)
SWEEP_SHAPES = [(8, 2), (32, 2), (64, 2), (128, 3)]


def _n(g, t):
    return g.x[t].shape[0]


@pytest.mark.parametrize("name", sc.ALL_CASES)
def test_case_layout_and_labels(name):
    """7 / 7 / 3 features, y in [0.5, 1.5], the reverse relations exact flips, every endpoint in range."""
    for g in sc.case(name).graphs:
        assert [g.x[t].shape[1] for t in sc.TYPES] == [7, 7, 3]
        assert g.y.shape == (_n(g, "path"),) and float(g.y.min()) >= 0.5 and float(g.y.max()) <= 1.5
        assert torch.equal(g.edge_index[REL_LP], g.edge_index[REL_PL].flip(0))
        assert torch.equal(g.edge_index[REL_NL], g.edge_index[REL_LN].flip(0))
        for (s, _, d), e in g.edge_index.items():
            assert e.dtype == torch.long and e.shape[0] == 2
            if e.shape[1]:
                assert 0 <= int(e[0].min()) and int(e[0].max()) < _n(g, s)
                assert 0 <= int(e[1].min()) and int(e[1].max()) < _n(g, d)


@pytest.mark.parametrize("name", list(sc.TOTALS_WANT))
def test_totals_sit_on_and_one_past_the_blocks(name):
    """The batch's rows per type are exactly the stated totals: one type a multiple of 32 (the scalar forward's block,
    the MFMA readout's tile; also of 8: the MFMA forward's block, the scalar readout's tile), one a multiple of 32 plus
    one, one a multiple of 8 (not of 32) plus one — each type taking each role once over the three cases."""
    c = sc.case(name)
    tot = c.totals(c.batches[0])
    assert tuple(tot[t] for t in sc.TYPES) == sc.TOTALS_WANT[name]
    kinds = sorted("32k" if v % 32 == 0 else "32k+1" if v % 32 == 1 else "8k+1" if v % 8 == 1 else "?"
                   for v in tot.values())
    assert kinds == ["32k", "32k+1", "8k+1"]


def test_one_node_and_tiny_paths():
    c = sc.case("one_node")
    for g in c.graphs:
        assert _n(g, "node") == 1 and int(g.edge_index[REL_LN][1].max()) == 0
        assert sc.degrees(g, REL_LN, 1, 1).tolist() == [g.edge_index[REL_LN].shape[1]]
    m = sc.case("mvalid")
    assert tuple(_n(m.graphs[0], t) for t in sc.TYPES) == sc.MVALID_BIG
    assert _n(m.graphs[1], "path") == 1 and _n(m.graphs[2], "path") == 2
    assert m.batch_size == 1 and not m.normalize


def test_empty_relation_pair():
    for g in sc.case("empty_ln").graphs:
        assert g.edge_index[REL_LN].shape == (2, 0) and g.edge_index[REL_NL].shape == (2, 0)
        assert g.edge_index[REL_PL].shape[1] > 0


@pytest.mark.parametrize("name", ["hub_link", "hub_path"])
def test_hubs_and_isolated_ends(name):
    """The hub's degree is exact in both directions (the forward's CSR row and the backward's CSC row), the first and
    the last row of every type carry no edge in any relation, and nothing else comes near the hub."""
    c = sc.case(name)
    assert c.isolated_ends
    for g in c.graphs:
        n = {t: _n(g, t) for t in sc.TYPES}
        for (s, _, d), e in g.edge_index.items():
            for side, t in ((0, s), (1, d)):
                deg = sc.degrees(g, (s, _, d), side, n[t])
                assert int(deg[0]) == 0 and int(deg[-1]) == 0, (s, d, side)
        by_path = sc.degrees(g, REL_PL, 0, n["path"])
        by_link = sc.degrees(g, REL_PL, 1, n["link"])
        assert torch.equal(by_path, sc.degrees(g, REL_LP, 1, n["path"]))
        assert torch.equal(by_link, sc.degrees(g, REL_LP, 0, n["link"]))
        if c.hub_link:
            hub = n["link"] // 2
            users = torch.unique(g.edge_index[REL_PL][0][g.edge_index[REL_PL][1] == hub])
            assert torch.equal(users, torch.arange(1, n["path"] - 1))   # every path that carries edges uses it
            assert int(by_link[hub]) >= n["path"] - 2 >= 300
            rest = by_link.clone()
            rest[hub] = 0
            assert int(rest.max()) < 40
        if c.hub_path:
            hub = n["path"] // 2
            assert int(by_path[hub]) >= sc.HUB_DEGREE >= 300
            rest = by_path.clone()
            rest[hub] = 0
            assert int(rest.max()) < 20   # the other chains of a gather_chain4 batch end after a round or two


@pytest.mark.parametrize("name", sc.ALL_CASES)
def test_collation_matches_collate_np(name):
    c = sc.case(name)
    for ids in c.batches:
        b = c.host_batch(ids)
        sc.assert_collation(b, c.host_singles(ids))
        assert {t: b.x[t].shape[0] for t in sc.TYPES} == c.totals(ids)


RO_CASE = "totals_p32k1_l8k1_n32k"   # tests/test_gpu_smallbatch_edges.py's readout case
RO_WIDTHS = [[256, 256], [256], [256, 256, 256], [128, 128], [96, 96], [1], [3, 5], [33, 1, 7]]


def _models_for(name):
    """(constructor overrides, batches) of every HetroGIN variant tests/test_gpu_smallbatch_edges.py runs the case
    with."""
    c = sc.case(name)
    if name == "sweep":
        overs = [dict(node_embedding_size=H, message_passing_layers=L) for H, L in SWEEP_SHAPES]
        overs += [dict(node_embedding_size=H) for H in (5, 63, 72, 127)]
        overs += [dict(mlp_bn=True, global_feats=True, bl_features=True),
                  dict(node_embedding_size=127, message_passing_layers=3, global_feats=True, bl_features=True)]
        return [(o, c.batches) for o in overs]
    if name == "mvalid":
        out = [(dict(node_embedding_size=H), c.batches) for H in (8, 64)]
        out += [(dict(node_embedding_size=H, mlp_bn=True), c.batches[2:]) for H in (8, 64)]
        return out + [(dict(node_embedding_size=H, global_feats=True, bl_features=True), c.batches[1:2])
                      for H in (8, 64)]
    out = [(dict(node_embedding_size=H), c.batches) for H in (8, 64)]
    if name == RO_CASE:
        out += [(dict(mlp_layers=w), c.batches) for w in RO_WIDTHS]
    return out


@pytest.mark.parametrize("name", sc.ALL_CASES)
def test_oracle_loss_and_live_gradients_are_nonzero(name):
    """In float64: a finite, non-zero loss, and a gradient norm above zero for every parameter autograd reaches — bar
    the convs of an empty relation pair, whose own gradients may vanish: with no link -> node edge nothing a node row
    holds reaches a path, so link -> node convs below the last layer and the aggregate columns of node -> link convs
    have a zero true gradient (asserted to be exactly that: nothing else may vanish)."""
    from hgin import HetroGIN
    from hgin.smallbatch import RELS, dead_convs
    c = sc.case(name)
    for over, batches in _models_for(name):
        kw = sc.model_kwargs(**over)
        torch.manual_seed(1997)
        model = HetroGIN(**sc.model_kwargs(**over))
        ref = sc.oracle_twin(model, kw)
        for ids in batches:
            lv = sc.oracle_step(ref, c.host_batch(ids))
            assert math.isfinite(lv) and lv > 0.0, (over, ids, lv)
            norms = sc.grad_norms(ref)
            dead = {f"convs.{l}.convs.{'__'.join(RELS[ri])}." for l, ri in dead_convs(kw["message_passing_layers"])}
            for n, v in norms.items():
                if any(n.startswith(d) for d in dead):
                    assert v is None, n
                    continue
                assert v is not None and math.isfinite(v), n
                if name == "empty_ln" and "link__connects__node" in n:
                    assert v == 0.0, (n, v)
                    continue
                if over.get("mlp_bn") and n.startswith("readout.") and n.endswith(".0.bias") \
                        and not n.startswith(f"readout.{len(kw['mlp_layers'])}."):
                    continue   # a Linear bias ahead of a BatchNorm: zero in exact arithmetic (the 1e-6 slack's reason)
                assert v > 0.0, (over, ids, n)


@pytest.mark.parametrize("H", [8, 64])
def test_two_row_batchnorm_case_is_conditioned_for_fp32(H):
    """MLP_BN over the two-row batch: BatchNorm's backward cancels to eps / (var + eps) of its terms there, and at most
    seeds of that graph torch's own fp32 evaluation of the oracle misses the GPU test's tolerance severalfold against
    its float64 evaluation.  The graph's seed is one at which it stays within a quarter of it, so a correct fp32 kernel
    has a fourfold margin; if this fails, the seed changes (as in tests/gat_cases.py), never the tolerance."""
    from hgin import HetroGIN
    c = sc.case("mvalid")
    over = dict(node_embedding_size=H, mlp_bn=True)
    torch.manual_seed(1997)
    model = HetroGIN(**sc.model_kwargs(**over))
    r = sc.fp32_ratio(model, sc.model_kwargs(**over), c.host_batch(c.batches[2]))
    assert r <= 0.25, r


@pytest.mark.parametrize("H,L", SWEEP_SHAPES)
def test_sweep_case_takes_two_staging_blocks_at_one_part(H, L):
    """With n_parts = 1 the sweep case re-stages in k_sb_bwd_w (every conv, every destination type), in
    ro_weight_part for every readout layer and for the head (N = 1); with n_parts = 128 it does not (one block)."""
    c = sc.case("sweep")
    rows = c.totals(c.batches[0])
    kw = sc.model_kwargs(node_embedding_size=H, message_passing_layers=L)
    for h, k, d in sc.conv_widths(kw):
        assert sc.staging_blocks(rows[d], 1, "gin", h, k) >= 2, (h, k, d)
        assert sc.staging_blocks(rows[d], 128, "gin", h, k) == 1
    for n, k in sc.readout_widths(kw):
        assert sc.staging_blocks(rows["path"], 1, "readout", H, k, n) >= 2, (n, k)
    assert sc.readout_widths(kw)[-1][0] == 1
    # n_parts = 3 and 8 too (chunks of 683 and 256 path rows): past one block wherever the cap is below the chunk
    assert sc.staging_blocks(rows["path"], 3, "gin", H, H) >= 2
    assert sc.final_idle_groups(1) == 7 and sc.final_idle_groups(3) == 5 and sc.final_idle_groups(8) == 0
    assert sc.empty_chunks(rows["node"], 1024) > 0 and sc.empty_chunks(rows["path"], 128) == 0


def test_other_sweep_models_take_two_staging_blocks_at_one_part():
    c = sc.case("sweep")
    rows = c.totals(c.batches[0])
    for kw in (sc.model_kwargs(mlp_bn=True, global_feats=True, bl_features=True),
               sc.model_kwargs(node_embedding_size=63), sc.model_kwargs(node_embedding_size=127)):
        for h, k, d in sc.conv_widths(kw):
            assert sc.staging_blocks(rows[d], 1, "gin", h, k) >= 2
        for n, k in sc.readout_widths(kw):
            assert sc.staging_blocks(rows["path"], 1, "readout", 0, k, n) >= 2
    gk = sc.gat_kwargs()
    assert sc.staging_blocks(rows["path"], 1, "gat", gk["heads"], 0) >= 2
    for n, k in sc.readout_widths(gk, H=128):
        assert sc.staging_blocks(rows["path"], 1, "readout", 128, k, n) >= 2


def test_weight_groups_past_the_first():
    """Where ``u > 0`` register-tile groups exist: not at hidden 8 or 32 (one group for every conv), but at hidden 63
    (two groups at the 63-wide layers) and in the readout's 128 -> 32 layer (three) — with n_parts = 1 those groups
    re-stage every row block."""
    assert sc.weight_groups(8, 6) == 1 and sc.weight_groups(8, 8) == 1 and sc.weight_groups(32, 32) == 1
    assert sc.weight_groups(63, 63) == 2 and sc.weight_groups(5, 5) == 1
    assert sc.weight_groups(32, 128) == 3 and sc.weight_groups(1, 32) == 1
    assert sc.weight_groups(256, 256) == 33


def test_existing_oracle_test_never_leaves_the_first_staging_block():
    """The gap this closes: at the sizes of tests/test_gpu_smallbatch.py::test_fused_step_vs_oracle (and n_parts = 128)
    every weight-gradient loop runs exactly once, at every hidden width that file uses."""
    rows = sc.existing_rows()
    assert 1500 < rows["path"] < 3500 and rows["link"] < rows["path"] and rows["node"] < rows["link"]
    for H in (8, 64, 96, 128):
        for L in (1, 2, 3):
            kw = sc.model_kwargs(node_embedding_size=H, message_passing_layers=L)
            for h, k, d in sc.conv_widths(kw):
                assert sc.staging_blocks(rows[d], 128, "gin", h, k) == 1
            for n, k in sc.readout_widths(kw):
                assert sc.staging_blocks(rows["path"], 128, "readout", H, k, n) == 1
    assert sc.stage_rows("gin", 128, 128) == 47   # the smallest cap a tested shape produces
