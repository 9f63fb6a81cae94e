"""The fused small-batch step (hgin/smallbatch.py, csrc/hgin_smallbatch.hip) past one staging block and at shape edges:
what tests/test_gpu_smallbatch.py and tests/test_gpu_smallbatch_gat.py compile and ship but never execute, because
every batch they run is three or four cfg1-sized uniform random graphs at n_parts = 128.

Each test is one captured step with Adam at lr 0 against the float64 CPU oracle on the host-collated batch
(tests/smallbatch_cases.py): the loss within 1e-5 relative, every gradient within 1e-4 of its norm (+ 1e-6 of the
largest norm with MLP_BN), the dead convs' gradients absent on both sides, and a second replay of the same batch
bitwise identical.  Staging claims ("this case re-stages") are asserted through the Python mirror of the kernels'
arithmetic, smallbatch_cases.staging_blocks.

What reaches what:

* the second and later ``rb`` blocks of k_sb_bwd_w<false> / <true>, ro_weight_part and k_sb_gat_bwd (re-staging, the
  accumulate-into-global branch, bsum / sp / epv carried across blocks): test_partition_sweep,
  test_partition_extremes, test_hidden_widths[*-1]; the ``u > 0`` groups that stage the rows again:
  test_hidden_widths[63-2-False-1] (k_sb_bwd_w<false>), test_wide_readout_restages_every_group (ro_weight_part);
* n_parts other than 128 (k_sb_final's idle lane groups, empty chunks: the MFMA kernel's zero fill, the scalar
  kernels' zero WgTile): test_partition_sweep (1, 3, 8; 1024 at hidden 8), test_partition_extremes (1, 1024);
* readout modes 0, 1, 2, 4 (4 on 32- and on 16-row tiles), widths of 256, 1 and odd, three hidden layers without
  BatchNorm, stage_ro_params' tail loop: test_readout_modes, test_wide_readout_auto_mode_as_stated,
  test_wide_readout_restages_every_group;
* hidden widths off the grid: test_hidden_widths;
* graph-shape edges: test_graph_shape_edges, test_tiny_batches_in_a_large_capacity_step,
  test_tiny_batch_mlp_bn_two_rows, test_tiny_batch_global_feats_one_row_graph, test_large_tiny_large.

Worst observed error / tolerance per family (one MI355X run of this file, 7 s in all; 1 = at the tolerance; every
test prints its own as ``ratio[family] ...``):

* C.1 staging and partition sweep: 0.19 (hidden 128, L = 3, n_parts = 3; n_parts = 1: 0.05 there, 0.012 at hidden 8,
  32 and 64; MLP_BN + GLOBAL_FEATS 0.08; HetroGAT 0.010);
* C.2 readout modes and widths: 0.20 ([256, 256, 256] at n_parts = 8; 0.15 at 128; every other width <= 0.013); the
  evaluation steps: 0.07;
* C.3 hidden widths: 0.03 (hidden 5 at n_parts = 1; 63, 72, 127: <= 0.013);
* C.4 graph-shape edges: 0.76 (MLP_BN over two rows at hidden 8, 0.16 at hidden 64: see
  smallbatch_cases.fp32_ratio); without BatchNorm 0.23 (the one-path batch at hidden 64), the hub link at hidden 64
  0.11, everything else <= 0.05.
"""
import ctypes

import pytest
import torch

import smallbatch_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda"

# this run's worst error / tolerance per test family (loss and gradients together), filled as the tests run
RATIOS = {}

_STORES, _BATCHES = {}, {}


def _store(name):
    from hgin.store import GraphStore
    if name not in _STORES:
        c = sc.case(name)
        _STORES[name] = GraphStore.build(list(c.graphs), device=DEV, normalize=c.normalize)
    return _STORES[name]


def _host_batch(name, ids):
    """The store's batch on the host, pinned to collate_np and to the case's own host collation (what the CPU tests
    checked); built once per (case, ids) and shared."""
    key = (name, tuple(ids))
    if key not in _BATCHES:
        b = sc.host_batch(_store(name), list(ids))
        want = sc.case(name).host_batch(ids)
        for t in sc.TYPES:
            assert torch.equal(b.x[t], want.x[t]), t
        for r in want.edge_index:
            assert torch.equal(b.edge_index[r], want.edge_index[r]), r
        assert torch.equal(b.y, want.y)
        _BATCHES[key] = b
    return _BATCHES[key]


def _build(name, over, gat=False, readout="auto", n_parts=None):
    """(model, captured step, constructor kwargs) on the case's store, warmed up on its first batch."""
    from hgin import HetroGAT, HetroGIN
    from hgin.smallbatch import SmallBatchStep
    c = sc.case(name)
    mk = (lambda: sc.gat_kwargs(**over)) if gat else (lambda: sc.model_kwargs(**over))   # noqa: E731
    torch.manual_seed(1997)
    model = (HetroGAT if gat else HetroGIN)(**mk()).to(DEV)
    step = SmallBatchStep(model, torch.optim.Adam(model.parameters(), lr=0.0), _store(name), c.batch_size,
                          warmup_ids=[list(c.batches[0])], warmup=1, readout=readout, n_parts=n_parts)
    torch.cuda.synchronize()
    assert step.folded and step.args.n_parts == (n_parts or 128)
    return model, step, mk()


def _check(family, name, model, step, kw, ids, gat=False, replay=True, tag=None):
    """One step on ``ids`` against the float64 oracle (+ the bitwise second replay); returns (the gradients, the
    oracle after its backward)."""
    ref = sc.oracle_twin(model, kw, gat=gat)   # (after the warm-up, which advanced MLP_BN's running statistics)
    lv = float(step.step(list(ids)))
    torch.cuda.synchronize()
    b = _host_batch(name, ids)
    assert int(step.batch.m_valid) == b.x["path"].shape[0]
    lv_ref = sc.oracle_step(ref, b)
    tag = (family, name, tag, tuple(ids))
    r = sc.check_step(model, ref, lv, lv_ref, bn=kw["mlp_bn"], tag=tag)
    print(f"ratio[{family}] {tag}: {r:.4f}")
    RATIOS[family] = max(RATIOS.get(family, 0.0), r)
    if kw["mlp_bn"]:
        sc.check_buffers(model, ref)
    grads = {n: sc.grad_of(p).clone() for n, p in model.named_parameters()}
    if replay:
        assert float(step.step(list(ids))) == lv, tag
        torch.cuda.synchronize()
        for n, p in model.named_parameters():
            assert torch.equal(sc.grad_of(p), grads[n]), (tag, n)
    return grads, ref


def _agree(ga, gb, ref, bn, tag):
    """Two partitions of the same sums differ by re-association only: within twice the tolerance of each other."""
    gmax = max(float(q.grad.double().norm()) for q in ref.parameters() if q.grad is not None)
    for n, q in ref.named_parameters():
        if q.grad is None:
            continue
        bound = 2.0 * (sc.GRAD_TOL * float(q.grad.double().norm()) + (sc.BN_SLACK * gmax if bn else sc.GRAD_ABS))
        d = float((ga[n].double() - gb[n].double()).norm())
        assert d <= bound, (tag, n, d, bound)


def _eval_check(family, name, over, ids):
    """One SmallBatchEval step against the eval-mode float64 oracle: loss 1e-5, predictions 1e-5."""
    from hgin import HetroGIN
    from hgin.smallbatch import SmallBatchEval
    c = sc.case(name)
    torch.manual_seed(1997)
    model = HetroGIN(**sc.model_kwargs(**over)).to(DEV).eval()
    ev = SmallBatchEval(model, _store(name), c.batch_size, warmup_ids=[list(c.batches[0])], warmup=1)
    lv = float(ev.step(list(ids)))
    torch.cuda.synchronize()
    ref = sc.oracle_twin(model, sc.model_kwargs(**over)).eval()
    with torch.no_grad():
        out, lv_ref = sc.oracle_forward(ref, _host_batch(name, ids))
    r = sc.check_eval(ev.out_pred[:out.shape[0]], lv, out, float(lv_ref), tag=(name, over))
    print(f"ratio[{family}] eval {name} {over}: {r:.4f}")
    RATIOS[family] = max(RATIOS.get(family, 0.0), r)
    return ev


def _lds_bytes(step, kw, mode):
    from hgin import _lib
    a = step.args
    w0 = a.H + (a.fdim[0] if a.concat_path else 0) + a.pool_w
    widths = (ctypes.c_int32 * 3)(*[a.rw[i] for i in range(3)])
    out = ctypes.c_size_t(0)
    _lib.check(_lib.lib().hgin_sb_readout_lds_bytes(a.H, w0 - a.H, int(w0 > a.H), a.nhid, widths, mode,
                                                    ctypes.byref(out)), "hgin_sb_readout_lds_bytes")
    return out.value


# ---- C.1 staging and partition sweep ------------------------------------------------------------------------------

SWEEP_SHAPES = [(8, 2), (32, 2), (64, 2), (128, 3)]


def _assert_restaged(kw, rows, H=None, types=sc.TYPES):
    for h, k, d in sc.conv_widths(kw):
        assert d not in types or sc.staging_blocks(rows[d], 1, "gin", h, k) >= 2, (h, k, d)
    for n, k in sc.readout_widths(kw, H):
        assert sc.staging_blocks(rows["path"], 1, "readout", 0, k, n) >= 2, (n, k)


@pytest.mark.parametrize("H,L", SWEEP_SHAPES)
def test_partition_sweep(H, L):
    """n_parts in {1, 3, 8, 128} (and 1024 at hidden 8) on 2048 / 1315 / 706 rows.  n_parts = 1: every conv of
    k_sb_bwd_w (the scalar kernel at hidden 8 and 32, the MFMA kernel at 64 and 128), every readout layer and the head
    (N = 1) of ro_weight_part take >= 2 ``rb`` blocks — the re-staging, ``*e = rb == i0 ? v : *e + v``, bsum / sp /
    epv across blocks — and 7 of k_sb_final's 8 lane groups have np == 0; n_parts = 3: 5 idle groups; n_parts = 1024:
    a third of the link chunks and most node chunks are empty (zero WgTiles).  The gradients of every partition agree with n_parts = 128's within twice the
    tolerance."""
    c = sc.case("sweep")
    rows = c.totals(c.batches[0])
    over = dict(node_embedding_size=H, message_passing_layers=L)
    _assert_restaged(sc.model_kwargs(**over), rows)
    assert sc.final_idle_groups(1) == 7 and sc.final_idle_groups(3) == 5
    grads, ref = {}, None
    for n_parts in (128, 1, 3, 8) + ((1024,) if H == 8 else ()):
        model, step, kw = _build("sweep", over, n_parts=n_parts)
        grads[n_parts], ref = _check("C.1", "sweep", model, step, kw, c.batches[0], tag=(H, L, n_parts))
    assert sc.empty_chunks(rows["link"], 1024) > 300 and sc.empty_chunks(rows["node"], 1024) > 300
    for n_parts in grads:
        _agree(grads[n_parts], grads[128], ref, False, (H, L, n_parts))


@pytest.mark.parametrize("variant", ["mlp_bn_global_feats", "gat"])
def test_partition_extremes(variant):
    """MLP_BN + GLOBAL_FEATS (the k_sb_bn_* readout: gamma / beta partials only in row chunk 0, the Linears through
    ro_weight_part) and the dropout-free default HetroGAT (k_sb_gat_bwd: 16 rows per pass) at n_parts = 1 — >= 2 blocks
    in every loop — and n_parts = 1024 — every chunk 2 rows or empty; the two agree within twice the tolerance."""
    c = sc.case("sweep")
    rows = c.totals(c.batches[0])
    gat = variant == "gat"
    over = {} if gat else dict(mlp_bn=True, global_feats=True, bl_features=True)
    if gat:
        gk = sc.gat_kwargs()
        assert sc.staging_blocks(rows["path"], 1, "gat", gk["heads"], 0) >= 2
        for n, k in sc.readout_widths(gk, H=gk["heads"] * gk["node_embedding_size"]):
            assert sc.staging_blocks(rows["path"], 1, "readout", 0, k, n) >= 2
    else:
        _assert_restaged(sc.model_kwargs(**over), rows)
    assert sc.empty_chunks(rows["link"], 1024) > 0
    grads, ref = {}, None
    for n_parts in (1, 1024):
        model, step, kw = _build("sweep", over, gat=gat, n_parts=n_parts)
        assert step.gat == gat and (gat or step.args.ro_wlds == 3)
        grads[n_parts], ref = _check("C.1", "sweep", model, step, kw, c.batches[0], gat=gat, tag=(variant, n_parts))
    _agree(grads[1], grads[1024], ref, not gat, variant)


# ---- C.2 readout modes and widths ---------------------------------------------------------------------------------

RO_CASE = "totals_p32k1_l8k1_n32k"   # 1217 path rows: the last readout tile holds one row (8-, 16- and 32-row tiles)
# name: (constructor overrides, ro_wlds with readout="auto", with readout="scalar")
READOUTS = {
    "w256_256": (dict(mlp_layers=[256, 256]), 4, 0),
    "w256": (dict(mlp_layers=[256]), 4, 1),
    "w256_256_256": (dict(mlp_layers=[256, 256, 256]), 0, 0),
    "w128_128": (dict(mlp_layers=[128, 128]), 4, 1),
    "w96_96": (dict(mlp_layers=[96, 96]), 2, 1),
    "w1": (dict(mlp_layers=[1]), 2, 1),
    "w3_5": (dict(mlp_layers=[3, 5]), 2, 1),
    "w33_1_7": (dict(mlp_layers=[33, 1, 7]), 2, 1),
    "hidden64": (dict(node_embedding_size=64), 4, 1),
}
RO_ORDER = {"auto": (2, 4, 1, 0), "scalar": (1, 0)}
LDS_LIMIT = 159 * 1024


@pytest.mark.parametrize("readout", ["auto", "scalar"])
@pytest.mark.parametrize("name", list(READOUTS))
def test_readout_modes(name, readout):
    """``mlp_layers=[256, 256]`` selects mode 4 (k_sb_readout_mfma<false>) with readout="auto" — on 16-row tiles, the
    32-row tile's 232,704 B of LDS being more than a readout is granted (ro_rows_m; [256] alone too: 166,912 B) — and
    mode 0 (k_sb_readout<false>: 8-row tiles, the weights through the caches) with readout="scalar"; three hidden
    layers without BatchNorm, [256, 256, 256], fit neither MFMA tile and run in mode 0 either way; mode 4 on 32-row
    tiles outside hidden 128 at [128, 128] and at hidden 64; mode 1 at hidden 64 and at every odd / unit width; mode 2
    at [1], [3, 5] and [33, 1, 7] (a 1-wide layer between two odd ones: K = 1 MFMA steps, N = 1 column blocks).  The
    selected mode is asserted, and that every mode ahead of it in the constructor's order does not fit the 159 KiB
    the constructor allows.  readout="auto" also runs one SmallBatchEval step against the eval-mode oracle (loss 1e-5,
    predictions 1e-5).

    stage_ro_params' tail loop ("wider layers than cfg1's": a staged W of more than 16 entries per thread) runs in mode
    1 at [128, 128], [96, 96] and hidden 64 (more than 4096 entries) and in mode 2 at [96, 96] (9216 > 8192)."""
    over, want_auto, want_scalar = READOUTS[name]
    c = sc.case(RO_CASE)
    ids = c.batches[0]
    if readout == "auto":
        ev = _eval_check("C.2", RO_CASE, over, ids)
        assert ev.args.ro_wlds == want_auto
    model, step, kw = _build(RO_CASE, over, readout=readout)
    want = want_auto if readout == "auto" else want_scalar
    assert step.args.ro_wlds == want, (name, readout, step.args.ro_wlds)
    for mode in RO_ORDER[readout]:
        if mode == want:
            assert _lds_bytes(step, kw, mode) <= LDS_LIMIT
            break
        assert _lds_bytes(step, kw, mode) > LDS_LIMIT, (name, mode)
    _check("C.2", RO_CASE, model, step, kw, ids, tag=(name, readout))


def test_wide_readout_auto_mode_as_stated():
    """``mlp_layers=[256, 256]`` with readout="auto" selects mode 4 and with readout="scalar" mode 0, at hidden 8 and at
    hidden 128 (the widest input the readout takes); the LDS the step asks for is the 16-row tile's."""
    for H in (8, 128):
        over = dict(mlp_layers=[256, 256], node_embedding_size=H)
        _, step, kw = _build(RO_CASE, over)
        assert step.args.ro_wlds == 4, (H, step.args.ro_wlds)
        assert step.lds == _lds_bytes(step, kw, 4) <= LDS_LIMIT and 2 * step.lds > LDS_LIMIT
        _, step, _ = _build(RO_CASE, over, readout="scalar")
        assert step.args.ro_wlds == 0, (H, step.args.ro_wlds)


def test_wide_readout_restages_every_group():
    """[256, 256, 256] at n_parts = 8: ro_weight_part's chunks of 153 rows take 10 blocks of 16 rows in the 256 -> 256
    layers, in each of their 33 register-tile groups (``u`` up to 32: wg_setup's kc0, the clamped kj past K + 1)."""
    c = sc.case(RO_CASE)
    rows = c.totals(c.batches[0])["path"]
    assert sc.staging_blocks(rows, 8, "readout", 0, 256, 256) == 10 and sc.weight_groups(256, 256) == 33
    model, step, kw = _build(RO_CASE, dict(mlp_layers=[256, 256, 256]), n_parts=8)
    assert step.args.ro_wlds == 0 and step.args.nhid == 3
    _check("C.2", RO_CASE, model, step, kw, c.batches[0], tag="w256x3_parts8")


# ---- C.3 hidden widths --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,L,global_feats,n_parts", [
    (5, 2, False, None), (63, 2, False, None), (72, 2, False, None), (127, 2, False, None), (127, 3, True, None),
    (5, 2, False, 1), (63, 2, False, 1), (72, 2, False, 1), (127, 2, False, 1)])
def test_hidden_widths(H, L, global_feats, n_parts):
    """Hidden widths off the multiples of 8.  5 and 63: the scalar kernels (63 the widest; its 63-wide convs have two
    weight groups, so with n_parts = 1 the ``u = 1`` group re-stages every row block); 72 and 127: the MFMA kernels
    with ``kn`` tails in every 16-column W chunk of the forward, N % 32 != 0 in tile_mfma, and at 127 (odd: H | 1 == H)
    no stride padding.  n_parts = 1: >= 2 staging blocks in every loop (asserted; at hidden 5 a block holds 742 rows
    of the first layer, more than the batch's 706 node rows: there for the path and link rows)."""
    c = sc.case("sweep")
    over = dict(node_embedding_size=H, message_passing_layers=L)
    if global_feats:
        over.update(global_feats=True, bl_features=True)
    if n_parts == 1:
        _assert_restaged(sc.model_kwargs(**over), c.totals(c.batches[0]),
                         types=("path", "link") if H == 5 else sc.TYPES)
    if H == 63:
        assert sc.weight_groups(63, 63) == 2
    model, step, kw = _build("sweep", over, n_parts=n_parts)
    assert step.args.H == H and (step.args.pool_w == 8) == global_feats
    _check("C.3", "sweep", model, step, kw, c.batches[0], tag=(H, L, global_feats, n_parts))


# ---- C.4 graph-shape edges ----------------------------------------------------------------------------------------

RO_MODE = {(8, "auto"): 2, (8, "scalar"): 1, (64, "auto"): 4, (64, "scalar"): 1}
edge_grid = lambda f: pytest.mark.parametrize("readout", ["auto", "scalar"])(   # noqa: E731
    pytest.mark.parametrize("H", [8, 64])(f))


@edge_grid
@pytest.mark.parametrize("name", sc.EDGE_CASES)
def test_graph_shape_edges(name, H, readout):
    """At hidden 8 (k_sb_fwd<false>: 32-row blocks) and 64 (k_sb_fwd<true>: 8-row blocks), readout on 32-row MFMA
    tiles and on 8-row scalar tiles:

    * totals_*: per type the batch's rows exactly 32 k, 32 k + 1 and 8 k + 1, each type in each role once — the last
      forward block / readout tile full, or holding a single row;
    * one_node: n_node = 1 in every graph (every link -> node edge of a graph ends in one row);
    * empty_ln: no link -> node / node -> link edge in the batch (empty CSR and CSC; the gradients that vanish with it
      must be exact zeros: 1e-4 of a zero norm + 1e-9);
    * hub_link / hub_path: a link used by every path / a path using 320 links — gather_chain and gather_chain4 run
      40+ rounds for one row while the other chains of the batch end after one or two — with the first and the last row
      of every type isolated (empty ranges at both ends of every CSR / CSC)."""
    c = sc.case(name)
    model, step, kw = _build(name, dict(node_embedding_size=H), readout=readout)
    assert step.args.ro_wlds == RO_MODE[(H, readout)]
    _check("C.4", name, model, step, kw, c.batches[0], tag=(H, readout))


@edge_grid
def test_tiny_batches_in_a_large_capacity_step(H, readout):
    """A step whose capacity comes from one graph of 2001 paths, replayed on batches of 1 and then 2 path rows: all but
    the first block of every forward launch exit at ``r0 >= n``, all but the first readout tile at ``tile >= ntile``,
    and with 128 chunks of ceil(m / 128) = 1 row all but one or two chunks are empty."""
    c = sc.case("mvalid")
    model, step, kw = _build("mvalid", dict(node_embedding_size=H), readout=readout)
    assert step.args.cap[0] == sc.MVALID_BIG[0] and step.args.ro_wlds == RO_MODE[(H, readout)]
    for ids in (c.batches[1], c.batches[2]):
        assert sc.empty_chunks(c.totals(ids)["path"], 128) >= 126
        _check("C.4", "mvalid", model, step, kw, ids, tag=(H, readout))


@pytest.mark.parametrize("H", [8, 64])
def test_tiny_batch_mlp_bn_two_rows(H):
    """MLP_BN on two path rows (torch's BatchNorm refuses one): one 32-row tile holding two rows in every k_sb_bn_*
    launch, the unbiased running variance over m - 1 = 1."""
    c = sc.case("mvalid")
    model, step, kw = _build("mvalid", dict(node_embedding_size=H, mlp_bn=True))
    assert step.args.ro_wlds == 3
    _check("C.4", "mvalid", model, step, kw, c.batches[2], tag=(H, "mlp_bn"))


@edge_grid
def test_tiny_batch_global_feats_one_row_graph(H, readout):
    """GLOBAL_FEATS over a graph of one path row (sb_pool: mean = max = the row; the padding rows pool apart)."""
    c = sc.case("mvalid")
    model, step, kw = _build("mvalid", dict(node_embedding_size=H, global_feats=True, bl_features=True),
                             readout=readout)
    assert step.args.pool_w == 8
    _check("C.4", "mvalid", model, step, kw, c.batches[1], tag=(H, readout, "global_feats"))


@edge_grid
def test_large_tiny_large(H, readout):
    """large -> 1-path -> large from one capture, each step against the oracle: the tiny step leaves the scratch rows
    past its own untouched (stale from the large batch), the second large step rewrites all it reads — its gradients
    are bitwise those of the first."""
    c = sc.case("mvalid")
    model, step, kw = _build("mvalid", dict(node_embedding_size=H), readout=readout)
    first, _ = _check("C.4", "mvalid", model, step, kw, c.batches[0], replay=False, tag=(H, readout, "large"))
    _check("C.4", "mvalid", model, step, kw, c.batches[1], replay=False, tag=(H, readout, "tiny"))
    again, _ = _check("C.4", "mvalid", model, step, kw, c.batches[0], replay=False, tag=(H, readout, "large again"))
    for n in first:
        assert torch.equal(first[n], again[n]), n
