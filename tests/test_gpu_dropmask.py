"""The fused small-batch step's dropout (csrc/hgin_smallbatch.hip drop_factor; models.py:358-359) pinned bit for bit to
its host restatement, oracle/dropout_np.py (itself pinned by tests/test_dropmask_host.py): the masks come from
(drop_seed, the step counter, layer, type, element) alone, computed on the host — no test here reads a mask back from
an output of the step.

Every step reads ``step.args.drop_seed`` and ``step.drop_ctr`` before it runs and asserts that the counter advanced by
exactly one after it.  The CPU oracle (oracle/pyg_cpu.py, float64) runs on the host-collated batch with
``torch.nn.functional.dropout`` replaced by those masks (tests/smallbatch_cases.py HostDropout), and the step is held to

* every element the host mask drops being an exact 0 in ``step.act`` (all layers, all three types, valid rows);
* every (layer, type) block of ``step.act`` — the kept elements' values and the last layer's link / node blocks, which
  feed nothing and so never show in a loss or a gradient — matching what the oracle's dropout returned;
* the loss (1e-5 relative) and every gradient (1e-4 of its norm) of tests/smallbatch_cases.py's check_step.

The stores are 10 - 12 cfg1 graphs at 0.5 - 1.5 of cfg1's 600 / 300 / 100 rows, the batches 1 - 4 of them: up to
~2400 path rows, many 32-row (hidden < 64) and 8-row (hidden >= 64) forward blocks past the first."""
import pytest
import torch

from hgin import HetroGAT, HetroGIN
from hgin.store import GraphStore

import smallbatch_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda"

# The activation bound: per case 8 x the worst (layer, type) block error |fp32 - fp64| / |fp64| of torch's own
# float32 evaluation of the oracle against its float64 evaluation, both under the same host masks, on the same batch
# (measured on the CPU over the drop seeds 1, 2, 3 and the counter 1; the fused kernels sum the same products in
# another order, hence the factor).  (hidden, layers, p, measured worst ratio)
GIN_CASES = [(8, 2, 0.3, 1.34e-7), (8, 2, 0.1, 1.35e-7), (64, 1, 0.5, 7.91e-8), (96, 3, 0.3, 2.21e-7),
             (128, 2, 0.3, 2.23e-7)]   # bounds 1.07e-6, 1.08e-6, 6.33e-7, 1.77e-6, 1.78e-6
GIN_STORE, GIN_IDS, GIN_WARM = dict(n=10, seed=61), (2, 7, 4), (0, 1)
# (heads, C, measured worst ratio) at p = 0.3 (the oracle's projections and attention vectors glorot-initialised on the
# host as GATConv.reset_parameters does, its biases zero: the HIP model's lazy projections only materialise on a device)
GAT_CASES = [(16, 8, 8.53e-8), (4, 16, 9.17e-8), (32, 4, 8.15e-8)]   # bounds 6.82e-7, 7.34e-7, 6.52e-7
GAT_STORE, GAT_IDS, GAT_WARM = dict(n=8, seed=67), (1, 6, 3), (0, 2)
ACT_FACTOR = 8.0


def _store(n, seed):
    return GraphStore.build(sc.store_graphs(n, seed), device=DEV, normalize=True)


def _build(kw, store, batch_size, warm, gat=False, lr=0.0, weight_decay=0.0, readout="auto"):
    """(model, step): the HIP model from seed 1997 and its captured fused step after one warm-up step."""
    from hgin.smallbatch import SmallBatchStep
    torch.manual_seed(1997)
    model = (HetroGAT if gat else HetroGIN)(**dict(kw, input_channels=dict(kw["input_channels"]))).to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=weight_decay, capturable=True)
    step = SmallBatchStep(model, opt, store, batch_size=batch_size, warmup_ids=[list(warm)], warmup=1, readout=readout)
    torch.cuda.synchronize()
    from oracle import dropout_np
    assert step.folded and step.args.drop_thr == dropout_np.drop_threshold(kw["dropout"])
    return model, step


def _rows(b):
    return {t: b.x[t].shape[0] for t in sc.TYPES}


def _step(step, ids):
    """One fused step: (loss, the counter its masks were drawn at).  The counter is read before the step and must
    have advanced by exactly one after it."""
    torch.cuda.synchronize()
    ctr = int(step.drop_ctr)
    lv = float(step.step(list(ids)))
    torch.cuda.synchronize()
    assert int(step.drop_ctr) == ctr + 1
    return lv, ctr


def _step_vs_oracle(model, step, kw, store, ids, monkeypatch, hd=None, gat=False, check_grads=None, act_ratio=None):
    """One fused step at lr 0 against the float64 oracle under the host masks of the step's counter: first the masks
    (every dropped element an exact 0; with ``act_ratio`` every block of step.act against the oracle's dropout output,
    _check_act), then loss and gradients — so a wrong mask is reported as one.  Returns (loss, ctr, the host dropout,
    the host batch's rows per type, the oracle, the step's blocks)."""
    torch.cuda.synchronize()
    ref = sc.oracle_twin(model, kw, torch.float64, gat)   # (before the step: MLP_BN's running statistics move)
    seed = int(step.args.drop_seed)
    lv, ctr = _step(step, ids)
    b = sc.host_batch(store, ids)
    n = _rows(b)
    if hd is None:
        hd = sc.host_dropout(monkeypatch, seed, ctr, kw["dropout"], n, step.args.H)
    else:
        assert hd.seed == seed
        hd.at(ctr, n)
    lv_ref = sc.oracle_step(ref, b)
    assert hd.calls == {ti: step.args.L for ti in range(3)}
    blocks = _check_act(step, hd, n, act_ratio)
    if check_grads is None:
        sc.check_step(model, ref, lv, lv_ref, bn=kw["mlp_bn"], tag=(tuple(ids), ctr))
    else:
        assert abs(lv - lv_ref) <= sc.LOSS_TOL * abs(lv_ref), (lv, lv_ref)
        check_grads(model, ref)
    return lv, ctr, hd, n, ref, blocks


def _check_act(step, hd, n, ratio=None):
    """The strict-zero check of the step that ``hd`` stands at over every (layer, type) block of step.act and, given
    the case's measured ``ratio``, the activation check: each block within ACT_FACTOR x ratio of what the oracle's
    dropout returned for it, |got - want| / |want| over the block.  Returns the blocks."""
    blocks = sc.act_blocks(step, n)
    sc.check_dropped_zero(blocks, hd)
    if ratio is not None:
        errs = sc.act_errors(blocks, hd.out)
        print("activation errors", {k: f"{v:.3g}" for k, v in errs.items()}, "bound", ACT_FACTOR * ratio)
        assert max(errs.values()) <= ACT_FACTOR * ratio, (errs, ACT_FACTOR * ratio)
    return blocks


@pytest.mark.parametrize("hidden,layers,p,ratio", GIN_CASES)
def test_dropout_masks_and_activations(hidden, layers, p, ratio, monkeypatch):
    """GIN at (hidden, layers, p): hidden 8 runs the scalar forward k_sb_fwd<false> (the factor at q = (r0 + ii) H + h)
    and the scalar weight-gradient kernel; hidden 64, 96 and 128 run the MFMA forward k_sb_fwd<true> (selected by
    H >= 64: 8-row blocks, the factor applied with the last relation into the type at q = r0 H + idx) and the MFMA
    weight-gradient kernel k_sb_bwd_w<true> (through gout()).  96 x 3 has a middle layer whose link / node outputs are
    live; 64 x 1's only layer is the last, whose link / node blocks feed nothing and show in the activation check alone.

    After one step at lr 0: the dropped elements are exact zeros, every block of step.act is within 8 x the float32
    oracle's own error of the float64 oracle's dropout output (measured worst block per case, GIN_CASES' last column:
    8 x that is the bound), loss and gradients pass check_step.  The same batch again: the counter advances once
    more, the new blocks are zero where the host mask of that counter says, and the zero patterns differ."""
    store = _store(**GIN_STORE)
    kw = sc.model_kwargs(node_embedding_size=hidden, message_passing_layers=layers, dropout=p)
    model, step = _build(kw, store, 4, GIN_WARM)
    assert (step.args.H >= sc.MFMA_MIN_H) == (hidden >= 64) and step.args.L == layers
    lv, ctr, hd, n, _, blocks = _step_vs_oracle(model, step, kw, store, GIN_IDS, monkeypatch, act_ratio=ratio)
    assert min(n.values()) > 3 * sc.FWD_ROWS   # several forward blocks per type: r0 > 0
    lv2, ctr2 = _step(step, GIN_IDS)
    assert ctr2 == ctr + 1 and lv2 != lv
    blocks2 = sc.act_blocks(step, n)
    sc.check_dropped_zero(blocks2, hd, ctr2)
    for k in blocks:
        assert not torch.equal(blocks[k] == 0, blocks2[k] == 0), k


@pytest.mark.parametrize("variant", ["mlp_bn_h128", "global_feats_h8", "no_concat_h128", "scalar_readout_h8"])
def test_dropout_variants_vs_oracle(variant, monkeypatch):
    """Dropout 0.3 with MLP_BN (also its running statistics: check_buffers), GLOBAL_FEATS, CONCAT_PATH off and the
    scalar readout, at hidden 8 (scalar kernels) and hidden 128 (k_sb_fwd<true>, k_sb_bwd_w<true> with the factor
    through gout()), two layers: loss, gradients and dropped zeros against the float64 oracle under the host masks."""
    over, readout = {"mlp_bn_h128": (dict(mlp_bn=True, node_embedding_size=128), "auto"),
                     "global_feats_h8": (dict(global_feats=True, bl_features=True), "auto"),
                     "no_concat_h128": (dict(concat_path=False, node_embedding_size=128), "auto"),
                     "scalar_readout_h8": ({}, "scalar")}[variant]
    store = _store(n=8, seed=71)
    kw = sc.model_kwargs(dropout=0.3, **over)
    model, step = _build(kw, store, 4, (0, 2), readout=readout)
    assert step.args.ro_wlds in ((3,) if kw["mlp_bn"] else (1,) if readout == "scalar" else (2, 4))
    assert bool(step.args.pool_w) == kw["global_feats"] and bool(step.args.concat_path) == kw["concat_path"]
    ref = _step_vs_oracle(model, step, kw, store, (1, 6, 3), monkeypatch)[4]
    if kw["mlp_bn"]:
        sc.check_buffers(model, ref)


def test_dropout_ragged_replays_vs_oracle(monkeypatch):
    """One capture of capacity 4 with dropout 0.3 replayed on 1, 4, 2 and 3 graphs: each step against the oracle under
    the host masks of its own counter (the mask of an element does not depend on the batch's rows or the capacity),
    the counter advancing by exactly one per replay."""
    store = _store(n=10, seed=73)
    kw = sc.model_kwargs(dropout=0.3)
    model, step = _build(kw, store, 4, (0, 1, 2, 3))
    hd, ctrs = None, []
    for ids in ((5,), (1, 2, 3, 4), (7, 0), (9, 6, 8)):
        _, ctr, hd = _step_vs_oracle(model, step, kw, store, ids, monkeypatch, hd)[:3]
        ctrs.append(ctr)
    assert ctrs == list(range(ctrs[0], ctrs[0] + 4))


def test_dropout_trajectory_vs_oracle(monkeypatch):
    """Five batches with the folded Adam (lr 1e-3, weight decay 1e-2) and dropout 0.3 against
    oracle.pyg_cpu.train_step (float64) under torch's Adam, each oracle step under the host masks of the fused step's
    counter: every loss within 1e-4 relative (tests/test_gpu_smallbatch.py's trajectory bound)."""
    from oracle.pyg_cpu import train_step
    graphs = sc.store_graphs(12, 79)
    store = GraphStore.build(graphs, device=DEV, normalize=True)
    seq = [(1, 6, 10), (4, 0, 11), (8, 3, 5), (9, 7, 2), (3, 10, 1)]
    kw = sc.model_kwargs(dropout=0.3)
    torch.manual_seed(1997)
    model = HetroGIN(**dict(kw, input_channels=dict(kw["input_channels"]))).to(DEV)
    ref = sc.oracle_twin(model, kw, torch.float64)   # (the parameters the warm-up step starts from)
    from hgin.smallbatch import SmallBatchStep
    o1 = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-2, capturable=True)
    step = SmallBatchStep(model, o1, store, batch_size=3, warmup_ids=[list(seq[0])], warmup=1)
    assert step.folded
    o2 = torch.optim.Adam(ref.parameters(), lr=1e-3, weight_decay=1e-2)
    hb = {ids: sc.host_batch(store, ids) for ids in seq}
    hd = sc.host_dropout(monkeypatch, int(step.args.drop_seed), 0, 0.3, _rows(hb[seq[0]]), step.args.H)

    def oracle(ids, ctr):
        b = hb[ids]
        hd.at(ctr, _rows(b))
        return float(train_step(ref, o2, {t: v.double() for t, v in b.x.items()}, b.edge_index_dict(),
                                b.batch["path"], b.y.double()))
    torch.cuda.synchronize()
    assert int(step.drop_ctr) == 1   # the warm-up step drew at counter 0 (the capture itself runs nothing)
    oracle(seq[0], 0)
    for k, ids in enumerate(seq):
        got, ctr = _step(step, ids)
        want = oracle(ids, ctr)
        sc.check_dropped_zero(sc.act_blocks(step, _rows(hb[ids])), hd)
        assert abs(got - want) <= 1e-4 * abs(want), (k, got, want)


@pytest.mark.parametrize("heads,C,ratio", GAT_CASES)
def test_dropout_gat_masks_and_activations(heads, C, ratio, monkeypatch):
    """HetroGAT (one layer of GATConvs, k_sb_gat_fwd / k_sb_gat_bwd) with dropout 0.3, the GATConv biases at their
    initial zeros: a destination row without edges outputs an exact 0 whether kept or not, which the host masks do not
    care about.  The dropped elements are exact zeros, the layer's three blocks within 8 x the float32 oracle's own
    error (GAT_CASES' last column) of the float64 oracle's dropout output, the loss within 1e-5 relative and the
    gradients within tests/test_gpu_smallbatch_gat.py's _check_grads."""
    from test_gpu_smallbatch_gat import _check_grads
    store = _store(**GAT_STORE)
    kw = sc.gat_kwargs(heads=heads, node_embedding_size=C, dropout=0.3)
    model, step = _build(kw, store, 4, GAT_WARM, gat=True)
    assert step.gat and step.args.H == heads * C
    for conv in model.convs[0].convs.values():
        assert not conv.bias.detach().any()
    _step_vs_oracle(model, step, kw, store, GAT_IDS, monkeypatch, gat=True, check_grads=_check_grads, act_ratio=ratio)
