"""Shared case builder of the fused small-batch step's shape tests (tests/test_smallbatch_shapes_host.py,
tests/test_gpu_smallbatch_edges.py; the oracle comparison also serves tests/test_gpu_smallbatch.py, the host dropout
masks tests/test_gpu_dropmask.py and the two files' dropout tests): small
deterministic graphs whose row counts and degrees are prescribed exactly, a Python mirror of the staging arithmetic of
csrc/hgin_smallbatch.hip's weight-gradient loops (so that a test can assert that its case reaches the loop iteration it
claims to reach), the host collation pinned to oracle/collate_np.py, and the comparison of one fused step with the CPU
oracle.  Nothing here touches a device; everything is deterministic from its seed.

The reference of the shape tests is ``OracleHetroGIN`` / ``OracleHetroGAT`` (oracle/pyg_cpu.py) loaded with the HIP
model's parameters and run in float64 (module and inputs ``.double()``) on the host-collated batch: every part of the
oracle runs in float64, so no case falls back to fp32.

Error measures: a ratio <= 1 means "within the tolerance" (tests/test_gpu_smallbatch.py's: the loss within 1e-5
relative, every gradient within 1e-4 of its norm + 1e-9, with MLP_BN + 1e-6 of the largest gradient norm instead)."""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from hgin.data import CONFIGS, REL_LN, REL_LP, REL_NL, REL_PL, HeteroGraph

TYPES = ("path", "link", "node")
LOSS_TOL, GRAD_TOL, GRAD_ABS, BN_SLACK, PRED_TOL = 1e-5, 1e-4, 1e-9, 1e-6, 1e-5

# ---- the staging arithmetic of csrc/hgin_smallbatch.hip -----------------------------------------------------------

K_SB_THREADS = 256               # hgin_smallbatch.hip:45   kSbThreads
K_SB_STAGE = 8192                # hgin_smallbatch.hip:1543 kSbStage (k_sb_bwd_w<false>, ro_weight_part, k_sb_gat_bwd)
K_SB_STAGE_M = 16384             # hgin_smallbatch.hip:1658 kSbStageM (k_sb_bwd_w<true>)
K_SB_RED_M = (K_SB_THREADS // 64) * 32 * 33   # hgin_smallbatch.hip:1658 kSbRedM = 4 * 32 * 33
K_SB_W_LDS = 2048                # hgin_smallbatch.hip:1748 wsz = H K <= 2048 ? H K : 0
K_RO_MO, K_RO_MK = 4, 2          # hgin_smallbatch.hip:1542 kRoMO, kRoMK
MFMA_MIN_H = 64                  # hgin_smallbatch.hip:2422 a.H >= 64 launches k_sb_bwd_w<true>
FWD_ROWS, FWD_ROWS_M = 32, 8     # hgin_smallbatch.hip:382 kSbFwdRows, :433 kSbFwdRowsM
RO_ROWS, RO_ROWS_M = 8, 32       # hgin_smallbatch.hip:46 kSbRows, :913 kSbRowsM


def stage_rows(kind: str, H: int, K: int, N: int = 0) -> int:
    """rcap: the most rows one staging block holds.  kind "gin": k_sb_bwd_w of a conv with H outputs and K inputs (the
    scalar kernel below H = 64, the MFMA kernel from there on); "readout": ro_weight_part of a layer with N outputs and
    K inputs (the head: N = 1); "gat": k_sb_gat_bwd's rows per pass with H heads."""
    if kind == "gin":
        if H >= MFMA_MIN_H:
            return (K_SB_STAGE_M - K_SB_RED_M) // ((H | 1) + (K | 1))   # hgin_smallbatch.hip:1686-1687
        wsz = H * K if H * K <= K_SB_W_LDS else 0                       # hgin_smallbatch.hip:1748
        return (K_SB_STAGE - wsz) // (H + K)                            # hgin_smallbatch.hip:1749
    if kind == "readout":
        return K_SB_STAGE // (N + K)                                    # hgin_smallbatch.hip:1630
    if kind == "gat":
        return K_SB_THREADS // H                                        # hgin_smallbatch.hip:1927 gat_rows_per_pass
    raise ValueError(kind)


def staging_blocks(rows: int, n_parts: int, kind: str, H: int, K: int, N: int = 0) -> int:
    """How many ``rb`` iterations (``for (rb = i0; rb < i1; rb += RS)``) the fullest row chunk of ``rows`` rows takes:
    chunk 0 holds min(ceil(rows / n_parts), rows) rows (hgin_smallbatch.hip:1619-1620, :1675-1676, :2085), staged
    RS = min(chunk, rcap) rows at a time (:1631, :1688, :1750).  0 for an empty chunk."""
    ch = -(-rows // n_parts)
    chunk = min(ch, rows)
    if chunk <= 0:
        return 0
    rs = min(chunk, stage_rows(kind, H, K, N))
    return -(-chunk // rs)


def empty_chunks(rows: int, n_parts: int) -> int:
    """The row chunks with i1 <= i0 (the MFMA kernel's zero fill, the scalar kernels' untouched zero WgTile)."""
    ch = max(-(-rows // n_parts), 1)
    return n_parts - min(n_parts, -(-rows // ch))


def weight_groups(N: int, K: int) -> int:
    """ro_groups_nk (hgin_smallbatch.hip:1545-1553): the register-tile groups ``u`` of an [N][K + 1] weight gradient;
    every group past the first stages the chunk's rows again."""
    t = 1
    while t < K_SB_THREADS and K_RO_MO * t < N:
        t *= 2
    tk = K_SB_THREADS // t
    return (K + 1 + K_RO_MK * tk - 1) // (K_RO_MK * tk)


def final_idle_groups(n_parts: int) -> int:
    """k_sb_final's 8 lane groups with np = (n_parts - g + 7) / 8 == 0 (hgin_smallbatch.hip:1887)."""
    return sum(1 for g in range(8) if (n_parts - g + 7) // 8 == 0)


# ---- models ------------------------------------------------------------------------------------------------------

def model_kwargs(**over) -> dict:
    """HetroGIN's constructor arguments as train.py passes them for cfg1 (a fresh input_channels dict per call: the
    constructor edits it in place, as the reference does), with overrides."""
    cfg = CONFIGS["cfg1"]
    return dict(cfg.model_kwargs({"link": cfg.f_link, "path": cfg.f_path, "node": cfg.f_node}), **over)


def gat_kwargs(**over) -> dict:
    """config.json's MODEL == "GAT" shape: HEADS 16, NODE_EMBEDDING_SIZE 8, MP_LAYERS 1."""
    return model_kwargs(**dict(dict(heads=16, node_embedding_size=8, message_passing_layers=1), **over))


def feature_widths(kw: dict) -> Dict[str, int]:
    """The sliced input columns per type (models.py:333-342) of the 7 / 7 / 3 layout."""
    p, l = 7, 7
    if not kw["divided_features"]:
        p, l = p - 3, l - 1
    if not kw["bl_features"]:
        p, l = p - 1, l - 3
    return {"path": p, "link": l, "node": 3}


def conv_widths(kw: dict) -> List[Tuple[int, int, str]]:
    """(H, K, destination type) of every GIN conv of the model, layer by layer in relation order."""
    f, H = feature_widths(kw), kw["node_embedding_size"]
    out = []
    for l in range(kw["message_passing_layers"]):
        for s, _, d in (REL_PL, REL_LP, REL_LN, REL_NL):
            out.append((H, f[s] + f[d] if l == 0 else H, d))
    return out


def readout_widths(kw: dict, H: Optional[int] = None) -> List[Tuple[int, int]]:
    """(N, K) of every readout layer, the head (N = 1) last; H: the conv output width (heads x C for HetroGAT)."""
    H = kw["node_embedding_size"] if H is None else H
    k = H + (feature_widths(kw)["path"] if kw["concat_path"] else 0) + (8 if kw["global_feats"] else 0)
    out = []
    for n in kw["mlp_layers"]:
        out.append((n, k))
        k = n
    return out + [(1, k)]


def oracle_twin(model, kw: dict, dtype=torch.float64, gat: bool = False):
    """The CPU oracle with the HIP model's parameters and buffers, in ``dtype``.  kw: the model's constructor arguments
    (HetroGAT: gat_kwargs; its lazy projections must be materialised)."""
    from oracle.pyg_cpu import OracleHetroGAT, OracleHetroGIN
    if gat:
        dims = {}
        for key, conv in model.convs[0].convs.items():
            s, _, d = key.split("__")
            dims[s], dims[d] = conv.lin_src.weight.shape[1], conv.lin_dst.weight.shape[1]
        ref = OracleHetroGAT(dims, kw["node_embedding_size"], kw["heads"], kw["dropout"], kw["concat_path"],
                             kw["bl_features"], kw["divided_features"], kw["global_feats"], list(kw["mlp_layers"]),
                             kw["act"], kw["mlp_head_act"], kw["mlp_bn"])
    else:
        kw = dict(kw, input_channels=dict(kw["input_channels"]), mlp_layers=list(kw["mlp_layers"]))
        kw.pop("heads", None)
        ref = OracleHetroGIN(**kw)
    ref.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
    return ref.to(dtype)


# ---- collation and the oracle comparison -------------------------------------------------------------------------

def assert_collation(b: HeteroGraph, singles: Sequence[HeteroGraph]) -> None:
    """``b`` (on the host) is the numpy restatement of PyG's ``Batch.from_data_list`` of ``singles``, bit for bit."""
    from oracle import collate_np
    want = collate_np.collate([collate_np.from_graph(g) for g in singles])
    for t in b.x:
        assert torch.equal(b.x[t], torch.from_numpy(want["x"][t])), t
        assert torch.equal(b.batch[t], torch.from_numpy(want["batch"][t])), t
    for r in b.edge_index:
        assert torch.equal(b.edge_index[r], torch.from_numpy(want["edge_index"][r])), r
    assert torch.equal(b.y, torch.from_numpy(want["y"]))


def host_batch(store, ids) -> HeteroGraph:
    """The batch ``ids`` of a GraphStore on the host, pinned to oracle/collate_np.py's collation of the same graphs."""
    b = store.collate(ids).to("cpu")
    assert_collation(b, [store.collate([i]).to("cpu") for i in ids])
    return b


def oracle_forward(ref, b: HeteroGraph):
    """(predictions, MAPE) of the oracle on the host batch, in the oracle's own dtype."""
    from oracle.pyg_cpu import mape
    dt = next(ref.parameters()).dtype
    out = ref({t: v.to(dt) for t, v in b.x.items()}, b.edge_index_dict(), b.batch["path"])
    return out, mape(out, b.y.to(dt).reshape(-1, 1))


def oracle_step(ref, b: HeteroGraph) -> float:
    """The oracle's forward and sqrt-MAPE backward (train.py:31-44 without the optimizer) on the host batch; returns
    the loss value, the gradients stay on ``ref``'s parameters."""
    for q in ref.parameters():
        q.grad = None
    _, lv = oracle_forward(ref, b)
    torch.sqrt(lv).backward()
    return float(lv.detach())


def grad_of(p) -> torch.Tensor:
    """A fused-step parameter's gradient; the dead convs' parameters keep .grad None, as in the reference."""
    return p.grad.detach() if p.grad is not None else torch.zeros_like(p.detach())


def grad_norms(ref) -> Dict[str, Optional[float]]:
    """Per parameter the norm of the oracle's gradient, None where autograd left none (the dead convs)."""
    return {n: None if q.grad is None else float(q.grad.double().norm()) for n, q in ref.named_parameters()}


def check_step(model, ref, lv: float, lv_ref: float, bn: bool = False, tag=None) -> float:
    """One fused step against the oracle after ``oracle_step``: the loss within 1e-5 relative; per parameter .grad is
    None exactly where the oracle's is (the dead convs) and within 1e-4 of the oracle's norm + 1e-9 (``bn``: + 1e-6 of
    the largest gradient norm instead: the Linear biases ahead of a BatchNorm have a zero true gradient).  Returns the
    worst error / tolerance."""
    assert abs(lv - lv_ref) <= LOSS_TOL * abs(lv_ref), (tag, lv, lv_ref)
    worst = abs(lv - lv_ref) / (LOSS_TOL * abs(lv_ref))
    gmax = max(float(q.grad.double().norm()) for q in ref.parameters() if q.grad is not None)
    slack = BN_SLACK * gmax if bn else GRAD_ABS
    for (n, p), (n2, q) in zip(model.named_parameters(), ref.named_parameters()):
        assert n == n2
        assert (p.grad is None) == (q.grad is None), (tag, n)   # the dead convs: no gradient on either side
        want = q.grad if q.grad is not None else torch.zeros_like(q)
        d = float((grad_of(p).cpu().double() - want.double()).norm())
        bound = GRAD_TOL * float(want.double().norm()) + slack
        assert d <= bound, (tag, n, d, float(want.norm()))
        worst = max(worst, d / bound)
    return worst


def fp32_ratio(model, kw: dict, b: HeteroGraph, gat: bool = False) -> float:
    """torch's own fp32 evaluation of the oracle against its float64 evaluation on the host batch ``b``, in
    check_step's measure: the worst error / tolerance over the loss and the gradients.  A condition on the inputs (as
    tests/gat_cases.py's) where a case is ill-conditioned by construction: MLP_BN over two rows cancels to
    eps / (var + eps) of its terms, the host test asserts <= 0.25 for it, and if a seed misses that, the seed
    changes, never the tolerance."""
    r64, r32 = oracle_twin(model, kw, torch.float64, gat), oracle_twin(model, kw, torch.float32, gat)
    l64, l32 = oracle_step(r64, b), oracle_step(r32, b)
    worst = abs(l32 - l64) / (LOSS_TOL * abs(l64))
    gmax = max(float(q.grad.norm()) for q in r64.parameters() if q.grad is not None)
    slack = BN_SLACK * gmax if kw["mlp_bn"] else GRAD_ABS
    for p, q in zip(r32.parameters(), r64.parameters()):
        if q.grad is not None:
            worst = max(worst, float((p.grad.double() - q.grad).norm()) / (GRAD_TOL * float(q.grad.norm()) + slack))
    return worst


def check_buffers(model, ref) -> None:
    """MLP_BN's running statistics and num_batches_tracked after the same step (tests/test_gpu_smallbatch.py's bound)."""
    for (n, u), (n2, v) in zip(model.named_buffers(), ref.named_buffers()):
        assert n == n2
        if v.dtype == torch.int64:
            assert torch.equal(u.cpu(), v), n
        else:
            assert torch.allclose(u.cpu().double(), v.double(), rtol=1e-5, atol=1e-6), \
                (n, float((u.cpu() - v).abs().max()))


# ---- dropout: the step's masks restated on the host ----------------------------------------------------------------

def store_graphs(n: int, seed: int) -> List[HeteroGraph]:
    """``n`` cfg1 graphs scaled by factors drawn in [0.5, 1.5) (tests/test_gpu_smallbatch.py's ``_store``, on the
    host): what a test hands to GraphStore.build(..., normalize=True)."""
    import numpy as np

    from hgin.data import scaled_config, synthetic_graph
    rng = np.random.default_rng(seed)
    cfg = CONFIGS["cfg1"]
    return [synthetic_graph(scaled_config(cfg, float(rng.uniform(0.5, 1.5)), name=f"g{i}"), seed=seed * 100 + i)
            for i in range(n)]


def store_host_batch(graphs: Sequence[HeteroGraph], ids) -> HeteroGraph:
    """The batch ``ids`` of the normalised store of ``graphs`` formed on the host alone (hgin.data.collate, then
    dataset.py:33-58's per-column normalisation, which is row by row what the store applies to all its rows)."""
    from hgin.data import collate
    from hgin.store import normalize_reference
    b = collate([graphs[i] for i in ids])
    return HeteroGraph(normalize_reference(b.x), b.edge_index, b.y, b.batch)


class HostDropout:
    """``torch.nn.functional.dropout`` replaced by the fused step's own masks, computed on the host by
    oracle/dropout_np.py from (seed, step counter, layer, type, element) alone: nothing here reads an output of the
    step.  The oracle calls F.dropout once per node type after every layer (models.py:358-359); the type is told by the
    row count (the three must differ), the layer by counting the calls per type.  ``out[(l, t)]`` keeps what the
    oracle's dropout returned for layer l and type index t (0 / 1 / 2 = path / link / node), detached.

    One oracle forward per ``at(ctr)``: it sets the step counter whose masks apply and restarts the layer count."""

    def __init__(self, seed: int, p: float, rows_by_type: Dict[str, int], H: int):
        rows = [rows_by_type[t] for t in TYPES]
        assert len(set(rows)) == 3, rows
        self.seed, self.p, self.rows, self.H = int(seed), float(p), rows, int(H)
        self.ctr, self.calls, self.out = None, {}, {}

    def at(self, ctr: int, rows_by_type: Optional[Dict[str, int]] = None) -> "HostDropout":
        if rows_by_type is not None:   # (another batch of the same capture)
            self.rows = [rows_by_type[t] for t in TYPES]
            assert len(set(self.rows)) == 3, self.rows
        self.ctr, self.calls, self.out = int(ctr), {}, {}
        return self

    def keep(self, l: int, ti: int, ctr: Optional[int] = None) -> torch.Tensor:
        """[rows of type ti][H] bool: the elements of layer l's type-ti output that the step ``ctr`` keeps."""
        from oracle import dropout_np
        return torch.from_numpy(dropout_np.keep_mask(self.seed, self.ctr if ctr is None else ctr, l, ti,
                                                     self.rows[ti], self.H, self.p))

    def __call__(self, x, p=0.5, training=True, inplace=False):
        from oracle import dropout_np
        assert training and not inplace and p == self.p and x.shape[1] == self.H and self.ctr is not None
        ti = self.rows.index(x.shape[0])
        l = self.calls.get(ti, 0)
        self.calls[ti] = l + 1
        y = x * (self.keep(l, ti).to(x.dtype) * dropout_np.drop_scale(self.p))
        self.out[(l, ti)] = y.detach().clone()
        return y


def host_dropout(monkeypatch, seed: int, ctr: int, p: float, rows_by_type: Dict[str, int], H: int) -> HostDropout:
    """Patch torch.nn.functional.dropout with the host masks of the step ``ctr`` (HostDropout) for the test's duration."""
    hd = HostDropout(seed, p, rows_by_type, H).at(ctr)
    monkeypatch.setattr(torch.nn.functional, "dropout", hd)
    return hd


def act_blocks(step, rows_by_type: Dict[str, int]) -> Dict[Tuple[int, int], torch.Tensor]:
    """(l, type index) -> the valid rows [n_t][H] of the step's layer outputs (``step.act``), on the host."""
    a, act = step.args, step.act.detach().cpu()
    out = {}
    for l in range(a.L):
        for ti, t in enumerate(TYPES):
            o, n = a.act_off[l][ti], rows_by_type[t]
            out[(l, ti)] = act[o:o + n * a.H].view(n, a.H).clone()
    return out


def check_dropped_zero(blocks, hd: HostDropout, ctr: Optional[int] = None) -> None:
    """Every element that the host mask of the step drops is an exact 0 in the step's layer outputs (no cap: one
    surviving element fails).  Kept elements may be 0 too (a row without edges and a zero bias): not asserted."""
    for (l, ti), blk in blocks.items():
        dropped = ~hd.keep(l, ti, ctr)
        assert dropped.shape == blk.shape, (l, ti)
        bad = int((blk[dropped] != 0).sum())
        assert bad == 0, (l, ti, bad, int(dropped.sum()))


def act_errors(blocks, want) -> Dict[Tuple[int, int], float]:
    """Per (l, type index) block |got - want| / |want| (norms over the block, in float64)."""
    assert sorted(blocks) == sorted(want), (sorted(blocks), sorted(want))
    return {k: float((blocks[k].double() - want[k].double()).norm() / want[k].double().norm()) for k in blocks}


def fp32_act_ratio(make_ref, b: HeteroGraph, p: float, H: int, seeds=(1, 2, 3), ctr: int = 1) -> float:
    """The yardstick of the activation check: torch's own float32 evaluation of the oracle against its float64
    evaluation on the host batch ``b``, both under the same host masks — the worst act_errors block over the drop
    ``seeds``.  make_ref(dtype) builds the oracle in that dtype from one set of parameters."""
    from unittest import mock
    n = {t: b.x[t].shape[0] for t in TYPES}
    r64, r32 = make_ref(torch.float64), make_ref(torch.float32)
    worst = 0.0
    for seed in seeds:
        hd = HostDropout(seed, p, n, H)
        outs = []
        with mock.patch.object(torch.nn.functional, "dropout", hd):
            for ref in (r64, r32):
                hd.at(ctr)
                with torch.no_grad():
                    oracle_forward(ref, b)
                outs.append(hd.out)
        worst = max(worst, max(act_errors(outs[1], outs[0]).values()))
    return worst


def glorot_gat_oracle(kw: dict):
    """OracleHetroGAT for ``kw`` (gat_kwargs) with its projections and attention vectors glorot-initialised and its
    biases zero, as GATConv.reset_parameters leaves them (the HIP model's lazy projections materialise on a device
    only); deterministic from torch's seed 1997."""
    from oracle.pyg_cpu import OracleHetroGAT
    torch.manual_seed(1997)
    ref = OracleHetroGAT(feature_widths(kw), kw["node_embedding_size"], kw["heads"], kw["dropout"], kw["concat_path"],
                         kw["bl_features"], kw["divided_features"], kw["global_feats"], list(kw["mlp_layers"]),
                         kw["act"], kw["mlp_head_act"], kw["mlp_bn"])
    for conv in ref.convs[0].convs.values():
        for w in (conv.att_src, conv.att_dst, conv.lin_src.weight, conv.lin_dst.weight):
            torch.nn.init.xavier_uniform_(w)
    return ref


def check_eval(pred: torch.Tensor, lv: float, out_ref: torch.Tensor, lv_ref: float, tag=None) -> float:
    """SmallBatchEval's loss (1e-5 relative) and predictions (1e-5 abs + rel) against the eval-mode oracle."""
    assert abs(lv - lv_ref) <= LOSS_TOL * abs(lv_ref), (tag, lv, lv_ref)
    got, want = pred.detach().cpu().double().reshape(-1), out_ref.detach().double().reshape(-1)
    r = float(((got - want).abs() / (PRED_TOL + PRED_TOL * want.abs())).max())
    assert r <= 1.0, (tag, r)
    return max(r, abs(lv - lv_ref) / (LOSS_TOL * abs(lv_ref)))


# ---- adversarial graphs ------------------------------------------------------------------------------------------

def _span(n: int, isolated_ends: bool) -> Tuple[int, int]:
    """The rows [lo, hi) of a type that may carry edges: all of them, or all but the first and the last."""
    return (1, n - 1) if isolated_ends and n >= 3 else (0, n)


def make_graph(n_path: int, n_link: int, n_node: int, seed: int, e_pl: Optional[int] = None,
               e_ln: Optional[int] = None, hub_link: bool = False, hub_path: int = 0, isolated_ends: bool = False
               ) -> HeteroGraph:
    """One graph in cfg1's 7 / 7 / 3 feature layout (features randn, y = rand + 0.5 in [0.5, 1.5], as
    hgin.data.synthetic_graph draws them) with exactly the requested rows per type and ``e_pl`` path -> link and
    ``e_ln`` link -> node edges with uniform endpoints (defaults 3 n_path and 2 n_link; the reverse relations are their
    flips), plus:

    * ``isolated_ends``: the first and the last row of every type with >= 3 rows carry no edge in any relation;
    * ``hub_link``: link n_link // 2 is used by every path that may carry edges (one more edge each);
    * ``hub_path`` = d: path n_path // 2 uses d more links, drawn with replacement (duplicates are separate edges);
    * ``e_ln`` = 0: the link -> node / node -> link pair is empty ([2, 0])."""
    g = torch.Generator().manual_seed(seed)
    pl0, pl1 = _span(n_path, isolated_ends)
    ll0, ll1 = _span(n_link, isolated_ends)
    nl0, nl1 = _span(n_node, isolated_ends)
    ri = lambda lo, hi, n: torch.randint(lo, hi, (n,), generator=g, dtype=torch.long)   # noqa: E731
    e_pl = 3 * n_path if e_pl is None else e_pl
    e_ln = 2 * n_link if e_ln is None else e_ln
    src, dst = [ri(pl0, pl1, e_pl)], [ri(ll0, ll1, e_pl)]
    if hub_link:
        src.append(torch.arange(pl0, pl1))
        dst.append(torch.full((pl1 - pl0,), n_link // 2, dtype=torch.long))
    if hub_path:
        src.append(torch.full((hub_path,), n_path // 2, dtype=torch.long))
        dst.append(ri(ll0, ll1, hub_path))
    pl = torch.stack([torch.cat(src), torch.cat(dst)])
    pl = pl[:, torch.randperm(pl.size(1), generator=g)].contiguous()
    ln = torch.stack([ri(ll0, ll1, e_ln), ri(nl0, nl1, e_ln)])
    ei = {REL_PL: pl, REL_LP: pl.flip(0).contiguous(), REL_LN: ln, REL_NL: ln.flip(0).contiguous()}
    rn = lambda n, f: torch.randn(n, f, generator=g)   # noqa: E731
    x = {"path": rn(n_path, 7), "link": rn(n_link, 7), "node": rn(n_node, 3)}
    y = torch.rand(n_path, generator=g) + 0.5
    return HeteroGraph(x, ei, y, {t: torch.zeros(x[t].shape[0], dtype=torch.long) for t in TYPES})


@dataclass(frozen=True)
class Case:
    """Graphs for one GraphStore and the batches a test runs from it."""
    name: str
    graphs: tuple          # HeteroGraph per store entry
    batches: tuple         # graph-id lists; batches[0] is also the warm-up batch
    batch_size: int
    normalize: bool        # the store's dataset.py:33-58 normalisation (fixed constants per column)
    hub_link: bool = False
    hub_path: int = 0
    isolated_ends: bool = False

    def totals(self, ids) -> Dict[str, int]:
        return {t: sum(self.graphs[i].x[t].shape[0] for i in ids) for t in TYPES}

    def host_batch(self, ids) -> HeteroGraph:
        """The store's batch formed on the host: hgin.data.collate of the (normalised) graphs."""
        from hgin.data import collate
        from hgin.store import normalize_reference
        b = collate([self.graphs[i] for i in ids])
        return HeteroGraph(normalize_reference(b.x) if self.normalize else b.x, b.edge_index, b.y, b.batch)

    def host_singles(self, ids) -> List[HeteroGraph]:
        return [self.host_batch([i]) for i in ids]


def degrees(g: HeteroGraph, rel, side: int, n: int) -> torch.Tensor:
    """Per row of the relation's source (side 0) or destination (side 1) type its edge count."""
    return torch.bincount(g.edge_index[rel][side], minlength=n)


HUB_DEGREE = 320   # >= 300: 40 rounds of gather_chain's 8 edges

# per-type (path, link, node) rows of the three graphs of a "totals" case; their sums sit on / one past the forward
# blocks (32 rows below H = 64, 8 from there on) and the readout tiles (8 scalar, 32 MFMA)
_TOTALS = {
    "totals_p32k_l32k1_n8k1": ((401, 407, 408), (211, 213, 217), (67, 71, 71)),     # 1216 = 32 38, 641, 209 = 8 26 + 1
    "totals_p32k1_l8k1_n32k": ((401, 407, 409), (203, 205, 209), (73, 75, 76)),     # 1217, 617 = 8 77 + 1, 224 = 32 7
    "totals_p8k1_l32k_n32k1": ((399, 403, 407), (211, 213, 216), (73, 75, 77)),     # 1209 = 8 151 + 1, 640, 225
}
TOTALS_WANT = {"totals_p32k_l32k1_n8k1": (1216, 641, 209), "totals_p32k1_l8k1_n32k": (1217, 617, 224),
               "totals_p8k1_l32k_n32k1": (1209, 640, 225)}
SWEEP_ROWS = ((650, 700, 698), (430, 440, 445), (230, 240, 236))   # 2048 paths, 1315 links, 706 nodes
MVALID_BIG = (2001, 1003, 351)


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    """The named case (built once, shared: callers must not modify its tensors)."""
    if name in _TOTALS:
        p, l, n = _TOTALS[name]
        gs = tuple(make_graph(p[i], l[i], n[i], seed=100 + 10 * len(name) + i) for i in range(3))
        return Case(name, gs, ((2, 0, 1),), 3, True)
    if name == "sweep":   # the staging / partition / width sweeps: uniform edges, enough rows for two staging blocks
        p, l, n = SWEEP_ROWS
        gs = tuple(make_graph(p[i], l[i], n[i], seed=200 + i) for i in range(3))
        return Case(name, gs, ((1, 2, 0),), 3, True)
    if name == "one_node":   # n_node = 1 in every graph: every link -> node edge ends in that row
        gs = tuple(make_graph(300 + 7 * i, 150 + 3 * i, 1, seed=300 + i) for i in range(3))
        return Case(name, gs, ((0, 2, 1),), 3, False)
    if name == "empty_ln":   # no link -> node / node -> link edge in the batch
        gs = tuple(make_graph(300 + 7 * i, 150 + 3 * i, 50 + i, seed=400 + i, e_ln=0) for i in range(3))
        return Case(name, gs, ((1, 0, 2),), 3, True)
    if name == "hub_link":
        gs = tuple(make_graph(330 + 7 * i, 150 + 3 * i, 50 + i, seed=500 + i, hub_link=True, isolated_ends=True)
                   for i in range(3))
        return Case(name, gs, ((2, 1, 0),), 3, True, hub_link=True, isolated_ends=True)
    if name == "hub_path":   # one hub per graph; the batch's other rows have uniform degrees of about 3
        gs = tuple(make_graph(330 + 7 * i, 150 + 3 * i, 50 + i, seed=600 + i, hub_path=HUB_DEGREE, isolated_ends=True)
                   for i in range(3))
        return Case(name, gs, ((0, 1, 2),), 3, True, hub_path=HUB_DEGREE, isolated_ends=True)
    if name == "mvalid":   # capacity from graph 0; graphs 1 and 2 have n_path = 1 and 2 (one-row types: no normalise)
        # (graph 2's seed: one at which MLP_BN over its two rows is conditioned for fp32, see fp32_ratio — at most
        # seeds torch's own fp32 backward misses the tolerance severalfold)
        gs = (make_graph(*MVALID_BIG, seed=700), make_graph(1, 4, 2, seed=701, e_pl=3, e_ln=5),
              make_graph(2, 5, 3, seed=708, e_pl=6, e_ln=7))
        return Case(name, gs, ((0,), (1,), (2,)), 1, False)
    raise KeyError(name)


EDGE_CASES = tuple(_TOTALS) + ("one_node", "empty_ln", "hub_link", "hub_path")
ALL_CASES = EDGE_CASES + ("sweep", "mvalid")

# the sizes of tests/test_gpu_smallbatch.py::test_fused_step_vs_oracle (store seed 11, ids [2, 8, 5, 0]: the rows of
# the batch per type, from hgin.data.scaled_config's rounding of the drawn factors) — see
# tests/test_smallbatch_shapes_host.py, which recomputes them
EXISTING_STORE = dict(n=10, seed=11, ids=(2, 8, 5, 0))


def existing_rows() -> Dict[str, int]:
    """Per type the rows of test_fused_step_vs_oracle's batch (its store's draw restated: no graph is generated)."""
    import numpy as np

    from hgin.data import scaled_config
    rng = np.random.default_rng(EXISTING_STORE["seed"])
    cfg = CONFIGS["cfg1"]
    cfgs = [scaled_config(cfg, float(rng.uniform(0.5, 1.5))) for _ in range(EXISTING_STORE["n"])]
    return {t: sum(getattr(cfgs[i], "n_" + t) for i in EXISTING_STORE["ids"]) for t in TYPES}
