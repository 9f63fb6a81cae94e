"""Shared case builder of the graph-attention degree tests (tests/test_gat_host.py, tests/test_gpu_gat_degrees.py,
tests/test_gpu_gat_wsum.py): graphs whose in- and out-degrees are prescribed exactly, so that every degree window the
kernels of csrc/hgin_gat.hip branch on is reached, their inputs, the float64 reference (oracle.pyg_cpu.gat_relation
with ``adjust_self_loops=False`` under autograd) and the error measures the tests hold the kernels to.  Everything
here runs on the host and is deterministic from its seed; the references are computed once and shared (callers must
not modify them).

What the kernels branch on: the lane-group width G (1 .. 64, the next power of two >= H C / 4), ES = G / H edge slots,
U = 4 (one-pass forward, backward) or 8 (two-pass forward) edges in flight, the 32 logits per row kept in LDS, and the
first G edge endpoints of a row arriving by shuffle (later ones are re-read).  ``LADDER_DEGREES`` are the neighbours
of all of these.

Error measures (``ratios``): a value <= 1 means "within the tolerance"; the GPU tests assert <= 1 for the kernels, the
host test asserts <= 0.25 for torch's own fp32 evaluation of the reference formula on the same inputs, i.e. the inputs
are conditioned well enough that a correct fp32 kernel has a fourfold margin.  That quarter is a condition on the
inputs: if a seed misses it, the seed changes, never the tolerance.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Dict, Optional

import torch
from torch import Tensor

SLOPE = 0.2
TOL = 1e-5          # output / alpha: abs + rel; gradients: of their norm (tests/test_gpu_gat.py's tolerances)
ALPHA_SUM_TOL = 1e-6   # |sum_k alpha_k - 1| <= 1e-6 deg per non-empty (row, head)

# (H, C, G): G = the wave-group width the launch trace must show, 0 = the thread-per-(row, head) form
SHAPES = [(1, 4, 1), (2, 4, 2), (1, 16, 4), (3, 4, 4), (2, 16, 8), (3, 8, 8), (16, 4, 16), (5, 8, 16), (16, 8, 32),
          (12, 8, 32), (64, 4, 64), (16, 16, 64), (12, 16, 64),
          (3, 6, 0), (2, 2, 0), (1, 1, 0), (5, 12, 0), (8, 64, 0)]
SHAPES_OPERANDS = [(16, 8, 32), (3, 8, 8), (3, 6, 0)]      # optional operands, strides, ordered rows
SHAPES_SHORT = [(1, 4, 1), (2, 4, 2), (16, 8, 32)]          # short_rows

LADDER_DEGREES = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 34, 39, 40, 41, 63, 64, 65, 66, 127, 128, 129,
                  200, 257, 0]
HUB = 5            # the source of every third edge of the ladder's rows of degree >= 64
N_IDLE = 20        # sources no edge leaves (the last N_IDLE of n_src)
ORDERED_DEG = 48
ORDERED_PEAK = 40  # "maximum at position 40": past the 32 LDS slots and past G = 32


@dataclass(frozen=True)
class Case:
    edge_index: Tensor   # int64 [2, E], used exactly as it stands (no self-loop adjustment)
    n_src: int
    n_dst: int

    @property
    def in_degree(self) -> Tensor:
        return torch.bincount(self.edge_index[1], minlength=self.n_dst)

    @property
    def out_degree(self) -> Tensor:
        return torch.bincount(self.edge_index[0], minlength=self.n_src)


def _from_rows(rows, n_src: int, gen: Optional[torch.Generator]) -> Case:
    """rows[i] = the sources of destination i in the order its edges shall have; gen: shuffle the edge list."""
    src = torch.cat([r for r in rows]) if rows else torch.zeros(0, dtype=torch.long)
    dst = torch.cat([torch.full((r.numel(),), i, dtype=torch.long) for i, r in enumerate(rows)])
    ei = torch.stack([src, dst])
    if gen is not None:
        ei = ei[:, torch.randperm(ei.size(1), generator=gen)]
    return Case(ei.contiguous(), n_src, len(rows))


def degree_ladder(n_src: int = 600, seed: int = 0) -> Case:
    """29 destinations with the in-degrees LADDER_DEGREES (an empty row first and last); sources drawn with
    replacement from [0, n_src - 20), duplicates being separate edges; in rows of degree >= 64 every third edge comes
    from source HUB (out-degree ~350: past G and many U-batches on the CSC side); the edge list is shuffled."""
    gen = torch.Generator().manual_seed(seed)
    rows = []
    for d in LADDER_DEGREES:
        r = torch.randint(0, n_src - N_IDLE, (d,), generator=gen)
        if d >= 64:
            r[::3] = HUB
        rows.append(r)
    return _from_rows(rows, n_src, gen)


def short_rows(n_dst: int = 515, n_src: int = 300, seed: int = 0) -> Case:
    """Degrees cycling 0 .. 9 over more than two 256-row blocks with a ragged end (the small-G row-to-group mapping:
    G = 1 puts 256 rows into one workgroup); sources as in degree_ladder, shuffled."""
    gen = torch.Generator().manual_seed(seed)
    rows = [torch.randint(0, n_src - N_IDLE, (i % 10,), generator=gen) for i in range(n_dst)]
    return _from_rows(rows, n_src, gen)


def ordered_rows(xs: Tensor, xd: Tensor, att_s: Tensor, att_d: Tensor, seed: int = 0) -> Case:
    """6 destinations (xd's rows) of degree ORDERED_DEG; the edge-list order within a row is chosen from the float64
    logits of head 0: row 0 ascending (the running maximum moves at every edge), row 1 descending, row 2 with its
    maximum at position ORDERED_PEAK, rows 3 .. 5 as drawn.  The rows are interleaved in the edge list (edge t of every
    row, then edge t + 1), which keeps each row's order."""
    gen = torch.Generator().manual_seed(seed)
    n_src, n_dst = xs.size(0), xd.size(0)
    assert n_dst == 6
    a_s = (xs.double() * att_s.double()).sum(-1)[:, 0]
    a_d = (xd.double() * att_d.double()).sum(-1)[:, 0]
    rows = []
    for i in range(n_dst):
        r = torch.randperm(n_src - N_IDLE, generator=gen)[:ORDERED_DEG]     # distinct sources: distinct logits
        e = torch.nn.functional.leaky_relu(a_s[r] + a_d[i], SLOPE)
        if i == 0:
            r = r[torch.argsort(e)]
        elif i == 1:
            r = r[torch.argsort(e, descending=True)]
        elif i == 2:
            k = int(torch.argmax(e))
            idx = list(range(ORDERED_DEG))
            idx[k], idx[ORDERED_PEAK] = idx[ORDERED_PEAK], idx[k]
            r = r[torch.tensor(idx)]
        rows.append(r)
    src = torch.stack(rows, 1).reshape(-1)                                  # [deg, n_dst] -> edge t of every row
    dst = torch.arange(n_dst).repeat(ORDERED_DEG)
    return Case(torch.stack([src, dst]).contiguous(), n_src, n_dst)


def inputs(H: int, C: int, n_src: int, n_dst: int, seed: int, att_src_scale: float = 0.3) -> Dict[str, Tensor]:
    """fp32 operands of one relation (tests/test_gpu_gat.py's distributions): unit-normal projections, bias, accum
    and upstream gradient, attention vectors 0.3 x unit-normal (att_src: att_src_scale x)."""
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen)   # noqa: E731
    return dict(xs=r(n_src, H * C), xd=r(n_dst, H * C), att_s=att_src_scale * r(1, H, C), att_d=0.3 * r(1, H, C),
                bias=r(H * C), g_out=r(n_dst, H * C), accum=r(n_dst, H * C))


def reference(case: Case, inp: Dict[str, Tensor], H: int, C: int, dtype=torch.float64, use_xd: bool = True,
              use_bias: bool = True, use_accum: bool = False) -> Dict[str, Tensor]:
    """out = aggregate (+ bias) (accum +), alpha per edge of case.edge_index, and the gradients of <out, g_out>, by
    oracle.pyg_cpu.gat_relation(adjust_self_loops=False) in ``dtype`` under autograd; plus, written out from the
    formulas of csrc/hgin_gat.hip's header, g_a_d[i, h] = sum_k g_pre_k and its condition T[i, h] = sum_k |g_pre_k|."""
    from oracle.pyg_cpu import gat_relation
    ns, nd = case.n_src, case.n_dst
    xs, xd, att_s, att_d, bias = (inp[k].to(dtype).clone().requires_grad_() for k in
                                  ("xs", "xd", "att_s", "att_d", "bias"))
    xdv = xd.view(nd, H, C) if use_xd else torch.zeros(nd, H, C, dtype=dtype)
    alpha, agg = gat_relation(xs.view(ns, H, C), xdv, case.edge_index, att_s, att_d, SLOPE, adjust_self_loops=False)
    out = agg.reshape(nd, H * C)
    if use_bias:
        out = out + bias
    if use_accum:
        out = inp["accum"].to(dtype) + out
    g_out = inp["g_out"].to(dtype)
    out.backward(g_out)
    ref = dict(out=out.detach(), alpha=alpha.detach(), g_xs=xs.grad, g_att_src=att_s.grad)
    if use_xd:
        ref.update(g_xd=xd.grad, g_att_dst=att_d.grad)
    if use_bias:
        ref["g_bias"] = bias.grad
    with torch.no_grad():
        j, i = case.edge_index
        xs3 = xs.view(ns, H, C)
        pre = (xs3 * att_s).sum(-1)[j] + (xdv * att_d).sum(-1)[i]
        g_alpha = (g_out.view(nd, H, C)[i] * xs3[j]).sum(-1)
        al = alpha.detach()
        S = torch.zeros(nd, H, dtype=dtype).index_add_(0, i, al * g_alpha)
        g_e = al * (g_alpha - S[i])
        g_pre = torch.where(pre > 0, g_e, SLOPE * g_e)
        ref["g_ad"] = torch.zeros(nd, H, dtype=dtype).index_add_(0, i, g_pre)
        ref["g_ad_cond"] = torch.zeros(nd, H, dtype=dtype).index_add_(0, i, g_pre.abs())
        ref["max_logit"] = torch.nn.functional.leaky_relu(pre, SLOPE).abs().max() if pre.numel() else pre.sum()
    return ref


def ratio_close(got: Tensor, ref: Tensor, tol: float = TOL) -> float:
    """max |got - ref| / (tol + tol |ref|): <= 1 is tests/test_gpu_gat.py's ``_close``."""
    got, ref = got.detach().double().cpu(), ref.double()
    if ref.numel() == 0:
        return 0.0
    return float(((got - ref).abs() / (tol + tol * ref.abs())).max())


def ratio_norm(got: Tensor, ref: Tensor, tol: float = TOL) -> float:
    """||got - ref|| / (tol ||ref|| + 1e-9): <= 1 is test_relation_forward_backward_vs_oracle's gradient bound."""
    got, ref = got.detach().double().cpu().reshape(ref.shape), ref.double()
    return float((got - ref).norm()) / (tol * float(ref.norm()) + 1e-9)


def ratio_bound(got: Tensor, ref: Tensor, bound: Tensor) -> float:
    """max |got - ref| / bound elementwise (bound > 0)."""
    got, ref = got.detach().double().cpu().reshape(ref.shape), ref.double()
    return float(((got - ref).abs() / bound).max())


def alpha_sum_ratio(alpha: Tensor, case: Case) -> float:
    """max over the non-empty (row, head) of |sum_k alpha_k - 1| / (1e-6 deg); alpha [E, H] in edge-list order."""
    a = alpha.detach().double().cpu()
    deg = case.in_degree.double()
    s = torch.zeros(case.n_dst, a.size(1), dtype=torch.float64).index_add_(0, case.edge_index[1], a)
    on = deg > 0
    return float(((s[on] - 1.0).abs() / (ALPHA_SUM_TOL * deg[on]).unsqueeze(1)).max())


GRADS = ("g_xs", "g_xd", "g_att_src", "g_att_dst", "g_bias")


def ratios(got: Dict[str, Tensor], ref: Dict[str, Tensor], case: Case, inp: Dict[str, Tensor], H: int, C: int,
           conditioned: bool = False) -> Dict[str, float]:
    """Error / tolerance of every entry of ``got`` that ``ref`` has.  ``conditioned`` (ordered_rows): g_x_d and
    g_att_dst are not held to their own norm, because with a softmax that peaked g_a_d = sum_k g_pre_k cancels to almost
    nothing; they are held to the cancellation's condition number instead, |g_a_d - ref| <= 1e-5 sum_k |g_pre_k| and
    what follows from it for g_x_d = g_a_d att_dst and g_att_dst = sum_i g_a_d x_d."""
    r = {}
    for k in ("out", "alpha"):
        if k in got:
            r[k] = ratio_close(got[k], ref[k])
    if "alpha" in got:
        r["alpha_sum"] = alpha_sum_ratio(got["alpha"], case)
    T = ref["g_ad_cond"]
    for k in GRADS:
        if k not in got or k not in ref:
            continue
        if conditioned and k == "g_xd":
            bound = TOL * (T.unsqueeze(-1) * inp["att_d"].double().abs()).reshape(case.n_dst, H * C) + 1e-12
            r[k] = ratio_bound(got[k], ref[k], bound)
        elif conditioned and k == "g_att_dst":
            bound = TOL * (T.unsqueeze(-1) * inp["xd"].double().view(case.n_dst, H, C).abs()).sum(0) + 1e-12
            r[k] = ratio_bound(got[k], ref[k].reshape(H, C), bound)
        else:
            r[k] = ratio_norm(got[k], ref[k])
    if "g_ad" in got:
        r["g_ad"] = ratio_bound(got["g_ad"], ref["g_ad"], TOL * T + 1e-12)
    return r


# ---- the cases the GPU tests use, each with its float64 reference, built once ------------------------------------

@functools.lru_cache(maxsize=None)
def ladder_case(H: int, C: int, use_xd: bool = True, use_bias: bool = True, use_accum: bool = False):
    case = _ladder()
    inp = inputs(H, C, case.n_src, case.n_dst, seed=1000 * H + C + 4)
    return case, inp, reference(case, inp, H, C, torch.float64, use_xd, use_bias, use_accum)


@functools.lru_cache(maxsize=None)
def _ladder() -> Case:
    return degree_ladder(seed=11)


@functools.lru_cache(maxsize=None)
def short_case(H: int, C: int):
    case = short_rows(seed=12)
    inp = inputs(H, C, case.n_src, case.n_dst, seed=2000 * H + C)
    return case, inp, reference(case, inp, H, C)


@functools.lru_cache(maxsize=None)
def ordered_case(H: int, C: int):
    """att_src = 3.0 x unit-normal: logits of tens, so the online softmax's rescale exp(m_old - m_new) spans many
    orders of magnitude and a dropped or misordered rescale is an error of order 1."""
    inp = inputs(H, C, 300, 6, seed=3000 * H + C, att_src_scale=3.0)
    case = ordered_rows(inp["xs"].view(-1, H, C), inp["xd"].view(-1, H, C), inp["att_s"], inp["att_d"], seed=13)
    return case, inp, reference(case, inp, H, C)


def fp32_ratios(case: Case, inp, ref, H: int, C: int, conditioned: bool = False, **variant) -> Dict[str, float]:
    """torch's fp32 evaluation of the reference formula against the float64 reference, in the tests' measures."""
    got = reference(case, inp, H, C, torch.float32, **variant)
    got = {k: v for k, v in got.items() if k in ("out", "alpha") + GRADS}   # autograd's results only
    return ratios(got, ref, case, inp, H, C, conditioned)


# ---- hgin_gat_wsum_f32 -------------------------------------------------------------------------------------------

# (n, H, C): around the 256-row block, more than 256 blocks (the final pass's t, t + 256 stride), H C > 256 (the
# f += 256 column loop) and a thread-form width
WSUM_CASES = [(0, 2, 4), (1, 2, 4), (255, 2, 4), (256, 2, 4), (257, 2, 4), (65537, 2, 4), (70001, 1, 4),
              (300, 8, 64), (300, 5, 12)]
WSUM_PAD = 3       # x is a column slice [:, 1 : 1 + H C] of a tensor WSUM_PAD columns wider


@functools.lru_cache(maxsize=None)
def wsum_case(n: int, H: int, C: int):
    """(x_wide fp32 [n, H C + WSUM_PAD], w fp32 [n, H], {weighted: (ref, bound)}): ref = sum_n w x in float64 per
    column, bound = 1e-5 sum_n |w x|."""
    gen = torch.Generator().manual_seed(7 * n + 100 * H + C)
    xw = torch.randn(n, H * C + WSUM_PAD, generator=gen)
    w = torch.randn(n, H, generator=gen)
    x = xw[:, 1:1 + H * C].double()
    refs = {}
    for weighted in (False, True):
        t = x * w.double().repeat_interleave(C, dim=1) if weighted else x
        refs[weighted] = (t.sum(0), TOL * t.abs().sum(0))
    return xw, w, refs


def wsum_fp32_ratio(n: int, H: int, C: int, weighted: bool) -> float:
    """torch's fp32 evaluation (products in fp32, rows added one after another in blocks of 256, then the blocks) over
    the bound; n = 0 has nothing to round."""
    xw, w, refs = wsum_case(n, H, C)
    if n == 0:
        return 0.0
    ref, bound = refs[weighted]
    x = xw[:, 1:1 + H * C]
    t = x * w.repeat_interleave(C, dim=1) if weighted else x
    parts = torch.stack([b.cumsum(0)[-1] for b in t.split(256)])     # fp32 running sums
    got = parts.cumsum(0)[-1]
    return float(((got.double() - ref).abs() / bound).max())
