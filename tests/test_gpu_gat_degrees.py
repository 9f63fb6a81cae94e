"""The graph-attention kernels of csrc/hgin_gat.hip across the degree windows and group widths they branch on
(tests/gat_cases.py builds the graphs with prescribed degrees and the float64 reference): every lane-group width
G = 1 .. 64 with and without idle lanes and the thread-per-(row, head) form; rows of degree 0 and around U = 4 / 8,
ES U, the 32 logits kept in LDS and G (the reload of edge endpoints past the shuffled first G, the spill of logits into
the alpha slots, the recompute of logits past ES U); a hub source on the CSC side; optional operands (a_d, bias, accum)
and padded row strides; and rows whose edge order makes the online softmax's maximum move at every edge, never, or late,
with logits of tens.  Tolerances are those of tests/test_gpu_gat.py::test_relation_forward_backward_vs_oracle: output
and alpha 1e-5 (abs + rel), every gradient 1e-5 of its norm; tests/test_gat_host.py holds the inputs to a quarter of
each (torch's fp32 evaluation of the reference formula against float64).
"""
import ctypes

import pytest
import torch

import gat_cases as gc

DEV = "cuda"
HGIN_E_ARG = -1     # include/hgin.h
SENTINEL = -7.5     # padding columns of strided outputs

pytestmark = pytest.mark.gpu

_GRAPHS = {}


def _graph(case):
    """The case's CSR / CSC on the device, edge list as given (built once per case)."""
    from hgin.gat import gat_graph
    if id(case) not in _GRAPHS:
        ei = case.edge_index.to(DEV)
        _GRAPHS[id(case)] = (case, ei, gat_graph(ei, case.n_src, case.n_dst, False))
    return _GRAPHS[id(case)][2]


def _expect_kernels(kernels, G, forward):
    """The launch trace shows the form the shape must take: the wave-group kernels at width G, or (G = 0) the
    thread-per-(row, head) kernels.  forward: 'attn' (one pass), 'fwd' (logits + two-pass), or None (no forward)."""
    sfx = f"_w<{G}>" if G else ""
    want = {"attn": ["k_gat_attn" + sfx], "fwd": ["k_gat_logits" + sfx, "k_gat_fwd" + sfx], None: []}[forward]
    for k in want:
        assert k in kernels, (k, kernels)
    return want


def _assert_within(r, what):
    print(what, {k: round(v, 4) for k, v in r.items()})     # each figure before it is held to its bound
    assert r and all(v <= 1.0 for v in r.values()), (what, r)


def _autograd(case, inp, H, C, G, use_xd=True, use_bias=True, use_accum=False):
    """_GatAttentionFn forward + backward on the case; the launch trace must show the shape's form in every kernel."""
    from hgin import _lib
    from hgin.gat import _GatAttentionFn
    graph = _graph(case)
    xs, xd, att_s, att_d, bias = (inp[k].to(DEV).requires_grad_() for k in ("xs", "xd", "att_s", "att_d", "bias"))
    accum = inp["accum"].to(DEV).requires_grad_() if use_accum else None
    with _lib.trace_launches() as tr:
        out = _GatAttentionFn.apply(xs, xd if use_xd else None, att_s, att_d, bias if use_bias else None, accum, graph,
                                    H, C, gc.SLOPE)
        out.backward(inp["g_out"].to(DEV))
        torch.cuda.synchronize()
    sfx = f"_w<{G}>" if G else ""
    for k in ("k_gat_logits", "k_gat_attn" if G else "k_gat_fwd", "k_gat_bwd_dst", "k_gat_bwd_src"):
        assert k + sfx in tr.kernels, (k + sfx, tr.kernels)
    assert "k_gat_wsum" in tr.kernels
    got = dict(out=out, g_xs=xs.grad, g_att_src=att_s.grad)
    if use_xd:
        got.update(g_xd=xd.grad, g_att_dst=att_d.grad)
    if use_bias:
        got["g_bias"] = bias.grad
    if use_accum:
        assert torch.equal(accum.grad, inp["g_out"].to(DEV))
    return got


def _direct(entry, case, inp, H, C, use_xd=True, use_bias=True, accum=None, pad=0):
    """One of the two C forward entry points ('attn': hgin_gat_attn_fwd_f32; 'fwd': hgin_gat_logits_f32 +
    hgin_gat_fwd_f32) on the case, alpha pre-filled with NaN (the one-pass kernel parks logits in those slots), x_s and
    out with a row stride of H C + pad and SENTINEL in the padding.  Returns (status, kernels, alpha in edge-list
    order, out)."""
    from hgin import _lib
    from hgin.gat import _logits
    from hgin.ops import _p, _stream
    graph = _graph(case)
    HC = H * C
    xs_w = torch.full((case.n_src, HC + pad), SENTINEL, device=DEV)
    out_w = torch.full((case.n_dst, HC + pad), SENTINEL, device=DEV)
    xs, out = xs_w[:, :HC], out_w[:, :HC]
    xs.copy_(inp["xs"])
    att_s = inp["att_s"].to(DEV).reshape(-1).contiguous()
    att_d = inp["att_d"].to(DEV).reshape(-1).contiguous()
    bias = inp["bias"].to(DEV) if use_bias else None
    alpha = torch.full((graph.n_edges, H), float("nan"), device=DEV)
    with _lib.trace_launches() as tr:
        a_d = _logits(inp["xd"].to(DEV), att_d, H, C) if use_xd else None
        first = _p(att_s) if entry == "attn" else _p(_logits(xs, att_s, H, C))
        rc = getattr(_lib.lib(), f"hgin_gat_{entry}_fwd_f32" if entry == "attn" else "hgin_gat_fwd_f32")(
            _p(graph.csr.rowptr), _p(graph.csr.col), case.n_dst, H, C, _p(xs), xs.stride(0), first, _p(a_d),
            ctypes.c_float(gc.SLOPE), _p(bias), _p(accum), accum.stride(0) if accum is not None else 0, _p(alpha),
            _p(out), out.stride(0), _stream(xs))
        torch.cuda.synchronize()
    assert bool((out_w[:, HC:] == SENTINEL).all()) and bool((xs_w[:, HC:] == SENTINEL).all())
    by_edge = torch.empty_like(alpha)
    by_edge[graph.csr.perm.long()] = alpha          # alpha of CSR position p belongs to edge perm[p]
    return rc, tr.kernels, by_edge, out


def _forward_checks(entry, case, inp, ref, H, C, G, what, **kw):
    rc, kernels, alpha, out = _direct(entry, case, inp, H, C, **kw)
    assert rc == 0, (what, rc)
    _expect_kernels(kernels, G, entry)
    assert bool(torch.isfinite(alpha).all()), what       # every slot of every edge written, none left as scratch
    _assert_within(gc.ratios(dict(alpha=alpha, out=out), ref, case, inp, H, C), (what, entry))
    return out


def _entries(G):
    return ("attn", "fwd") if G else ("fwd",)


@pytest.mark.parametrize("H,C,G", gc.SHAPES)
def test_ladder_autograd(H, C, G):
    """The degree ladder through _GatAttentionFn (the default forward, both backward kernels, the column sums), bias
    and x_d present."""
    case, inp, ref = gc.ladder_case(H, C)
    got = _autograd(case, inp, H, C, G)
    _assert_within(gc.ratios(got, ref, case, inp, H, C), "ladder")
    empty = (case.in_degree == 0).to(DEV)
    assert int(empty.sum()) == 2
    assert torch.equal(got["out"][empty], inp["bias"].to(DEV).expand(2, -1))       # 0 / 1e-16 + bias, exactly
    idle = (case.out_degree == 0).to(DEV)
    assert int(idle.sum()) >= gc.N_IDLE and not bool(got["g_xs"][idle].any())       # exact zeros


@pytest.mark.parametrize("H,C,G", gc.SHAPES)
def test_ladder_forward_entry_points(H, C, G):
    """The degree ladder through both C forward entry points: alpha of every edge and the output."""
    case, inp, ref = gc.ladder_case(H, C)
    for entry in _entries(G):
        _forward_checks(entry, case, inp, ref, H, C, G, "ladder")
    if not G:       # the one-pass entry point refuses the thread-form shapes without launching
        rc, kernels, _, _ = _direct("attn", case, inp, H, C)
        assert rc == HGIN_E_ARG and kernels == ["k_gat_logits"], (rc, kernels)      # (a_d's logits only)


@pytest.mark.parametrize("H,C,G", gc.SHAPES_OPERANDS)
@pytest.mark.parametrize("variant", ["no_a_d", "no_bias", "accum"])
def test_optional_operands(H, C, G, variant):
    """a_d = NULL, bias = NULL, and accum as a column slice of a wider tensor (ld_acc = H C + 8), through both forward
    entry points and through autograd (a backward without g_a_d / g_x_d, without g_bias, with g_accum = g_out)."""
    kw = dict(use_xd=variant != "no_a_d", use_bias=variant != "no_bias", use_accum=variant == "accum")
    case, inp, ref = gc.ladder_case(H, C, **kw)
    acc = None
    if kw["use_accum"]:
        wide = torch.full((case.n_dst, H * C + 8), SENTINEL, device=DEV)
        acc = wide[:, 4:4 + H * C]
        acc.copy_(inp["accum"])
    for entry in _entries(G):
        _forward_checks(entry, case, inp, ref, H, C, G, variant, use_xd=kw["use_xd"], use_bias=kw["use_bias"],
                        accum=acc)
    _assert_within(gc.ratios(_autograd(case, inp, H, C, G, **kw), ref, case, inp, H, C), (variant, "autograd"))


@pytest.mark.parametrize("H,C,G", gc.SHAPES_OPERANDS)
def test_row_strides(H, C, G):
    """x_s and out with a row stride of H C + 4 stay in the wave-group form; H C + 1 (rows no longer 16-B aligned)
    falls back: hgin_gat_fwd_f32 runs the thread form, hgin_gat_attn_fwd_f32 returns HGIN_E_ARG without launching.
    The padding columns keep their sentinel (checked in _direct)."""
    case, inp, ref = gc.ladder_case(H, C)
    for entry in _entries(G):
        _forward_checks(entry, case, inp, ref, H, C, G, "ld + 4", pad=4)
    rc, kernels, alpha, out = _direct("fwd", case, inp, H, C, pad=1)
    assert rc == 0 and "k_gat_fwd" in kernels and "k_gat_logits" in kernels, (rc, kernels)
    assert bool(torch.isfinite(alpha).all())
    _assert_within(gc.ratios(dict(alpha=alpha, out=out), ref, case, inp, H, C), "ld + 1")
    rc, kernels, alpha, out = _direct("attn", case, inp, H, C, pad=1)
    assert rc == HGIN_E_ARG and not any(k.startswith("k_gat_attn") or k.startswith("k_gat_fwd") for k in kernels)
    assert bool(torch.isnan(alpha).all()) and bool((out == SENTINEL).all())          # nothing ran


@pytest.mark.parametrize("H,C,G", gc.SHAPES_OPERANDS)
def test_ordered_rows(H, C, G):
    """Rows of 48 edges ordered by their head-0 logit (ascending: the online softmax rescales at every edge;
    descending; maximum at position 40, past the LDS slots and G = 32), logits up to 25 .. 37, smallest alpha 1e-13 ..
    1e-18.  alpha, out, g_x_s, g_att_src at the usual tolerances; g_x_d and g_att_dst in the conditioned measure of
    gat_cases.ratios (1e-5 of sum_k |g_pre_k| of the float64 reference), because g_a_d = sum_k g_pre_k cancels.
    Before the destination-side backward subtracted the residue of sum_k g_e_k (GatDstSum in csrc/hgin_gat.hip) g_x_d
    stood at 222 x / 117 x / 23 x that bound on the three shapes; with it at 0.017 x / 0.009 x / 0.009 x."""
    case, inp, ref = gc.ordered_case(H, C)
    for entry in _entries(G):
        _forward_checks(entry, case, inp, ref, H, C, G, "ordered")
    got = _autograd(case, inp, H, C, G)
    _assert_within(gc.ratios(got, ref, case, inp, H, C, conditioned=True), ("ordered", "autograd"))


@pytest.mark.parametrize("H,C,G", gc.SHAPES_SHORT)
def test_short_rows(H, C, G):
    """515 rows of degree 0 .. 9: more than two 256-row workgroups at G = 1 with a ragged end."""
    case, inp, ref = gc.short_case(H, C)
    got = _autograd(case, inp, H, C, G)
    _assert_within(gc.ratios(got, ref, case, inp, H, C), "short_rows")
    empty = (case.in_degree == 0).to(DEV)
    assert torch.equal(got["out"][empty], inp["bias"].to(DEV).expand(int(empty.sum()), -1))
    for entry in _entries(G):
        _forward_checks(entry, case, inp, ref, H, C, G, "short_rows")
