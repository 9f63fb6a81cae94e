"""hgin_gat_wsum_f32 (the fixed-order column sums behind g_att_src, g_att_dst and g_bias) against float64, at the
row counts where its two passes change shape: around one 256-row block, more than 256 blocks (the final pass's
t, t + 256, ... stride; production calls it at millions of rows), H C > 256 (the f += 256 column loop) and n = 0.
Bound per column: |out - ref| <= 1e-5 sum_n |w x| (tests/test_gat_host.py holds an fp32 evaluation to a quarter of
it)."""
import ctypes

import pytest
import torch

import gat_cases as gc

DEV = "cuda"
HGIN_E_WORKSPACE = -3     # include/hgin.h

pytestmark = pytest.mark.gpu


def _wsum(x, w, n, H, C, short_by=0):
    """(status, out, kernels) of one call with a workspace of exactly the required size minus short_by bytes."""
    from hgin import _lib
    from hgin.ops import _p, _stream
    nbytes = ctypes.c_size_t(0)
    _lib.check(_lib.lib().hgin_gat_wsum_workspace_size(n, H, C, ctypes.byref(nbytes)), "gat_wsum_workspace_size")
    assert nbytes.value == 4 * max((n + 255) // 256, 1) * H * C
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=DEV)
    out = torch.full((H * C,), float("nan"), device=DEV)
    with _lib.trace_launches() as tr:
        rc = _lib.lib().hgin_gat_wsum_f32(_p(x), x.stride(0), n, H, C, _p(w), _p(out), _p(ws), nbytes.value - short_by,
                                          _stream(out))
        torch.cuda.synchronize()
    return rc, out, tr.kernels


@pytest.mark.parametrize("n,H,C", gc.WSUM_CASES)
def test_wsum_vs_float64(n, H, C):
    xw, w, refs = gc.wsum_case(n, H, C)
    xw_d, w_d = xw.to(DEV), w.to(DEV)
    x_slice = xw_d[:, 1:1 + H * C]                  # row stride H C + 3, rows not 16-B aligned
    assert x_slice.stride(0) == H * C + gc.WSUM_PAD or n <= 1
    for x in (x_slice, x_slice.contiguous()):
        for weighted in (False, True):
            ref, bound = refs[weighted]
            rc, out, kernels = _wsum(x, w_d if weighted else None, n, H, C)
            assert rc == 0, (n, H, C, weighted, rc)
            if n == 0:
                assert kernels == [] and not bool(out.any()) and bool(torch.isfinite(out).all())    # exact zeros
                continue
            assert kernels == ["k_gat_wsum"]
            err = (out.double().cpu() - ref).abs()
            print((n, H, C, weighted), "max err / bound", float((err / bound).max()))
            assert bool((err <= bound).all()), (n, H, C, weighted, float((err / bound).max()))
            rc2, out2, _ = _wsum(x, w_d if weighted else None, n, H, C)
            assert rc2 == 0 and torch.equal(out, out2)                                               # fixed order
    if n > 0:
        rc, out, kernels = _wsum(x_slice, None, n, H, C, short_by=1)
        assert rc == HGIN_E_WORKSPACE and kernels == [] and bool(torch.isnan(out).all())
