"""The fp32 weight-stationary dW kernels (k_wsp_f32 at N = K = 256, k_wsd_f32 elsewhere) run a steady-state loop
without row predicates and peel the start-up blocks and each workgroup's last block, the only one that can hold rows
past M.  Row counts around every boundary of that peeling, with G = the launch grid = the CU count:

    M = 1, 15, 16, 17          one workgroup, one (partial / exact / two) block(s)
    M = 16 G - 1, 16 G, 16 G + 1   one block per workgroup, the last partial / whole / one workgroup with two
    M = 32 G + 5               some workgroups hold one block more than the others; a partial last block
    M = 48 G - 16              three blocks per workgroup but the last: start-up, one steady block, tail

for the three shapes of the fp32 path: N = K = 256 (k_wsp_f32), N = 256 with K = 256 + 256 (the PReLU-fused pass
and a plain pass on the stored g_z), N = 128 with K = 384 + 128 (k_wsd_f32<128, 512>, a lane's B piece from either
source).  Checked: g_z bit-identical to hgin_prelu_bwd, g_w bit-identical to the plain dW on it, g_w / g_b / g_a
against float64 at test_wsd_prelu_fused_equals_two_pass's bounds, a second call bit-identical, and every output
byte-identical to the parent commit's kernels (SHA-256 recorded by tests/golden/make_wsd_tail_sha256.py on a build
of the commit before the loops were peeled; the M partition, product order and sum orders did not change)."""
import ctypes
import hashlib
import json
import os

import pytest
import torch

from hgin import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
SLOPE = 0.3
SHAPES = {"n256_k256": (256, 256, 0), "n256_k256+256": (256, 256, 256), "n128_k384+128": (128, 384, 128)}
ROWS = {"1": lambda G: 1, "15": lambda G: 15, "16": lambda G: 16, "17": lambda G: 17,
        "16G-1": lambda G: 16 * G - 1, "16G": lambda G: 16 * G, "16G+1": lambda G: 16 * G + 1,
        "32G+5": lambda G: 32 * G + 5, "48G-16": lambda G: 48 * G - 16}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wsd_tail_sha256.json")
POISON = -7.25


def grid():
    return torch.cuda.get_device_properties(0).multi_processor_count


def make_inputs(shape, rows, pad=0):
    """(g_y, z, slope, b1, b2) on the device, built on the CPU from a fixed seed; z holds exact zeros and
    negatives.  pad > 0: every operand is a column slice of a buffer ``pad`` columns wider (row stride > width)."""
    N, K1, K2 = SHAPES[shape]
    M = ROWS[rows](grid())
    torch.manual_seed(1000 * N + K1 + K2 + list(ROWS).index(rows))
    gy, z, b1 = torch.randn(M, N + pad), torch.randn(M, N + pad), torch.randn(M, K1 + pad)
    b2 = torch.randn(M, K2 + pad) if K2 else None
    z[torch.rand(M, N + pad) < 0.125] = 0.0
    out = []
    for t, w in ((gy, N), (z, N), (b1, K1), (b2, K2)):
        out.append(None if t is None else t.to(DEV)[:, :w] if pad else t.to(DEV))
    return out[0], out[1], torch.tensor([SLOPE], device=DEV), out[2], out[3]


def run_ops(shape, rows):
    """The five outputs through hgin.ops: (g_w, g_a, g_b, g_z) of mlp_bwd_w and the plain gemm_tn on g_z."""
    gy, z, a, b1, b2 = make_inputs(shape, rows)
    g_w, g_a, g_b, g_z = ops.mlp_bwd_w(gy, z, a, b1, b2, want_gz=True)
    tn = ops.gemm_tn(g_z, b1, b2)
    torch.cuda.synchronize()
    return {"g_w": g_w, "g_a": g_a, "g_b": g_b, "g_z": g_z, "tn": tn}


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def case_hashes(shape, rows):
    return {k: sha(v) for k, v in run_ops(shape, rows).items()}


_cache = {}


def outputs(shape, rows):   # computed once per case, shared by the tests below and left unchanged
    if (shape, rows) not in _cache:
        _cache[(shape, rows)] = run_ops(shape, rows)
    return _cache[(shape, rows)]


def check_f64(gy, z, b1, b2, g_w, g_a, g_b):
    b = b1 if b2 is None else torch.cat((b1, b2), 1)
    gzd = torch.where(z.double() > 0, gy.double(), gy.double() * SLOPE)
    ref_w = gzd.t() @ b.double()
    assert ((g_w.double() - ref_w).abs() <= 1e-5 * (gzd.abs().t() @ b.double().abs() + 1)).all()
    assert ((g_b.double() - gzd.sum(0)).abs() <= 1e-5 * gzd.abs().sum(0) + 1e-6).all()
    zr = z.double()
    ga_ref = (torch.where(zr > 0, torch.zeros_like(zr), zr) * gy.double()).sum()
    assert abs(float(g_a) - float(ga_ref)) <= 1e-5 * (float((zr * gy.double()).abs().sum()) + 1)


@pytest.mark.parametrize("rows", list(ROWS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_wsd_tail_values(shape, rows):
    N, K1, K2 = SHAPES[shape]
    gy, z, a, b1, b2 = make_inputs(shape, rows)
    with _lib.trace_launches() as tr:
        again = ops.mlp_bwd_w(gy, z, a, b1, b2, want_gz=True)
    torch.cuda.synchronize()
    want = "k_wsp_f32<256,256,prelu_bwd_fused>" if N == 256 else "k_wsd_f32<128,512,prelu_bwd_fused>"
    assert want in tr.kernels, tr.kernels
    o = outputs(shape, rows)
    gz2, _, _ = ops.prelu_bwd(gy, z, a)
    assert torch.equal(o["g_z"], gz2)
    assert torch.equal(o["g_w"], o["tn"])          # the plain dW on g_z: same partition, passes and product order
    check_f64(gy, z, b1, b2, o["g_w"], o["g_a"], o["g_b"])
    for p, q in zip(again, (o["g_w"], o["g_a"], o["g_b"], o["g_z"])):   # a second call: the same bits
        assert torch.equal(p, q)


@pytest.mark.parametrize("rows", list(ROWS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_wsd_tail_bytes_equal_parent(shape, rows):
    gold = json.load(open(GOLDEN))
    assert gold["cus"] == grid(), f"hashes recorded for a {gold['cus']}-CU grid, this device has {grid()}"
    got = {k: sha(v) for k, v in outputs(shape, rows).items()}
    assert got == gold["cases"][f"{shape}/{rows}"]


@pytest.mark.parametrize("shape,rows", [("n256_k256", "32G+5"), ("n128_k384+128", "32G+5"),
                                        ("n256_k256+256", "16G+1")])
def test_wsd_tail_strided_and_guarded(shape, rows):
    """Row strides larger than the widths on every operand and output (the C ABI called with the test's own
    buffers), a poison-filled guard row after each output: same bits as the dense call, guards untouched."""
    N, K1, K2 = SHAPES[shape]
    K = K1 + K2
    gy, z, a, b1, b2 = make_inputs(shape, rows, pad=8)
    M = gy.shape[0]
    dense = ops.mlp_bwd_w(gy.contiguous(), z.contiguous(), a, b1.contiguous(),
                          None if b2 is None else b2.contiguous(), want_gz=True)
    ldw, ldgz = K + 4, N + 12
    g_w = torch.full((N + 1, ldw), POISON, device=DEV)
    g_z = torch.full((M + 1, ldgz), POISON, device=DEV)
    g_b = torch.full((N + 1,), POISON, device=DEV)
    g_a = torch.full((2,), POISON, device=DEV)
    nbytes = ctypes.c_size_t(0)
    _lib.check(_lib.lib().hgin_gin_mlp_bwd_w_workspace_size(M, N, K, 4, 1, ctypes.byref(nbytes)), "workspace_size")
    ws = ops._workspace(nbytes.value, gy.device)
    p = ops._p
    _lib.call("hgin_gin_mlp_bwd_w_f32", p(gy), gy.stride(0), p(z), z.stride(0), p(a), p(b1), b1.stride(0), K1, p(b2),
              b2.stride(0) if b2 is not None else 0, M, N, K, p(g_w), ldw, p(g_a), p(g_b), p(g_z), ldgz, p(ws),
              nbytes.value, ops._stream(gy))
    tn = torch.full((N + 1, ldw), POISON, device=DEV)
    nb2 = ctypes.c_size_t(0)
    _lib.check(_lib.lib().hgin_gemm_tn_workspace_size(M, N, K, ctypes.byref(nb2)), "gemm_tn_workspace_size")
    ws2 = ops._workspace(nb2.value, gy.device)
    gzv = g_z[:M, :N]
    _lib.call("hgin_gemm_tn_f32", p(gzv), ldgz, p(b1), b1.stride(0), K1, p(b2), b2.stride(0) if b2 is not None else 0,
              M, N, K, p(tn), ldw, p(ws2), nb2.value, ops._stream(gy))
    torch.cuda.synchronize()
    assert torch.equal(g_w[:N, :K], dense[0]) and torch.equal(tn[:N, :K], dense[0])
    assert torch.equal(g_a[:1], dense[1]) and torch.equal(g_b[:N], dense[2]) and torch.equal(gzv, dense[3])
    for t, r, c in ((g_w, N, K), (tn, N, K), (g_z, M, N)):   # the guard row and the padding columns
        assert bool((t[r] == POISON).all()) and bool((t[:, c:] == POISON).all())
    assert float(g_b[N]) == POISON and float(g_a[1]) == POISON
