"""The fp32 weight-stationary dW kernels (k_wsp_f32 at N = K = 256, k_wsd_f32 elsewhere) run a steady-state loop
without row predicates and peel the start-up blocks and each workgroup's last block, the only one that can hold rows
past M.  Row counts around every boundary of that peeling, with G = the launch grid = the CU count:

    M = 1, 15, 16, 17          one workgroup, one (partial / exact / two) block(s)
    M = 16 G - 1, 16 G, 16 G + 1   one block per workgroup, the last partial / whole / one workgroup with two
    M = 32 G + 5               some workgroups hold one block more than the others; a partial last block
    M = 48 G - 16              three blocks per workgroup but the last: start-up, one steady block, tail
    M = 96 G + 5               6 G + 1 blocks: workgroup 0 holds 7, the others 6, the last block 5 rows.  Workgroup b of
                               a grid of min(G, blocks) runs my = (blocks - 1 - b) // G + 1 blocks, and the loops enter
                               their steady-state iteration only at my >= 4 (k_wsp_f32: `i + 3 < my`), my >= 4
                               (k_wsd_f32 fused, 2-deep ring: one start-up block, then `i + 2 < my`) and my >= 6
                               (k_wsd_f32 plain, 3-deep ring: two start-up blocks, then `i + 3 < my`)

for the three shapes of the fp32 path: N = K = 256 (k_wsp_f32), N = 256 with K = 256 + 256 (the PReLU-fused pass
and a plain pass on the stored g_z), N = 128 with K = 384 + 128 (k_wsd_f32<128, 512>, a lane's B piece from either
source).  Checked: g_z bit-identical to hgin_prelu_bwd, g_w bit-identical to the plain dW on it, g_w / g_b / g_a
against float64 at test_wsd_prelu_fused_equals_two_pass's bounds, a second call bit-identical, and every output
byte-identical to the parent commit's kernels (SHA-256 recorded by tests/golden/make_wsd_tail_sha256.py on a build
of the commit before the loops were peeled; the M partition, product order and sum orders did not change).

The other instantiations of the family are pinned to bytes the same way (test_wsd_more_*; hashes recorded on a build
of the commit before the split product order, the opaque thread id and the launch code became shared helpers):

    fp32  N = 256, K = 128; N = 128, K = 128; N = 128, K = 256: the fused kernel (mlp_bwd_w) and the plain one (gemm_tn
          on g_z) of k_wsd_f32 at each, M = 1 (one partial block), 17 (two workgroups, one block each, the second one
          row), 16 G + 1 (workgroup 0 holds two blocks, its last one row), 96 G + 5 (above).
    bf16  k_wsd_bf16, 32-row blocks, a 4-deep ring (3-deep fused): N = K = 256 fused and plain; N = 256, K = 256 + 256
          (the fused pass over columns [0, 256), then the plain one over [256, 512) on the stored g_z); N = 128,
          K = 384 + 128 fused (one pass, a lane's B chunk from either source); M = 1, 33 (two workgroups, the second
          one row), 32 G + 1 (workgroup 0 holds two blocks), 160 G + 5 (5 G + 1 blocks: 6 in workgroup 0, 5 elsewhere,
          so every ring slot is refilled; the last block 5 rows).  One z-from-y case (y_alt) at N = K = 256,
          M = 32 G + 1.  bf16 outputs hash as their raw 16-bit patterns."""
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
        "32G+5": lambda G: 32 * G + 5, "48G-16": lambda G: 48 * G - 16, "96G+5": lambda G: 96 * G + 5}
SHAPES_F32 = {"n256_k128": (256, 128, 0), "n128_k128": (128, 128, 0), "n128_k256": (128, 256, 0)}
ROWS_F32 = ("1", "17", "16G+1", "96G+5")
SHAPES_BF16 = {"bf16_n256_k256": (256, 256, 0), "bf16_n256_k256+256": (256, 256, 256),
               "bf16_n128_k384+128": (128, 384, 128)}
ROWS_BF16 = {"1": ROWS["1"], "33": lambda G: 33, "32G+1": lambda G: 32 * G + 1, "160G+5": lambda G: 160 * G + 5}
ZY_CASE = ("bf16_n256_k256", "32G+1")
ALL_SHAPES = {**SHAPES, **SHAPES_F32, **SHAPES_BF16}
ALL_ROWS = {**ROWS, **ROWS_BF16}   # (the keys of ROWS first: the seeds of the first cases stay)
MORE = [(s, r) for s in SHAPES_F32 for r in ROWS_F32] + [(s, r) for s in SHAPES_BF16 for r in ROWS_BF16]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wsd_tail_sha256.json")
POISON = -7.25


def grid():
    return torch.cuda.get_device_properties(0).multi_processor_count


def make_inputs(shape, rows, pad=0):
    """(g_y, z, slope, b1, b2) on the device, built on the CPU from a fixed seed; z holds exact zeros and
    negatives.  pad > 0: every operand is a column slice of a buffer ``pad`` columns wider (row stride > width)."""
    N, K1, K2 = ALL_SHAPES[shape]
    M = ALL_ROWS[rows](grid())
    torch.manual_seed(1000 * N + K1 + K2 + list(ALL_ROWS).index(rows))
    gy, z, b1 = torch.randn(M, N + pad), torch.randn(M, N + pad), torch.randn(M, K1 + pad)
    b2 = torch.randn(M, K2 + pad) if K2 else None
    z[torch.rand(M, N + pad) < 0.125] = 0.0
    out = []
    for t, w in ((gy, N), (z, N), (b1, K1), (b2, K2)):
        if t is not None and shape in SHAPES_BF16:
            t = t.to(torch.bfloat16)
        out.append(None if t is None else t.to(DEV)[:, :w] if pad else t.to(DEV))
    return out[0], out[1], torch.tensor([SLOPE], device=DEV), out[2], out[3]


def run_traced(shape, rows, zy=False):
    """(the five outputs, the weight-stationary launches of mlp_bwd_w, those of gemm_tn).  zy: the bf16 z-from-y form
    (y = prelu(z) passed as y_alt; no gemm_tn)."""
    gy, z, a, b1, b2 = make_inputs(shape, rows)
    y = torch.where(z > 0, z, (SLOPE * z.float()).to(z.dtype)) if zy else None
    with _lib.trace_launches() as tr1:
        g_w, g_a, g_b, g_z = ops.mlp_bwd_w(gy, z, a, b1, b2, want_gz=True, y_alt=y)
    out = {"g_w": g_w, "g_a": g_a, "g_b": g_b, "g_z": g_z}
    with _lib.trace_launches() as tr2:
        if not zy:
            out["tn"] = ops.gemm_tn(g_z, b1, b2)
    torch.cuda.synchronize()
    return out, [k for k in tr1.kernels if k.startswith("k_ws")], [k for k in tr2.kernels if k.startswith("k_ws")]


def run_ops(shape, rows):
    """The five outputs through hgin.ops: (g_w, g_a, g_b, g_z) of mlp_bwd_w and the plain gemm_tn on g_z."""
    return run_traced(shape, rows)[0]


def sha(t):
    t = t.detach().contiguous()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def case_hashes(shape, rows, zy=False):
    return {k: sha(v) for k, v in run_traced(shape, rows, zy)[0].items()}


def all_case_hashes():
    """{golden key: hashes} of every case of this module (tests/golden/make_wsd_tail_sha256.py)."""
    cases = {f"{s}/{r}": case_hashes(s, r) for s in SHAPES for r in ROWS}
    cases.update({f"{s}/{r}": case_hashes(s, r) for s, r in MORE})
    cases["/".join(ZY_CASE) + "/zy"] = case_hashes(*ZY_CASE, zy=True)
    return cases


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


def expected_kernels(shape):
    """The weight-stationary launches of (mlp_bwd_w, gemm_tn on g_z) at a shape of SHAPES_F32 / SHAPES_BF16."""
    N, K1, K2 = ALL_SHAPES[shape]
    K = K1 + K2
    if shape in SHAPES_F32:
        return [f"k_wsd_f32<{N},{K},prelu_bwd_fused>"], [f"k_wsd_f32<{N},{K}>"]
    kv = 256 if (K == 512 and N == 256) else K   # N = 256, K = 512: two 256-column passes
    fused = [f"k_wsd_bf16<{N},{kv},prelu_bwd_fused>"] + ([f"k_wsd_bf16<{N},256>"] if kv != K else [])
    return fused, [f"k_wsd_bf16<{N},{min(K, 256)}>"] * (2 if K == 512 else 1)


_more = {}


def more_outputs(shape, rows, zy=False):   # computed once per case, shared and left unchanged
    if (shape, rows, zy) not in _more:
        _more[(shape, rows, zy)] = run_traced(shape, rows, zy)
    return _more[(shape, rows, zy)]


def check_more(shape, rows, zy):
    """Kernels from the launch trace; g_z the documented arithmetic exactly (z > 0 ? g_y : slope * g_y in fp32, one
    RNE rounding to the storage type); g_w against float64 on that g_z; a second call the same bits.
    g_w bound: every fp32 addition errs by at most one ulp, 2^-23 of the running magnitude <= sum |g_z b| (whether the
    matrix unit rounds to nearest or truncates; the fp32 split drops terms below 2^-25 |ab|); a workgroup chains
    its own rows (at most ceil(blocks / grid) blocks) and k_slab_reduce adds the slabs in two levels of 16, so at
    most rows_per_workgroup + 32 additions reach an output element."""
    N, K1, K2 = ALL_SHAPES[shape]
    gy, z, a, b1, b2 = make_inputs(shape, rows)
    o, tr_fused, tr_plain = more_outputs(shape, rows, zy)
    want_fused, want_plain = expected_kernels(shape)
    assert tr_fused == want_fused, tr_fused
    assert tr_plain == ([] if zy else want_plain), tr_plain
    gz_ref = torch.where(z > 0, gy.float(), a * gy.float()).to(z.dtype)
    assert torch.equal(o["g_z"], gz_ref)
    b = b1 if b2 is None else torch.cat((b1, b2), 1)
    M, bm = z.shape[0], 32 if shape in SHAPES_BF16 else 16
    blocks = -(-M // bm)
    adds = -(-blocks // min(grid(), blocks)) * bm + 32
    ref_w = o["g_z"].double().t() @ b.double()
    bound = adds * 2.0 ** -23 * (o["g_z"].double().abs().t() @ b.double().abs()) + 1e-30
    for name in ("g_w",) if zy else ("g_w", "tn"):
        err = (o[name].double() - ref_w).abs()
        print(f"{shape}/{rows}{'/zy' if zy else ''} {name}: max err / bound = {float((err / bound).max()):.3g}")
        assert (err <= bound).all()
    again = run_traced(shape, rows, zy)[0]
    for k in o:
        assert torch.equal(again[k], o[k]), k


@pytest.mark.parametrize("shape,rows", MORE)
def test_wsd_more_values(shape, rows):
    check_more(shape, rows, False)


def test_wsd_more_values_zy():
    check_more(*ZY_CASE, True)


@pytest.mark.parametrize("shape,rows", MORE)
def test_wsd_more_bytes_equal_parent(shape, rows):
    gold = json.load(open(GOLDEN))
    assert gold["cus"] == grid(), f"hashes recorded for a {gold['cus']}-CU grid, this device has {grid()}"
    got = {k: sha(v) for k, v in more_outputs(shape, rows)[0].items()}
    assert got == gold["cases"][f"{shape}/{rows}"]


def test_wsd_more_bytes_equal_parent_zy():
    gold = json.load(open(GOLDEN))
    assert gold["cus"] == grid(), f"hashes recorded for a {gold['cus']}-CU grid, this device has {grid()}"
    got = {k: sha(v) for k, v in more_outputs(*ZY_CASE, True)[0].items()}
    assert got == gold["cases"]["/".join(ZY_CASE) + "/zy"]
