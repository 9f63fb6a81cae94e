"""The weight-stationary NT GEMMs of csrc/hgin_gemm_nt.hip (k_wss_f32, k_ws_f32, k_ws_bf16) at every ring depth and
row tail.  Each streams the blocks of BM rows it owns through an LDS ring with counted vmcnt waits; a wrong count reads
a slot before its DMA landed or after its refill and stores a plausible wrong row, so every check here is bitwise.

Row counts.  A launch of nblk = ceil(M / BM) blocks runs min(nblk, Gw) workgroups; workgroup b owns the blocks
b + i Gw, i < my, with my = (nblk - 1 - b) // Gw + 1.  BM = 32 (64 for bf16 K = 128); Gw = G, the CU count (what
ws_grid() reads), or 2 G for the two-workgroups-per-CU forms (trace tags ",cpw64" / ",wpc2").  Only the last block of
the grid can be partial (t rows), and it is the last block of its workgroup.  M = BM (nblk - 1) + t:

    nblk       t        my (workgroup 0 / the others)
    1          1        1          M = 1
    1          BM - 1   1          one partial block
    1          BM       1          one exact block
    2          1        1 / 1      two workgroups, the second one row
    Gw         BM       1          every workgroup one whole block
    Gw + 1     5        2 / 1      workgroup 0's second block partial
    2 Gw       BM       2          exact
    2 Gw + 1   5        3 / 2
    3 Gw + 1   5        4 / 3
    4 Gw + 1   5        5 / 4
    6 Gw + 1   5        7 / 6

Which wait each depth reaches, read from the kernels:

  k_wss_f32 (two plane buffers; waves 0-3 run E(i - 1), split(i + 1), MFMA(i); waves 4-7 MFMA(i), E(i), split(i + 1)).
    my = 1   every wait is wait_vm<0>; no split inside the loop.
    my = 2   the split waits: waves 0-3 wait_vm<PR> (i == 0), waves 4-7 wait_vm<S + PR>.  wait_rows still takes
             wait_vm<0> everywhere (waves 0-3: j + 2 < my fails; waves 4-7: j >= 1 && j + 1 < my fails).  kInit
             (the concat's second pass): wait_init 0 at i = 0, wait_vm<S> at i = 1.
    my = 3   wait_rows takes wait_vm<PA> for the first time (waves 0-3 at j = 0, waves 4-7 at j = 1); waves 0-3's
             second split waits wait_vm<S + PR>; plane buffer 0 is written a second time (block 2).  kInit: waves 0-3
             wait_vm<PA> at i = 0, waves 4-7 wait_vm<S + PA> at i = 1.
    my = 4   kInit waves 0-3 wait_vm<S + PA> at i = 1: every branch of every wait has now been taken.
    my >= 5  the same waits repeat (my = 5 / 7: both parities of the last block's plane buffer).
  k_ws_f32<256,256,EPI4> with g_prev (2-slot A ring, g_prev rows DMA'd into the block's dead A slot).
    my = 1   wait_vm<0> only.
    my = 2   wait_vm<S + PR2> at i = 1; the epilogue's wait is always wait_vm<0> with g_prev.
    my >= 3  A(i + 2) refills the slot that held g_prev(i).
    Its EPI 1 instantiations and EPI 4 without g_prev are unreachable: wss_enabled() is a constant true, so
    k_wss_f32 takes those calls.  They are not tested and no switch is added to reach them.
  k_ws_bf16 (NST-deep ring; iteration i waits kWaitSteady [kWaitSteady0 under zy] if i + NST - 2 < my and
  i >= NST - 1, kWaitEarly if i + NST - 2 < my and i < NST - 1, else wait_vm<0>).
    NST = 2  (K = 512, N = 128, ",wpc2"): Early (= 0) at i = 0, Steady at every i >= 1: reached at my = 2.
    NST = 3  (512,256 / 128,256 with accum; the combine with g_prev): my = 1: 0.  my = 2: Early, 0.  my = 3: Early,
             Early, 0.  my = 4: Early, Early, Steady, 0.  my >= 5: more Steady.
    NST = 4  (every other form): my <= 2: 0 only.  my = 3: Early, 0, 0.  my = 4: Early, Early, 0, 0.  my = 5: three
             Early, every slot refilled.  my = 6 / 7: Steady at i = 3 [, 4], then 0, 0.

Forms (one kernel instantiation each, asserted from the launch trace): FORMS below.  Checks per form:
  1  integer oracle: small-integer operands built on the CPU from a fixed seed, A with three nonzeros per row and every
     row different; every product, partial sum and stored value is exactly representable (asserted on the float64
     reference alone: it round-trips through the storage type, A and W fit one bf16 plane, and sum |a| |w| + |bias| +
     |accum| stays below 2^24 (fp32) / 2^8 (bf16) quanta), so the kernel must return the reference, no tolerance.  The
     eps gradient (per-workgroup partial sums) against float64 of the kernel's own C at 1e-5 sum |c x_dst|.
  4  guards, in the same call: 64 NaN rows behind every row operand, 64 poisoned rows behind every output.
  2  prefix consistency: dense random operands; the run on the first M rows equals rows [0, M) of the run at the
     largest M bit for bit: a row's arithmetic does not depend on its block, workgroup or the ring state.
  3  float64 bound at the largest M: tests/gemm_child.py's bounds (fp32 without its + 1 slack).
  5  strides: every row stride the ABI allows larger than the width, padding poisoned; bit-equal to the packed call.
  6  dispatch guard: A starting 4 bytes off 16-B alignment runs the tiled kernel and still meets the oracle.
  7  determinism: a second call at 3 Gw + 1 blocks gives the same bits, the eps gradient included.
and two outputs above 512 MiB (the non-temporal store branch, nt_io), M = 2^19 + 37."""
import ctypes
from dataclasses import dataclass

import pytest
import torch

from hgin import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF = torch.float32, torch.bfloat16
SLOPE, EPS = 0.25, 0.5          # PReLU slope, eps = eps2 of the integer oracle
POISON = -7.25
GUARD = 64


@dataclass(frozen=True)
class Form:
    name: str
    kind: str                   # "fwd" (gin_mlp_fwd) | "plain" (gemm_nt) | "comb" (gemm_nt_combine, cs = 0)
    dt: torch.dtype
    K: int
    N: int
    tags: tuple                 # the GEMM launches of the call, in order
    accum: bool = False
    save_z: bool = False
    zy: bool = False
    k1: int = 0                 # two-source A [a1 | (1 + eps2) a2]: the columns of a1 (0: one source)
    pad_a1: int = 0             # extra columns in a1's / a2's row stride
    pad_a2: int = 0
    want_gx: bool = False
    prev: bool = False

    @property
    def bm(self):
        return 64 if (self.dt == BF and self.K == 128) else 32

    @property
    def wpc(self):
        return 2 if self.tags[-1].endswith((",cpw64>", ",wpc2>")) else 1

    def __str__(self):
        return self.name


def _forms():
    f = []
    for r in (0, 1):
        for z in (0, 1):
            f.append(Form(f"f32_fwd_acc{r}_z{z}", "fwd", F32, 256, 256, (f"k_wss_f32<EPI1,{r},{z}>",), accum=bool(r),
                          save_z=bool(z)))
    for z in (1, 0):
        for pad in (0, 128):
            f.append(Form(f"f32_cat_z{z}" + ("_strided" if pad else ""), "fwd", F32, 512, 256,
                          ("k_wss_f32<EPI5,0,0>", f"k_wss_f32<EPI1,1,{z},init>"), save_z=bool(z), k1=256, pad_a2=pad))
    f.append(Form("f32_plain_k256", "plain", F32, 256, 256, ("k_wss_f32<EPI5,0,0>",)))
    f.append(Form("f32_plain_k128", "plain", F32, 128, 256, ("k_wss_f32<EPI5,0,0,K128>",)))
    f.append(Form("f32_plain_k128_strided", "plain", F32, 128, 256, ("k_wss_f32<EPI5,0,0,K128>",), pad_a1=64))
    for z in (1, 0):
        f.append(Form(f"f32_comb_gx{z}", "comb", F32, 256, 256, (f"k_wss_f32<EPI4,1,{z}>",), want_gx=bool(z)))
    f.append(Form("f32_comb_prev", "comb", F32, 256, 256, ("k_ws_f32<256,256,EPI4>",), want_gx=True, prev=True))

    def bf_tag(K, N, epi, rows_img):
        sfx = ",cpw64" if (N == 256 and K <= 256 and not rows_img) else ",wpc2" if (K == 512 and N == 128) else ""
        return (f"k_ws_bf16<{K},{N},EPI{epi}{sfx}>",)
    for K, N in ((512, 256), (256, 256), (128, 256), (512, 128), (256, 128), (128, 128)):
        f.append(Form(f"bf16_fwd_{K}x{N}_acc_z", "fwd", BF, K, N, bf_tag(K, N, 1, True), accum=True, save_z=True))
        f.append(Form(f"bf16_fwd_{K}x{N}", "fwd", BF, K, N, bf_tag(K, N, 1, False)))
    for K in (256, 512):
        f.append(Form(f"bf16_fwd_{K}x256_zy", "fwd", BF, K, 256, bf_tag(K, 256, 1, False), save_z=True, zy=True))
    f.append(Form("bf16_fwd_512x256_eps2_half", "fwd", BF, 512, 256, bf_tag(512, 256, 1, True), accum=True,
                  save_z=True, k1=256))
    f.append(Form("bf16_fwd_256x256_eps2_k64", "fwd", BF, 256, 256, bf_tag(256, 256, 1, False), save_z=True, k1=64))
    for K in (256, 128):
        f.append(Form(f"bf16_plain_{K}x256", "plain", BF, K, 256, bf_tag(K, 256, 0, False)))
    f.append(Form("bf16_comb_gx0", "comb", BF, 256, 256, bf_tag(256, 256, 4, True)))
    f.append(Form("bf16_comb_gx1", "comb", BF, 256, 256, bf_tag(256, 256, 4, True), want_gx=True))
    f.append(Form("bf16_comb_prev", "comb", BF, 256, 256, bf_tag(256, 256, 4, True), want_gx=True, prev=True))
    return f


FORMS = _forms()
# (id, blocks(Gw), rows of the last block(BM))
ROWS = [("n1_t1", lambda g: 1, lambda bm: 1), ("n1_tBM-1", lambda g: 1, lambda bm: bm - 1),
        ("n1_tBM", lambda g: 1, lambda bm: bm), ("n2_t1", lambda g: 2, lambda bm: 1),
        ("nG_tBM", lambda g: g, lambda bm: bm), ("nG+1_t5", lambda g: g + 1, lambda bm: 5),
        ("n2G_tBM", lambda g: 2 * g, lambda bm: bm), ("n2G+1_t5", lambda g: 2 * g + 1, lambda bm: 5),
        ("n3G+1_t5", lambda g: 3 * g + 1, lambda bm: 5), ("n4G+1_t5", lambda g: 4 * g + 1, lambda bm: 5),
        ("n6G+1_t5", lambda g: 6 * g + 1, lambda bm: 5)]
RIDS = [r[0] for r in ROWS]
LAST = RIDS[-1]
CASES = [(f, r) for f in FORMS for r in RIDS]          # form-major: a form's operands are built once
CASE_IDS = [f"{f}-{r}" for f, r in CASES]
ROW_IN = ("a1", "a2", "accum", "xd", "prev")            # operands with one row per output row
OUT_NAMES = {"fwd": ("z", "y"), "plain": ("c",), "comb": ("c", "gx")}
_grid = None


def grid():
    global _grid
    if _grid is None:
        _grid = torch.cuda.get_device_properties(0).multi_processor_count
    return _grid


def rows(form, rid):
    _, nblk, t = ROWS[RIDS.index(rid)]
    return form.bm * (nblk(grid() * form.wpc) - 1) + t(form.bm)


def blocks_per_workgroup(nblk, gw, b):
    """my of workgroup b, as the kernels compute it."""
    return (nblk - 1 - b) // gw + 1


def gemm_launches(kernels):
    return [k for k in kernels if k.startswith(("k_ws", "k_gemm_nt"))]


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------------------------
def sparse_rows(M, K, g, device):
    """[M, K] fp32: three nonzeros of +-1 / +-2 per row at distinct random columns, no two rows alike."""
    def draw(n):
        ri = lambda lo, hi, *s: torch.randint(lo, hi, s, generator=g, device=device)   # noqa: E731
        c0, d1, d2 = ri(0, K, n), ri(1, K // 2, n), ri(1, K // 2, n)                 # d1 + d2 < K: distinct columns
        cols = torch.stack((c0, c0 + d1, c0 + d1 + d2), 1) % K
        vals = ri(1, 3, n, 3) * (2 * ri(0, 2, n, 3) - 1)
        return torch.zeros(n, K, device=device).scatter_(1, cols, vals.float())
    a = draw(M)
    key = torch.randint(1, 1 << 40, (K,), generator=g, device=device)
    while True:
        _, inv, cnt = torch.unique((a.long() * key).sum(1), return_inverse=True, return_counts=True)
        dup = cnt[inv] > 1
        if not bool(dup.any()):
            return a
        a[dup] = draw(int(dup.sum()))


def split_sources(form, A):
    """{a1[, a2]} of the form from the whole A, in its storage type and row strides (padding: NaN)."""
    def strided(t, pad):
        if not pad:
            return t.to(form.dt).contiguous()
        buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), dtype=form.dt, device=t.device)
        buf[:, :t.shape[1]] = t
        return buf[:, :t.shape[1]]
    if not form.k1:
        return {"a1": strided(A, form.pad_a1)}
    return {"a1": strided(A[:, :form.k1], form.pad_a1), "a2": strided(A[:, form.k1:], form.pad_a2)}


def int_operands(form, M, seed, gen="cpu", device=DEV):
    """Small-integer operands of the form at M rows on ``device``, drawn on ``gen`` from ``seed``."""
    g = torch.Generator(device=gen).manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g, device=gen).float().to(device)   # noqa: E731
    one = lambda v: torch.tensor([v], dtype=F32, device=device)                                        # noqa: E731
    o = split_sources(form, sparse_rows(M, form.K, g, gen).to(device))
    o["w"] = ri(-2, 2, form.N, form.K).to(form.dt)
    if form.kind == "fwd":
        o["b"], o["slope"] = ri(-3, 3, form.N), one(SLOPE)
        if form.accum:
            o["accum"] = ri(-4, 4, M, form.N).to(form.dt)
        if form.k1:
            o["eps2"] = one(EPS)
    elif form.kind == "comb":
        o["xd"], o["eps"] = ri(-4, 4, M, form.N).to(form.dt), one(EPS)
        if form.prev:
            o["prev"] = ri(-4, 4, M, form.N).to(form.dt)
    return o


def int_reference(form, o):
    """The float64 evaluation of the form on integer operands, in the storage type, after asserting on it alone that
    the kernel can have no rounding to do: A and W fit one bf16 plane (the fp32 split's other two are zero), every
    output is a multiple of the quantum q below 2^24 q (fp32) / 2^8 q (bf16) even if all terms had one sign, and the
    reference round-trips through the storage type."""
    d = lambda t: t.double()   # noqa: E731
    A = d(o["a1"]) if "a2" not in o else torch.cat((d(o["a1"]), (1.0 + EPS) * d(o["a2"])), 1)
    W = d(o["w"])
    assert torch.equal(A, A.to(BF).double()) and torch.equal(W, W.to(BF).double())
    acc, mag = A @ W.t(), A.abs() @ W.abs().t()
    if form.kind == "fwd":
        z = acc + d(o["b"])
        y = torch.where(z > 0, z, SLOPE * z)
        mag = mag + d(o["b"]).abs()
        if form.accum:
            y, mag = y + d(o["accum"]), mag + d(o["accum"]).abs()
        ref, q = {"z": z, "y": y}, SLOPE * (0.5 if form.k1 else 1.0)
        if not form.save_z:
            del ref["z"]
    elif form.kind == "plain":
        ref, q = {"c": acc}, 1.0
    else:
        ref, q = {"c": acc}, 0.5
        mag = (1.0 + EPS) * mag
        if form.want_gx:
            ref["gx"] = (1.0 + EPS) * acc
            if form.prev:
                ref["gx"], mag = ref["gx"] + d(o["prev"]), mag + d(o["prev"]).abs()
    assert bool((mag < 2.0 ** (24 if form.dt == F32 else 8) * q).all()), (form.name, float(mag.max()), q)
    for k, r in ref.items():
        assert torch.equal(r, torch.round(r / q) * q) and torch.equal(r, r.to(form.dt).double()), (form.name, k)
    return {k: r.to(form.dt) for k, r in ref.items()}


def dense_operands(form, M):
    """Dense random operands as tests/gemm_child.py draws them."""
    g = torch.Generator(device=DEV).manual_seed(977 + FORMS.index(form))
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)               # noqa: E731
    one = lambda v: torch.tensor([v], dtype=F32, device=DEV)               # noqa: E731
    o = split_sources(form, rn(M, form.K))
    o["w"] = (rn(form.N, form.K) / form.K ** 0.5).to(form.dt)
    if form.kind == "fwd":
        o["b"], o["slope"] = rn(form.N), one(SLOPE)
        if form.accum:
            o["accum"] = rn(M, form.N).to(form.dt)
        if form.k1:
            o["eps2"] = one(0.37)
    elif form.kind == "comb":
        o["xd"], o["eps"] = rn(M, form.N).to(form.dt), one(0.3)
        if form.prev:
            o["prev"] = rn(M, form.N).to(form.dt)
    return o


def first_rows(o, M):
    return {k: (v[:M] if k in ROW_IN else v) for k, v in o.items()}


# ------------------------------------------------------------------------------------------------------------------
# launches
# ------------------------------------------------------------------------------------------------------------------
def launch(form, o, M, out):
    """The form's C entry point on the operands ``o`` (row views of any stride) into the buffers ``out`` ([rows, ld]
    tensors, written from their first element with row stride ld).  Returns the launch trace."""
    p, st, sfx = ops._p, ops._stream(o["w"]), "bf16" if form.dt == BF else "f32"
    K, N, a1, a2 = form.K, form.N, o["a1"], o.get("a2")
    ld = lambda t: t.stride(0) if t is not None else 0   # noqa: E731
    with _lib.trace_launches() as tr:
        if form.kind == "fwd":
            for name in ("z", "y"):
                assert name not in out or out[name].stride(0) == N       # packed by contract
            head = (p(a1), ld(a1), form.k1 or K, p(a2), ld(a2), p(o.get("eps2")), p(o["w"]), p(o["b"]), p(o["slope"]))
            if form.zy:
                _lib.call("hgin_gin_mlp_fwd_zy_bf16", *head, p(out["z"]), p(out["y"]), M, N, K, st)
            else:
                _lib.call(f"hgin_gin_mlp_fwd_{sfx}", *head, p(o.get("accum")), p(out.get("z")), p(out["y"]), M, N, K,
                          None, st)
        elif form.kind == "plain":
            _lib.call(f"hgin_gemm_nt_{sfx}", p(a1), ld(a1), p(o["w"]), K, p(out["c"]), ld(out["c"]), M, N, K, None, st)
        else:
            nbytes = ctypes.c_size_t(0)
            _lib.check(_lib.lib().hgin_gemm_nt_combine_workspace_size(M, N, ctypes.byref(nbytes)), "workspace_size")
            ws = ops._workspace(nbytes.value, a1.device)
            gx, prev = out.get("gx"), o.get("prev")
            _lib.call(f"hgin_gemm_nt_combine_{sfx}", p(a1), ld(a1), p(o["w"]), K, p(out["c"]), ld(out["c"]), M, N, K,
                      p(o["xd"]), ld(o["xd"]), p(gx), ld(gx), p(prev), ld(prev), 0, p(o["eps"]), p(out["ge"]), p(ws),
                      nbytes.value, None, st)
    return gemm_launches(tr.kernels)


def out_buffers(form, M, pads=None):
    """Poison-filled output buffers of M + GUARD rows (pads: extra columns per output name)."""
    out = {}
    for name in OUT_NAMES[form.kind]:
        if (name == "z" and not form.save_z) or (name == "gx" and not form.want_gx):
            continue
        out[name] = torch.full((M + GUARD, form.N + (pads or {}).get(name, 0)), POISON, dtype=form.dt, device=DEV)
    if form.kind == "comb":
        out["ge"] = torch.full((2,), POISON, dtype=F32, device=DEV)
    return out


def nan_tail(t, M):
    """Rows [0, M) of t in a fresh buffer of t's row stride, followed by GUARD rows of NaN."""
    buf = torch.full((M + GUARD, t.stride(0)), float("nan"), dtype=t.dtype, device=t.device)
    buf[:M, :t.shape[1]] = t[:M]
    return buf[:M, :t.shape[1]]


def run_guarded(form, o, M, **replace):
    """The form on rows [0, M) of ``o`` with NaN rows behind every row operand and poisoned rows behind every output."""
    og = {k: (nan_tail(v, M) if k in ROW_IN else v) for k, v in o.items()}
    og.update(replace)
    out = out_buffers(form, M)
    kernels = launch(form, og, M, out)
    torch.cuda.synchronize()
    return out, kernels


def check_oracle(form, out, ref, M, z_written):
    """Outputs equal to the reference exactly; guard rows untouched; the eps gradient within its bound."""
    for name in OUT_NAMES[form.kind]:
        if name not in out:
            continue
        buf = out[name]
        assert bool((buf[M:] == POISON).all()), (form.name, name, "guard rows written")
        if name == "z" and not z_written:      # zy with a positive slope: the weight-stationary kernel stores no z
            assert bool((buf == POISON).all()), (form.name, "z written under zy")
            continue
        got = buf[:M, :form.N]
        assert bool(torch.isfinite(got.float()).all()), (form.name, name, "NaN / inf in an output row")
        bad = (got != ref[name][:M]).any(1).nonzero().flatten()
        assert bad.numel() == 0, (form.name, name, f"{bad.numel()} wrong rows, first {bad[:8].tolist()}")
    if form.kind == "comb":
        assert float(out["ge"][1]) == POISON


def check_g_eps(ge, c, xd):
    """tests/gemm_child.py's bound: the eps gradient against float64 of the kernel's own C."""
    prod = c.double() * xd.double()
    assert abs(float(ge) - float(prod.sum())) <= 1e-5 * float(prod.abs().sum()), (float(ge), float(prod.sum()))


def run_ops(form, o, M):
    """The form through hgin.ops on rows [0, M) of ``o``: ({name: output}, launch trace)."""
    r = first_rows(o, M)
    with _lib.trace_launches() as tr:
        if form.kind == "fwd":
            z, y = ops.gin_mlp_fwd(r["a1"], r["w"], r["b"], r["slope"], r.get("accum"), save_z=form.save_z,
                                   comb2=r.get("a2"), eps2=r.get("eps2"), zy=form.zy)
            out = {"y": y}
            if form.save_z and not form.zy:
                out["z"] = z
        elif form.kind == "plain":
            out = {"c": ops.gemm_nt(r["a1"], r["w"])}
        else:
            prev = r["prev"].clone() if form.prev else None        # accumulated in place
            c, gx, ge = ops.gemm_nt_combine(r["a1"], r["w"], r["xd"], r["eps"], 0, form.want_gx, g_prev=prev)
            out = {"c": c, "ge": ge}
            if form.want_gx:
                out["gx"] = gx
    torch.cuda.synchronize()
    return out, gemm_launches(tr.kernels)


# computed once per form, shared by the tests below and left unchanged; dropped when the module is done
_int, _dense = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _drop_caches():
    yield
    _int.clear()
    _dense.clear()
    torch.cuda.empty_cache()


def int_case(form):
    if form.name not in _int:
        o = int_operands(form, rows(form, LAST), 4242 + FORMS.index(form))
        _int[form.name] = (o, int_reference(form, o))
    return _int[form.name]


def dense_case(form):
    if form.name not in _dense:
        M = rows(form, LAST)
        o = dense_operands(form, M)
        out, kernels = run_ops(form, o, M)
        assert kernels == list(form.tags), kernels
        _dense[form.name] = (o, out)
    return _dense[form.name]


# ------------------------------------------------------------------------------------------------------------------
# tests
# ------------------------------------------------------------------------------------------------------------------
def test_ws_tail_rows_per_workgroup():
    """The docstring's table: my of workgroup 0 / of the last workgroup at every row count."""
    gw = grid()
    want = {"n1_t1": (1, 1), "n1_tBM-1": (1, 1), "n1_tBM": (1, 1), "n2_t1": (1, 1), "nG_tBM": (1, 1),
            "nG+1_t5": (2, 1), "n2G_tBM": (2, 2), "n2G+1_t5": (3, 2), "n3G+1_t5": (4, 3), "n4G+1_t5": (5, 4),
            "n6G+1_t5": (7, 6)}
    for rid, nblk, _ in ROWS:
        n = nblk(gw)
        wgs = min(n, gw)
        assert (blocks_per_workgroup(n, gw, 0), blocks_per_workgroup(n, gw, wgs - 1)) == want[rid], rid
        assert sum(blocks_per_workgroup(n, gw, b) for b in range(wgs)) == n


@pytest.mark.parametrize("form,rid", CASES, ids=CASE_IDS)
def test_ws_tail_integer_oracle(form, rid):
    """Checks 1 and 4."""
    o, ref = int_case(form)
    M = rows(form, rid)
    out, kernels = run_guarded(form, o, M)
    assert kernels == list(form.tags), kernels
    check_oracle(form, out, ref, M, z_written=not form.zy)
    if form.kind == "comb":
        check_g_eps(out["ge"][0], out["c"][:M], o["xd"][:M])


@pytest.mark.parametrize("form,rid", CASES, ids=CASE_IDS)
def test_ws_tail_prefix(form, rid):
    """Check 2, and check 7 at 3 Gw + 1 blocks."""
    o, big = dense_case(form)
    M = rows(form, rid)
    out, kernels = run_ops(form, o, M)
    assert kernels == list(form.tags), kernels
    for name, t in out.items():
        if name != "ge":
            assert same_bits(t, big[name][:M]), (form.name, rid, name)
    if form.kind == "comb":
        check_g_eps(out["ge"], out["c"], o["xd"][:M])
    if rid == "n3G+1_t5":
        again, _ = run_ops(form, o, M)
        for name, t in out.items():
            assert same_bits(t, again[name]), (form.name, "second call", name)


@pytest.mark.parametrize("form", FORMS, ids=str)
def test_ws_tail_f64_bound(form):
    """Check 3: the largest M against float64 at tests/gemm_child.py's bounds for the entry point."""
    o, out = dense_case(form)
    d = lambda t: t.double()   # noqa: E731
    if "a2" in o:   # the kernels' self term: fp32 (1 + eps2) * a2, rounded once to the storage type
        sc = torch.tensor(1.0, device=DEV) + o["eps2"]
        A = torch.cat((d(o["a1"]), d((sc * o["a2"].float()).to(form.dt))), 1)
    else:
        A = d(o["a1"])
    W = d(o["w"])
    r, mag = A @ W.t(), A.abs() @ W.abs().t()
    if form.dt == F32:
        tol = lambda ref, m: 1e-6 * ref.abs() + 1e-5 * m              # noqa: E731
    else:
        tol = lambda ref, m: 2.0 ** -8 * ref.abs() + 1e-3 * (m + 1)    # noqa: E731
    if form.kind == "fwd":
        z = r + d(o["b"])
        y = torch.where(z > 0, z, SLOPE * z) + (d(o["accum"]) if form.accum else 0.0)
        if form.dt == F32:
            mag = mag + d(o["b"]).abs()
        assert bool(((d(out["y"]) - y).abs() <= tol(y, mag)).all()), (form.name, "y")
        if "z" in out:
            assert bool(((d(out["z"]) - z).abs() <= tol(z, mag)).all()), (form.name, "z")
        return
    c = out["c"]
    assert bool(((d(c) - r).abs() <= tol(r, mag)).all()), (form.name, "c")
    if form.kind == "comb":
        check_g_eps(out["ge"], c, o["xd"])
        if form.want_gx:
            sc = torch.tensor(1.0, device=DEV) + o["eps"]        # fp32 (1 + eps), then the product, [+ g_prev]
            gr = sc * c.float()
            if form.dt == F32:
                assert torch.equal(out["gx"], o["prev"] + gr if form.prev else gr), (form.name, "g_x_dst")
            else:
                gr = (o["prev"].float() + gr if form.prev else gr).to(BF).float()
                assert bool(((out["gx"].float() - gr).abs() <= 2.0 ** -7 * gr.abs() + 1e-6).all()), (form.name, "gx")


def padded(t, pad, fill):
    buf = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=t.dtype, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


@pytest.mark.parametrize("form", FORMS, ids=str)
def test_ws_tail_strided(form):
    """Check 5 at 2 Gw + 1 blocks: every row stride the ABI allows larger than the width (lda; for the dX forms ldc,
    ldxd, ldgd, ldgp too — the forward's z / y / accum are packed by contract), the padding poisoned."""
    o, _ = dense_case(form)
    M = rows(form, "n2G+1_t5")
    r = first_rows(o, M)
    packed = out_buffers(form, M)
    assert launch(form, r, M, packed) == list(form.tags)
    in_pads = {"a1": 8, "a2": 16} if form.kind == "fwd" else {"a1": 8, "xd": 24, "prev": 32}
    out_pads = {} if form.kind == "fwd" else {"c": 16, "gx": 8}
    s = {k: (padded(v, in_pads[k], float("nan")) if k in in_pads else v) for k, v in r.items()}
    for k in in_pads:
        assert k not in s or s[k].stride(0) > s[k].shape[1]
    out = out_buffers(form, M, out_pads)
    kernels = launch(form, s, M, out)
    torch.cuda.synchronize()
    assert kernels == list(form.tags), kernels
    for name, buf in out.items():
        if name == "ge":
            assert same_bits(buf, packed["ge"])
            continue
        assert same_bits(buf[:M, :form.N], packed[name][:M]), (form.name, name)
        assert bool((buf[M:] == POISON).all()) and bool((buf[:, form.N:] == POISON).all()), (form.name, name)


@pytest.mark.parametrize("form", FORMS, ids=str)
def test_ws_tail_misaligned_a_runs_tiled(form):
    """Check 6 at Gw + 1 blocks: A starting 4 bytes off 16-B alignment."""
    o, ref = int_case(form)
    M = rows(form, "nG+1_t5")
    off = 1 if form.dt == F32 else 2
    a1 = o["a1"][:M]
    buf = torch.full((M + GUARD, a1.shape[1] + 8), float("nan"), dtype=form.dt, device=DEV)
    buf[:M, off:off + a1.shape[1]] = a1
    a1 = buf[:M, off:off + a1.shape[1]]
    assert a1.data_ptr() % 16 == 4
    out, kernels = run_guarded(form, o, M, a1=a1)
    tiled = "k_gemm_nt<" if form.dt == F32 else "k_gemm_nt_bf16<"
    assert kernels and all(k.startswith(tiled) for k in kernels), kernels
    check_oracle(form, out, ref, M, z_written=True)
    if form.kind == "comb":
        check_g_eps(out["ge"][0], out["c"][:M], o["xd"][:M])


LARGE = [f for f in FORMS if f.name in ("f32_fwd_acc1_z1", "f32_comb_gx1")]


@pytest.mark.parametrize("form", LARGE, ids=str)
def test_ws_tail_large_output(form):
    """Outputs above 512 MiB take the non-temporal store branch (nt_io): M = 2^19 + 37 at N = 256, the smallest M past
    the threshold.  Integer-oracle operands generated on the device; the exact reference is a float64 matmul there, in
    row chunks."""
    M = (1 << 19) + 37
    assert M * form.N * 4 > (512 << 20) >= (M - 37) * form.N * 4
    o = int_operands(form, M, 99 + FORMS.index(form), gen=DEV)
    out = out_buffers(form, M)
    kernels = launch(form, o, M, out)
    torch.cuda.synchronize()
    assert kernels == list(form.tags), kernels
    step = 1 << 16
    for r0 in range(0, M, step):
        n = min(step, M - r0)
        oc = {k: (v[r0:r0 + n] if k in ROW_IN else v) for k, v in o.items()}
        ref = int_reference(form, oc)
        for name, want in ref.items():
            bad = (out[name][r0:r0 + n] != want).any(1).nonzero().flatten()
            assert bad.numel() == 0, (form.name, name, f"{bad.numel()} wrong rows from {r0 + int(bad[0])}")
    for name in ref:
        assert bool((out[name][M:] == POISON).all()), (form.name, name, "guard rows written")
    if form.kind == "comb":
        check_g_eps(out["ge"][0], out["c"][:M], o["xd"])
        assert float(out["ge"][1]) == POISON
