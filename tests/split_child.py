"""Child process of tests/test_gpu_split_planes.py: every fp32 GEMM form of csrc/hgin_gemm_nt.hip and
csrc/hgin_gemm_tn.hip under the process-static HGIN_* switches its parent set, on the exact three-plane oracles of
tests/split_oracles.py.  Each case runs through hgin.ops with 64 NaN rows behind every row operand and 64 poisoned rows
behind every output the op allocates (GuardedTorch), records its launch trace, and compares every output tensor with
the float64 reference bit for bit (g_eps / g_b / g_a, sums over per-workgroup partials, at the project's 1e-5 forms).
Nothing is asserted here but the references' own conditions: the findings go to the parent as JSON.

The operands and the float64 references are built on the device with plain torch operations (split_oracles' builders
with device="cuda": elementwise arithmetic, index_add, for D1 / D1m a float64 matmul — all exact here, as the
conditions assert), which keeps a switch set at a few seconds; tests/test_split_planes_host.py runs the same builders
on the CPU.  A weight-stationary NT case at M rows is the first M rows of the case built at the largest row count.

    python tests/split_child.py OUT.json

{case id: {"kernels": [launch tags], "fail": [what differed], "rows": M}}; a case id is form/rows/oracle."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "gnn-link-prediction_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import split_oracles as so  # noqa: E402
from hgin import _lib, ops  # noqa: E402

DEV = "cuda"
GUARD = 64
POISON = -7.25
GEMM_TAGS = ("k_ws", "k_gemm_nt", "k_gemm_tn", "k_tn_small")

# NT forms: name -> (kind, N, K, keywords of so.nt_case, rows, misaligned A).  Rows: "ws" = 1, BM Gw + 5, BM (3 Gw) + 5
# with BM = 32 and Gw = the CU count (the weight-stationary forms: workgroups of 1, 2 / 1 and 4 / 3 blocks, every wait
# branch taken — the table of tests/test_gpu_ws_tail.py); a number = that many rows.
NT_FORMS = {
    "fwd256_acc0_z0": ("fwd", 256, 256, dict(), "ws", False, dict(save_z=False)),
    "fwd256_acc0_z1": ("fwd", 256, 256, dict(), "ws", False, dict()),
    "fwd256_acc1_z0": ("fwd", 256, 256, dict(accum=True), "ws", False, dict(save_z=False)),
    "fwd256_acc1_z1": ("fwd", 256, 256, dict(accum=True), "ws", False, dict()),
    "cat512_z1": ("fwd", 256, 512, dict(k1=256), "ws", False, dict()),
    "cat512_z0": ("fwd", 256, 512, dict(k1=256), "ws", False, dict(save_z=False)),
    "cat512_z1_off256": ("fwd", 256, 512, dict(k1=256, off=256), "ws", False, dict()),
    "plain256_k256": ("plain", 256, 256, dict(), "ws", False, dict()),
    "plain256_k128": ("plain", 256, 128, dict(), "ws", False, dict()),
    "comb256_gx0": ("comb", 256, 256, dict(), "ws", False, dict(want_gx=False)),
    "comb256_gx1": ("comb", 256, 256, dict(), "ws", False, dict()),
    "comb256_prev": ("comb", 256, 256, dict(prev=True), "ws", False, dict()),
    # the tiled k_gemm_nt at every tile and epilogue
    "t64x128_fwd": ("fwd", 128, 128, dict(), 300, False, dict()),
    "t128x128_lin_k256": ("lin", 128, 256, dict(), 70_001, False, dict()),
    "t128x128_plain_k128": ("plain", 128, 128, dict(), 70_001, False, dict()),
    "t128x128_comb_k128": ("comb", 128, 128, dict(prev=True), 70_001, False, dict()),
    "t128x256_fwd_k384": ("fwd", 256, 384, dict(accum=True), 35_001, False, dict()),
    "t256x32_fwd": ("fwd", 32, 128, dict(accum=True), 4_101, False, dict()),
    "t256x32_fwd_n7": ("fwd", 7, 64, dict(), 4_101, False, dict()),
    "t_unclean_k100": ("fwd", 128, 100, dict(), 4_101, False, dict()),
    "t_misaligned_a": ("fwd", 256, 256, dict(accum=True), 8_197, True, dict()),
    "t_cat512_acc": ("fwd", 256, 512, dict(k1=256, accum=True), 35_001, False, dict()),
}
# TN forms: name -> (N, K1, K2, how: "plain" (gemm_tn) | "fused" (mlp_bwd_w, g_z returned) | "fused_nogz", rows).
# Rows "ws" = 1, 17, 16 G + 1, 96 G + 5 (tests/test_gpu_wsd_tail.py: start-up, steady state and tail of both rings).
TN_FORMS = {}
for _n, _k1, _k2 in ((256, 256, 0), (256, 128, 0), (128, 128, 0), (128, 256, 0), (128, 384, 128), (256, 256, 256)):
    for _how in ("plain", "fused"):
        TN_FORMS[f"tn_n{_n}_k{_k1}+{_k2}_{_how}"] = (_n, _k1, _k2, _how, "ws")
for _n, _k1, _k2 in ((128, 384, 0), (64, 64, 0), (100, 77, 0), (32, 128, 0), (17, 64, 64)):
    for _how in ("plain", "fused", "fused_nogz"):
        TN_FORMS[f"tt_n{_n}_k{_k1}+{_k2}_{_how}"] = (_n, _k1, _k2, _how, 4_101)


class GuardedTorch:
    """Stands in for the torch module inside hgin.ops: an fp32 output it allocates is the leading rows of a larger,
    poisoned buffer, so a store past the last row is seen."""

    def __init__(self):
        self.bufs = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *shape, **kw):
        if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
            shape = tuple(shape[0])
        if kw.get("dtype") is torch.float32 and shape and shape[0] > 0:
            buf = torch.full((shape[0] + GUARD,) + tuple(shape[1:]), POISON, dtype=torch.float32, device=kw["device"])
            self.bufs.append((buf, shape[0]))
            return buf[:shape[0]]
        return torch.empty(*shape, **kw)

    def empty_like(self, t, **kw):
        return self.empty(*t.shape, dtype=t.dtype, device=t.device)

    def untouched(self):
        return all(bool((b[n:] == POISON).all()) for b, n in self.bufs)


def guarded_rows(t, off=0):
    """t [M, w] on the device as the leading rows of a NaN buffer (off: columns to skip, 4 bytes each)."""
    M, w = t.shape
    ld = w + (8 if off else 0)
    buf = torch.full((M + GUARD, ld), float("nan"), dtype=torch.float32, device=DEV)
    buf[:M, off:off + w] = t
    return buf[:M, off:off + w]


def one(v):
    return torch.tensor([v], dtype=torch.float32, device=DEV)


def run_guarded(fn):
    """fn() through hgin.ops with guarded outputs and the launch trace: (result, gemm launches, guards untouched)."""
    gt = GuardedTorch()
    ops.torch = gt
    try:
        with _lib.trace_launches() as tr:
            res = fn()
        torch.cuda.synchronize()
    finally:
        ops.torch = torch
    return res, [k for k in tr.kernels if k.startswith(GEMM_TAGS)], gt.untouched()


def compare(fail, name, got, ref):
    """got (device fp32) against the float64 reference, bit for bit."""
    want = ref.float()
    assert torch.equal(want.double(), ref)
    if got is None or got.shape != want.shape:
        fail.append(f"{name}: missing or misshapen")
    elif not torch.equal(got, want):
        bad = (got != want) | (got != got)
        i = bad.nonzero()[0].tolist()
        fail.append(f"{name}: {int(bad.sum())} of {bad.numel()} differ, first at {i}: got "
                    f"{float(got[tuple(i)])!r} want {float(want[tuple(i)])!r}")


def selfcheck():
    """compare() itself: silent on equal tensors, reports one element that is off by one ulp, and a NaN."""
    ref = so.values("T3", (64, 32), torch.Generator(device=DEV).manual_seed(1)).double()
    got, fails = ref.float(), ([], [], [])
    compare(fails[0], "same", got.clone(), ref)
    ulp = got.clone()
    ulp[5, 7] = torch.nextafter(ulp[5, 7], torch.tensor(9.0, device=DEV))
    compare(fails[1], "ulp", ulp, ref)
    nan = got.clone()
    nan[63, 31] = float("nan")
    compare(fails[2], "nan", nan, ref)
    return not fails[0] and "1 of 2048 differ, first at [5, 7]" in fails[1][0] and "[63, 31]" in fails[2][0]


_nt_cache = {}
ROW_IN = ("a1", "a2", "accum", "xd", "prev")


def nt_case(oracle, kind, M, Mmax, N, K, seed, kw):
    """The case at M rows: the first M rows of the case built once at Mmax (every condition is one per output row,
    and a selector's column depends on its own row alone)."""
    key = (oracle, kind, Mmax, N, K, seed, tuple(sorted(kw.items())))
    if key not in _nt_cache:
        if len(_nt_cache) > 6:
            _nt_cache.clear()
        _nt_cache[key] = so.nt_case(oracle, kind, Mmax, N, K, seed, device=DEV, **kw)
    c = _nt_cache[key]
    return {"in": {k: (v[:M] if k in ROW_IN else v) for k, v in c["in"].items()},
            "ref": {k: v[:M] for k, v in c["ref"].items()}, "table": c["table"]}


def run_nt(name, M, Mmax, oracle, seed):
    kind, N, K, kw, _, mis, okw = NT_FORMS[name]
    c = nt_case(oracle, kind, M, Mmax, N, K, seed, kw)
    i, ref, fail = c["in"], c["ref"], []
    a1 = guarded_rows(i["a1"], 1 if mis else 0)
    assert a1.data_ptr() % 16 == (4 if mis else 0)
    a2 = guarded_rows(i["a2"]) if "a2" in i else None
    w = i["w"].to(DEV)
    row = lambda k: guarded_rows(i[k]) if k in i else None   # noqa: E731
    if kind in ("fwd", "lin"):
        save_z = okw.get("save_z", True) and kind == "fwd"
        (z, y), kernels, clean = run_guarded(lambda: ops.gin_mlp_fwd(
            a1, w, i["b"].to(DEV), one(so.SLOPE) if kind == "fwd" else None, row("accum"), save_z=save_z, comb2=a2,
            eps2=one(so.SCALE - 1.0) if a2 is not None else None))
        compare(fail, "y", y, ref["y"])
        if save_z:
            compare(fail, "z", z, ref["z"])
    elif kind == "plain":
        out, kernels, clean = run_guarded(lambda: ops.gemm_nt(a1, w))
        compare(fail, "c", out, ref["c"])
    else:
        want_gx = okw.get("want_gx", True)
        xd, prev = row("xd"), row("prev")
        (out, gx, ge), kernels, clean = run_guarded(lambda: ops.gemm_nt_combine(
            a1, w, xd, one(so.SCALE - 1.0), 0, want_gx, g_prev=prev))
        compare(fail, "c", out, ref["c"])
        if want_gx:
            compare(fail, "g_x_dst", gx, ref["gx"])
            if prev is not None and not bool(torch.isnan(prev._base[M:]).all()):   # accumulated in place
                fail.append("g_prev: guard rows written")
        prod = ref["c"] * i["xd"].double()
        if not abs(float(ge) - float(prod.sum())) <= 1e-5 * float(prod.abs().sum()):
            fail.append(f"g_eps: {float(ge)!r} want {float(prod.sum())!r}")
    if not clean:
        fail.append("guard rows behind an output written")
    outs = [t for t in ((z, y) if kind in ("fwd", "lin") else (out,)) if t is not None]
    return {"kernels": kernels, "fail": fail, "rows": M, "table": c["table"], "_out": outs}


def run_tn(name, M, oracle, seed):
    N, K1, K2, how, _ = TN_FORMS[name]
    c = so.tn_case(oracle, M, N, K1 + K2, seed, how != "plain", device=DEV)
    i, ref, fail = c["in"], c["ref"], []
    b1 = guarded_rows(i["b"][:, :K1].contiguous())
    b2 = guarded_rows(i["b"][:, K1:].contiguous()) if K2 else None
    if how == "plain":
        gz = guarded_rows(ref["g_z"].float())
        out, kernels, clean = run_guarded(lambda: ops.gemm_tn(gz, b1, b2))
        compare(fail, "g_w", out, ref["g_w"])
    else:
        gy, z = guarded_rows(i["gy"]), guarded_rows(i["z"])
        (g_w, g_a, g_b, g_z), kernels, clean = run_guarded(lambda: ops.mlp_bwd_w(
            gy, z, one(so.SLOPE), b1, b2, want_gz=how == "fused"))
        compare(fail, "g_w", g_w, ref["g_w"])
        if how == "fused":
            compare(fail, "g_z", g_z, ref["g_z"])
        # test_wsd_prelu_fused_equals_two_pass's bounds
        if not bool(((g_b.double() - ref["g_b"]).abs() <= 1e-5 * ref["g_b_mag"] + 1e-6).all()):
            fail.append("g_b out of its bound")
        if not abs(float(g_a) - float(ref["g_a"])) <= 1e-5 * (float(ref["g_a_mag"]) + 1):
            fail.append(f"g_a: {float(g_a)!r} want {float(ref['g_a'])!r}")
    if not clean:
        fail.append("guard rows behind an output written")
    return {"kernels": kernels, "fail": fail, "rows": M, "table": c["table"]}


def planes_case(G):
    """hgin_nt_planes_f32: the 128 x 128 / 128 x 256 tiles with B copied from the pre-split planes and splitting B
    themselves: the same bits, both the oracle's."""
    res = {}
    if not ops.BDMA:
        return res
    for name in ("t128x128_lin_k256", "t128x128_plain_k128", "t128x256_fwd_k384"):
        for oracle in ("O2", "O3"):       # W dense T3; W a T2 selector
            M = NT_FORMS[name][4]
            with_planes = run_nt(name, M, M, oracle, 77)
            ops.BDMA = False
            try:
                without = run_nt(name, M, M, oracle, 77)
            finally:
                ops.BDMA = True
            if not all(torch.equal(p, q) for p, q in zip(with_planes["_out"], without["_out"])):
                without["fail"].append("differs from the run on pre-split planes")
            res[f"planes/{name}/{oracle}/with"] = with_planes
            res[f"planes/{name}/{oracle}/without"] = without
    return res


def main():
    torch.cuda.init()
    G = torch.cuda.get_device_properties(0).multi_processor_count
    res = {}
    for name, form in NT_FORMS.items():
        rows = (1, 32 * G + 5, 96 * G + 5) if form[4] == "ws" else (form[4],)
        for M in rows:
            for oi, oracle in enumerate(so.NT_ORACLES):
                res[f"{name}/{M}/{oracle}"] = run_nt(name, M, rows[-1], oracle, 1000 + oi)
                res[f"{name}/{M}/{oracle}"].pop("_out")
    for fi, (name, form) in enumerate(TN_FORMS.items()):
        rows = (1, 17, 16 * G + 1, 96 * G + 5) if form[4] == "ws" else (17, form[4])
        for M in rows:
            for oi, oracle in enumerate(so.TN_ORACLES):
                res[f"{name}/{M}/{oracle}"] = run_tn(name, M, oracle, 5000 + 10 * fi + oi)
    res.update(planes_case(G))
    for v in res.values():
        v.pop("_out", None)
    res["_meta"] = {"cus": G, "selfcheck": selfcheck(),
                    "env": {k: v for k, v in os.environ.items() if k.startswith("HGIN_")}}
    with open(sys.argv[1], "w") as f:
        json.dump(res, f)
    print("split child done", res["_meta"], sum(bool(v.get("fail")) for k, v in res.items() if k != "_meta"),
          "failing of", len(res) - 1, flush=True)


if __name__ == "__main__":
    main()
