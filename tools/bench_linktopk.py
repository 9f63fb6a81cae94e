#!/usr/bin/env python3
"""Time top-K link retrieval (A16, ``link_topk``), unfiltered and filtered, against what a user would write in torch
today and against the sweep without a selection, on one GPU in one process.

Shapes: the ('path', 'uses', 'link') relation of CONFIGS[cfg] as tools/bench_linkrank.py plans it; the queries are the
sources of the first ``--queries`` positives, the known edges the whole relation.  Three things are timed per shape:
  (a) fused     ``link_topk(z_src, z_dst, src, k[, known])`` for every k of ``--ks``;
  (b) torch     a chunk of queries against every destination (``z_src[src[chunk]] @ z_dst.T``, the chunk sized to about
                1 GB of fp32 scores), the known pairs set to -inf from lists prepared outside the timed region (as the
                fused path's CSR of the known edges is cached on the tensor), then ``torch.topk``: the baseline;
  (c) floor     ``link_full_ranks`` on the same queries: the same sweep with a counting epilogue, no selection.
All paths get identical inputs, are warmed up per shape and alternate; every timed repeat is ``inner`` calls between
two HIP events.  Reported per shape and path: median / min / max of the repeats; per k and filter: torch / fused,
fused / floor (the selection overhead), whether the fused path is faster than torch by more than the spread (its
slowest repeat under the baseline's fastest), and how many rows the two paths fill differently (torch's GEMM rounds
its sums in another order and ``torch.topk`` orders ties as it likes).  The exit status gates k = ``--gate-k`` only.
There is no CPU fallback: without a HIP device the tool prints the plan and fails.

    python tools/bench_linktopk.py --out profiles/linktopk/linktopk_bench.json
    python tools/bench_linktopk.py --configs cfg1 --scale 0.1 --queries 64      # a tiny run
"""
import argparse
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "gnn-link-prediction_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

F32_MFMA_PEAK = 157.0e12       # v_mfma_f32_32x32x2_f32, FLOP / s


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def plan(configs, queries: int, scale: float, ks=(10, 100)):
    shapes = _tool("bench_linkrank").plan(configs, queries, scale)
    for s in shapes:
        s["ks"] = [int(k) for k in ks]
    return shapes


def _baseline(torch, z_src, z_dst, src, k, chunk_rows, pairs=None):
    """Chunked scores + ``torch.topk``.  ``pairs`` = (query index, destination, per-chunk offsets) of the known pairs
    to mask (sorted by query), or None for the unfiltered result."""
    Q = int(src.numel())
    idx = torch.empty((Q, k), dtype=torch.int64, device=src.device)
    val = torch.empty((Q, k), dtype=torch.float32, device=src.device)
    for i, lo in enumerate(range(0, Q, chunk_rows)):
        hi = min(Q, lo + chunk_rows)
        sc = z_src[src[lo:hi]] @ z_dst.T
        if pairs is not None:
            a, b = pairs[2][i], pairs[2][i + 1]
            sc[pairs[0][a:b] - lo, pairs[1][a:b]] = float("-inf")
        val[lo:hi], idx[lo:hi] = torch.topk(sc, k, dim=1)
    return idx, val


def run_shape(torch, shape, repeats, warmup, target_ms, seed=1234):
    lp, lr = _tool("bench_linkpred"), _tool("bench_linkrank")
    from hgin.linkpred import _known_csr, link_full_ranks, link_topk
    dev = "cuda"
    n_src, n_dst, E, F, Q = (shape[x] for x in ("n_src", "n_dst", "E", "F", "Q"))
    g = torch.Generator(device=dev).manual_seed(seed)
    known = torch.stack([torch.randint(0, n_src, (E,), generator=g, device=dev),
                         torch.randint(0, n_dst, (E,), generator=g, device=dev)])
    pos = known[:, :Q].contiguous()
    src = pos[0].contiguous()
    z_src = torch.randn(n_src, F, generator=g, device=dev) * 0.1
    z_dst = torch.randn(n_dst, F, generator=g, device=dev) * 0.1
    chunk = shape["baseline_chunk_rows"]
    rowptr, col = _known_csr(known, n_src, n_dst)
    # every known neighbour of every query's source (no destination is left out: -1 matches none)
    pairs = lr._known_pairs(torch, torch.stack([src, torch.full_like(src, -1)]), rowptr, col, chunk)
    out = dict(shape, known_pairs_masked=int(pairs[0].numel()))

    paths = {"floor_ranks_unfiltered": lambda _: link_full_ranks(z_src, z_dst, pos),
             "floor_ranks_filtered": lambda _: link_full_ranks(z_src, z_dst, pos, known)}
    for k in shape["ks"]:
        k = min(k, n_dst)
        paths[f"fused_k{k}_unfiltered"] = lambda _, k=k: link_topk(z_src, z_dst, src, k)
        paths[f"fused_k{k}_filtered"] = lambda _, k=k: link_topk(z_src, z_dst, src, k, known)
        paths[f"torch_k{k}_unfiltered"] = lambda _, k=k: _baseline(torch, z_src, z_dst, src, k, chunk)
        paths[f"torch_k{k}_filtered"] = lambda _, k=k: _baseline(torch, z_src, z_dst, src, k, chunk, pairs)
    res = {}
    for _ in range(warmup):
        for name, fn in paths.items():
            res[name] = fn(0)
    torch.cuda.synchronize()
    cases = [(min(k, n_dst), kind) for k in shape["ks"] for kind in ("unfiltered", "filtered")]
    for k, kind in cases:
        f, t = res[f"fused_k{k}_{kind}"], res[f"torch_k{k}_{kind}"]
        out[f"rows_filled_differently_k{k}_{kind}"] = int((f[0].long() != t[0]).any(1).sum())
    res.clear()
    inner = {}
    for name, fn in paths.items():
        inner[name] = lp._inner_for(torch, fn, target_ms)
        print(f"{shape['config']}: {name}: {inner[name]} call(s) per timed repeat", file=sys.stderr, flush=True)
    times = {name: [] for name in paths}
    for _ in range(repeats):      # the paths alternate
        for name, fn in paths.items():
            times[name].append(lp._timed(torch, fn, inner[name], 0))
    for name in paths:
        out[name] = dict(lp._stats(times[name]), inner=inner[name])
        print(f"{shape['config']}: {name}: median {out[name]['median_ms']:.3f} ms", file=sys.stderr, flush=True)
    for k, kind in cases:
        f, t, c = out[f"fused_k{k}_{kind}"], out[f"torch_k{k}_{kind}"], out[f"floor_ranks_{kind}"]
        rate = shape["flop"] / (f["median_ms"] * 1e-3)
        f.update(fp32_equivalent_tflops=rate / 1e12, fraction_of_f32_mfma_peak=rate / F32_MFMA_PEAK)
        out[f"torch_over_fused_k{k}_{kind}"] = t["median_ms"] / f["median_ms"]
        out[f"fused_over_floor_k{k}_{kind}"] = f["median_ms"] / c["median_ms"]
        out[f"fused_faster_beyond_spread_k{k}_{kind}"] = f["max_ms"] < t["min_ms"]
    del z_src, z_dst, pos, src, known, pairs
    torch.cuda.empty_cache()
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--configs", default="cfg2,cfg3")
    ap.add_argument("--queries", type=int, default=65536)
    ap.add_argument("--ks", default="10,100", help="comma-separated k values (each in [1, 128])")
    ap.add_argument("--gate-k", type=int, default=10, help="the k whose comparison decides the exit status")
    ap.add_argument("--scale", type=float, default=1.0, help="multiply every node / edge count (tiny runs)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--target-ms", type=float, default=30.0, help="device time of one timed repeat, at least")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    ks = [int(k) for k in args.ks.split(",")]
    if args.repeats < 5:
        ap.error("--repeats must be at least 5")
    if args.queries < 1 or args.warmup < 1:
        ap.error("--queries and --warmup must be at least 1")
    if any(k < 1 or k > 128 for k in ks) or args.gate_k not in ks:
        ap.error("--ks must lie in [1, 128] and contain --gate-k")
    shapes = plan(args.configs.split(","), args.queries, args.scale, ks)
    for s in shapes:
        print("plan:", json.dumps(s), file=sys.stderr)

    import torch
    if not torch.cuda.is_available():
        print("bench_linktopk: no HIP device is visible; the top-K retrieval path has no CPU fallback",
              file=sys.stderr)
        return 2
    from hgin import _lib
    _lib.lib()
    results = [run_shape(torch, s, args.repeats, args.warmup, args.target_ms) for s in shapes]
    flags = [r[f"fused_faster_beyond_spread_k{min(args.gate_k, r['n_dst'])}_{kind}"] for r in results
             for kind in ("unfiltered", "filtered")]
    doc = {"tool": "tools/bench_linktopk.py", "device": torch.cuda.get_device_name(0),
           "f32_mfma_peak_flop_per_s": F32_MFMA_PEAK, "arithmetic": "v_mfma_f32_32x32x2_f32",
           "repeats": args.repeats, "warmup": args.warmup, "gate_k": args.gate_k, "shapes": results,
           "fused_faster_at_every_shape": all(flags)}
    text = json.dumps(doc)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    print(text)
    return 0 if doc["fused_faster_at_every_shape"] else 1


if __name__ == "__main__":
    sys.exit(main())
