#!/usr/bin/env python3
"""Time forward + backward of the full-candidate softmax denominator (A23, ``link_lse``) against its unfused torch form
(``link_lse_unfused``: chunked ``z_src[src] @ z_dst.T``, masked, ``torch.logsumexp``), on one GPU in one process.

Shapes: in-batch negatives (4096 sources x 4096 destinations, F = 128 and 256) and 4096 sources against every link of
cfg2 (300k, F = 128) and cfg3 (3M, F = 256), each without and with a ``known`` edge set of average degree 6 per source.
What is timed: ``lse = f(z_src, z_dst, src, T, known); lse.sum().backward()`` with gradients on both embeddings.  The two
paths get identical inputs, are warmed up per shape and alternate; every timed window is ``inner`` calls between two HIP
events and ends in a synchronise.  Reported per shape and path: median / min / max of the windows, unfused / fused, and
whether the fused path is faster by more than the spread (its slowest window under the baseline's fastest).  FLOPs are
computed from the shapes: the forward sweep is 2 Q n_dst F, each gradient kernel recomputes it once per chunk of output
features (one chunk up to F = 256) and adds a second product of the same size.  Per-kernel rates against the f32-MFMA
peak come from a separate ``rocprofv3 --kernel-trace --stats`` run of this tool on ONE shape name, whose kernel trace
``--rates-from`` then reduces (median duration of each A23 kernel, divided into ``kernel_flop``; needs no device).
There is no CPU fallback: without a HIP device the tool prints the plan and fails.

``--graphs G`` (A24) cuts every shape into G equal graphs (sources, queries and destinations; the remainders are
dropped) and times ``link_lse(segments=)`` forward + backward against the same call without ``segments`` and against
``link_lse_unfused(segments=)``: the same tensors, the three paths alternating in one run, once with the queries sorted
by graph and once shuffled; known edges (where the shape has them) stay inside the source's graph.

    python tools/bench_linklse.py --out profiles/linklse/linklse_bench.json
    python tools/bench_linklse.py --scale 0.01 --queries 256          # a tiny run
    rocprofv3 --kernel-trace --stats -d prof -o cfg2 --output-format csv -- python tools/bench_linklse.py --only cfg2
    python tools/bench_linklse.py --only cfg2 --rates-from prof/cfg2_kernel_trace.csv --out rates_cfg2.json
    python tools/bench_linklse.py --graphs 8 --only inbatch_f128,cfg2 --out profiles/linklse/linklse_seg_bench.json
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
CHUNK_BYTES = 1 << 30          # fp32 scores per chunk of the unfused path
KNOWN_DEGREE = 6


def feature_chunk(F: int) -> int:
    """Output features per backward workgroup (csrc/hgin_linklse.hip lse_feature_chunk)."""
    return 256 if F > 128 else 128


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def kernel_flop(Q: int, n_dst: int, F: int) -> dict:
    """fp32 FLOPs of each kernel from the shapes: the sweep is one Q x n_dst x F product; a gradient kernel recomputes
    it for every chunk of output features (128, or 256 once F exceeds 128) and multiplies the Q x n_dst tile of weights
    into F output features."""
    sweep = 2 * Q * n_dst * F
    chunks = -(-F // feature_chunk(F))
    bwd = chunks * sweep + sweep
    return {"k_lse_sweep": sweep, "k_lse_bwd_src": bwd, "k_lse_bwd_dst": bwd, "total": sweep + 2 * bwd}


TRACED = {"k_lse_sweep": "k_lse_sweep<", "k_lse_bwd_src": ", false,", "k_lse_bwd_dst": ", true,"}


def kernel_rates(trace_csv: str, shape: dict) -> dict:
    """Per A23 kernel of a rocprofv3 kernel trace (CSV) of a run on ``shape`` alone: launches, median duration and the
    fp32 FLOP rate ``kernel_flop`` gives it, against the f32-MFMA peak.  The gradient kernels are told apart by their
    second template argument (k_lse_bwd<VEC, DST, NU>)."""
    import csv
    import statistics
    us = {k: [] for k in TRACED}
    with open(trace_csv, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            for k, mark in TRACED.items():
                if ("k_lse_bwd<" in name and mark in name) if k != "k_lse_sweep" else mark in name:
                    us[k].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    out = {}
    for k, v in us.items():
        if not v:
            raise ValueError(f"{trace_csv}: no launch of {k}")
        med = statistics.median(v)
        rate = shape["flop"][k] / (med * 1e-6)
        out[k] = {"launches": len(v), "median_us": med, "flop": shape["flop"][k], "tflops": rate / 1e12,
                  "fraction_of_f32_mfma_peak": rate / F32_MFMA_PEAK}
    return out


def plan(scale: float = 1.0, queries: int = 4096):
    from hgin.data import CONFIGS
    shapes = []

    def add(name, n_src, n_dst, F, Q):
        for deg in (0, KNOWN_DEGREE):
            shapes.append({"name": name, "scale": scale, "n_src": n_src, "n_dst": n_dst, "F": F, "Q": Q,
                           "known_degree": deg, "flop": kernel_flop(Q, n_dst, F),
                           "score_bytes_not_materialised": 4 * Q * n_dst,
                           "baseline_chunk_rows": max(1, CHUNK_BYTES // (4 * n_dst))})

    Q = max(1, int(queries))
    add("inbatch_f128", Q, Q, 128, Q)
    add("inbatch_f256", Q, Q, 256, Q)
    for cfg, F in (("cfg2", 128), ("cfg3", 256)):
        n_dst = max(1, int(CONFIGS[cfg].n_link * scale))
        add(cfg, Q, n_dst, F, Q)
    return shapes


def seg_plan(shape: dict, graphs: int) -> dict:
    """``shape`` cut into ``graphs`` equal graphs: every count rounded down to a multiple of G; ``flop`` is the
    unsegmented work of the cut shape, ``flop_seg`` the work the candidates need (1 / G of it)."""
    G = int(graphs)
    if G < 1 or G > min(shape["Q"], shape["n_src"], shape["n_dst"]):
        raise ValueError(f"--graphs must be in [1, min(Q, n_src, n_dst)], got {G}")
    out = dict(shape, graphs=G)
    for k in ("Q", "n_src", "n_dst"):
        out[k] = shape[k] - shape[k] % G
    out["queries_per_graph"], out["dst_per_graph"] = out["Q"] // G, out["n_dst"] // G
    out["flop"] = kernel_flop(out["Q"], out["n_dst"], out["F"])
    out["flop_seg"] = {k: v // G for k, v in out["flop"].items()}
    out["score_bytes_not_materialised"] = 4 * out["Q"] * out["n_dst"]
    out["baseline_chunk_rows"] = max(1, CHUNK_BYTES // (4 * out["n_dst"]))
    return out


def run_seg_shape(torch, shape, repeats, warmup, target_ms, seed=1234):
    """``shape`` = a ``seg_plan``.  Per query order (sorted by graph, shuffled): the three paths' windows, segmented over
    unsegmented, and whether the difference is beyond the spread."""
    lp = _tool("bench_linkpred")
    from hgin.linkpred import LinkSegments, link_lse, link_lse_unfused
    dev = "cuda"
    n_src, n_dst, F, Q, deg, G = (shape[x] for x in ("n_src", "n_dst", "F", "Q", "known_degree", "graphs"))
    g = torch.Generator(device=dev).manual_seed(seed)
    z_src = (torch.randn(n_src, F, generator=g, device=dev) * 0.1).requires_grad_(True)
    z_dst = (torch.randn(n_dst, F, generator=g, device=dev) * 0.1).requires_grad_(True)
    per_src, per_dst = n_src // G, n_dst // G
    batch_src = torch.arange(n_src, device=dev) // per_src
    segments = LinkSegments(batch_src, torch.arange(n_dst, device=dev) // per_dst, G)
    shuffled = torch.randperm(n_src, generator=g, device=dev)[:Q].contiguous()
    orders = {"sorted": shuffled[torch.sort(batch_src[shuffled], stable=True).indices].contiguous(),
              "shuffled": shuffled}
    chunk = shape["baseline_chunk_rows"]
    out = dict(shape)
    for order, src in orders.items():
        known = None
        if deg:
            s_rep = src.repeat_interleave(deg)
            inside = torch.randint(0, per_dst, (Q * deg,), generator=g, device=dev)
            known = torch.stack([s_rep, batch_src[s_rep] * per_dst + inside])

        def step_of(fn, **kw):
            def step(_):
                z_src.grad = z_dst.grad = None
                lse = fn(z_src, z_dst, src, 0.5, known, **kw)
                lse.sum().backward()
                return lse
            return step

        paths = {"seg": step_of(link_lse, segments=segments), "unseg": step_of(link_lse),
                 "unfused_seg": step_of(link_lse_unfused, chunk_rows=chunk, segments=segments)}
        res, grads = {}, {}
        for _ in range(warmup):
            for name, fn in paths.items():
                res[name] = fn(0).detach()
                grads[name] = (z_src.grad.clone(), z_dst.grad.clone())
        torch.cuda.synchronize()
        o = {"max_abs_lse_difference": float((res["seg"] - res["unfused_seg"]).abs().max()),
             "max_abs_grad_difference": max(float((a - b).abs().max())
                                            for a, b in zip(grads["seg"], grads["unfused_seg"]))}
        res.clear()
        grads.clear()
        inner = {name: lp._inner_for(torch, fn, target_ms) for name, fn in paths.items()}
        times = {name: [] for name in paths}
        for _ in range(repeats):      # the paths alternate
            for name, fn in paths.items():
                times[name].append(lp._timed(torch, fn, inner[name], 0))
        for name in paths:
            o[name] = dict(lp._stats(times[name]), inner=inner[name])
            print(f"{shape['name']} known={deg} G={G} {order}: {name}: median {o[name]['median_ms']:.3f} ms "
                  f"[{o[name]['min_ms']:.3f} - {o[name]['max_ms']:.3f}]", file=sys.stderr, flush=True)
        o["seg_over_unseg"] = o["seg"]["median_ms"] / o["unseg"]["median_ms"]
        o["seg_faster_beyond_spread"] = o["seg"]["max_ms"] < o["unseg"]["min_ms"]
        o["seg_slower_beyond_spread"] = o["seg"]["min_ms"] > o["unseg"]["max_ms"]
        o["unfused_seg_over_seg"] = o["unfused_seg"]["median_ms"] / o["seg"]["median_ms"]
        out[order] = o
    del z_src, z_dst
    torch.cuda.empty_cache()
    return out


def run_shape(torch, shape, repeats, warmup, target_ms, seed=1234):
    lp = _tool("bench_linkpred")
    from hgin.linkpred import link_lse, link_lse_unfused
    dev = "cuda"
    n_src, n_dst, F, Q, deg = (shape[x] for x in ("n_src", "n_dst", "F", "Q", "known_degree"))
    g = torch.Generator(device=dev).manual_seed(seed)
    z_src = (torch.randn(n_src, F, generator=g, device=dev) * 0.1).requires_grad_(True)
    z_dst = (torch.randn(n_dst, F, generator=g, device=dev) * 0.1).requires_grad_(True)
    src = torch.randperm(n_src, generator=g, device=dev)[:Q].contiguous()
    known = None
    if deg:
        known = torch.stack([src.repeat_interleave(deg), torch.randint(0, n_dst, (Q * deg,), generator=g, device=dev)])
    chunk = shape["baseline_chunk_rows"]

    def step_of(fn, **kw):
        def step(_):
            z_src.grad = z_dst.grad = None
            lse = fn(z_src, z_dst, src, 0.5, known, **kw)
            lse.sum().backward()
            return lse
        return step

    paths = {"fused": step_of(link_lse), "unfused": step_of(link_lse_unfused, chunk_rows=chunk)}
    res, grads = {}, {}
    for _ in range(warmup):
        for name, fn in paths.items():
            res[name] = fn(0).detach()
            grads[name] = (z_src.grad.clone(), z_dst.grad.clone())
    torch.cuda.synchronize()
    out = dict(shape)
    out["max_abs_lse_difference"] = float((res["fused"] - res["unfused"]).abs().max())
    out["max_abs_grad_difference"] = max(float((a - b).abs().max()) for a, b in zip(grads["fused"], grads["unfused"]))
    res.clear()
    grads.clear()
    inner = {name: lp._inner_for(torch, fn, target_ms) for name, fn in paths.items()}
    times = {name: [] for name in paths}
    for _ in range(repeats):      # the paths alternate
        for name, fn in paths.items():
            times[name].append(lp._timed(torch, fn, inner[name], 0))
    for name in paths:
        out[name] = dict(lp._stats(times[name]), inner=inner[name])
        print(f"{shape['name']} known={deg}: {name}: median {out[name]['median_ms']:.3f} ms", file=sys.stderr,
              flush=True)
    rate = shape["flop"]["total"] / (out["fused"]["median_ms"] * 1e-3)
    out["fused"].update(fp32_tflops=rate / 1e12, fraction_of_f32_mfma_peak=rate / F32_MFMA_PEAK)
    out["unfused_over_fused"] = out["unfused"]["median_ms"] / out["fused"]["median_ms"]
    out["fused_faster_beyond_spread"] = out["fused"]["max_ms"] < out["unfused"]["min_ms"]
    del z_src, z_dst, src, known
    torch.cuda.empty_cache()
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scale", type=float, default=1.0, help="multiply the cfg2 / cfg3 destination counts (tiny runs)")
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--only", default=None, help="comma-separated shape names to run")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--target-ms", type=float, default=30.0, help="device time of one timed window, at least")
    ap.add_argument("--out", default=None)
    ap.add_argument("--graphs", type=int, default=0, metavar="G",
                    help="cut every shape into G equal graphs and time link_lse(segments=) against the unsegmented call "
                         "and link_lse_unfused(segments=), queries sorted by graph and shuffled")
    ap.add_argument("--rates-from", default=None, metavar="TRACE.csv",
                    help="reduce the rocprofv3 kernel trace of a run on the one shape named by --only; no device needed")
    args = ap.parse_args(argv)
    if args.repeats < 5:
        ap.error("--repeats must be at least 5")
    if args.queries < 1 or args.warmup < 1:
        ap.error("--queries and --warmup must be at least 1")
    if args.graphs < 0 or (args.graphs and args.rates_from):
        ap.error("--graphs must be positive and does not combine with --rates-from")
    shapes = plan(args.scale, args.queries)
    if args.only:
        shapes = [s for s in shapes if s["name"] in args.only.split(",")]
    if args.graphs:
        try:
            shapes = [seg_plan(s, args.graphs) for s in shapes]
        except ValueError as e:
            ap.error(str(e))
    for s in shapes:
        print("plan:", json.dumps(s), file=sys.stderr)
    if args.rates_from:
        if len({s["name"] for s in shapes}) != 1:
            ap.error("--rates-from needs --only with exactly one shape name")
        s = shapes[0]
        doc = {"tool": "tools/bench_linklse.py --rates-from", "shape": s["name"], "Q": s["Q"], "n_dst": s["n_dst"],
               "F": s["F"], "f32_mfma_peak_flop_per_s": F32_MFMA_PEAK, "kernels": kernel_rates(args.rates_from, s)}
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(doc, indent=1) + "\n")
        print(json.dumps(doc))
        return 0

    import torch
    if not torch.cuda.is_available():
        print("bench_linklse: no HIP device is visible; the full softmax loss has no CPU fallback", file=sys.stderr)
        return 2
    from hgin import _lib
    _lib.lib()
    if args.graphs:
        results = [run_seg_shape(torch, s, args.repeats, args.warmup, args.target_ms) for s in shapes]
        doc = {"tool": f"tools/bench_linklse.py --graphs {args.graphs}", "device": torch.cuda.get_device_name(0),
               "graphs": args.graphs, "repeats": args.repeats, "warmup": args.warmup, "shapes": results}
    else:
        results = [run_shape(torch, s, args.repeats, args.warmup, args.target_ms) for s in shapes]
        doc = {"tool": "tools/bench_linklse.py", "device": torch.cuda.get_device_name(0),
               "f32_mfma_peak_flop_per_s": F32_MFMA_PEAK, "arithmetic": "v_mfma_f32_32x32x2_f32",
               "repeats": args.repeats, "warmup": args.warmup, "shapes": results,
               "fused_faster_at_every_shape": all(r["fused_faster_beyond_spread"] for r in results)}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))
    return 0


if __name__ == "__main__":
    sys.exit(main())
