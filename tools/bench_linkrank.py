#!/usr/bin/env python3
"""Time full-candidate link ranking (A15, ``link_full_ranks``), unfiltered and filtered, against what a user would
write in torch today, on one GPU in one process.

Shapes: the ('path', 'uses', 'link') relation of CONFIGS[cfg] as tools/bench_linkpred.py plans it (n_path sources,
n_link destinations, F = the config's hidden width); the queries are the first ``--queries`` positives, the known
edges the whole relation.  The torch baseline scores a chunk of queries against every destination
(``z_src[pos[0, chunk]] @ z_dst.T``, the chunk sized to about 1 GB of fp32 scores), masks the known pairs, compares
with the positive's own entry and sums the rows; its pair lists are prepared outside the timed region, as the fused
path's CSR of the known edges is (cached on the tensor).  Both paths get identical inputs, are warmed up per shape
and alternate; every timed repeat is ``inner`` calls between two HIP events.  Reported per shape: median / min / max
of the repeats, the ratio, whether the fused path is faster by more than the spread (its slowest repeat under the
baseline's fastest), the fused path's fp32-equivalent rate 2 Q n_dst F / t beside the 157 TF/s peak of the fp32 MFMA
it uses, and how many queries the two paths count differently (torch's GEMM rounds its sums in another order).
There is no CPU fallback: without a HIP device the tool prints the plan and fails.

    python tools/bench_linkrank.py --out profiles/linkrank/linkrank_bench.json
    python tools/bench_linkrank.py --graphs 8      # profiles/linkseg/linkrank_seg_bench.json, "full_rank_sweep"
    python tools/bench_linkrank.py --configs cfg1 --scale 0.1 --queries 64      # a tiny run

``--graphs G`` (include/hgin.h A19; default 1: everything above, unchanged) cuts the relation into G equal graphs with
the queries sorted by graph and times ``link_full_ranks`` with ``segments=`` against the same call without it.
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
SPLIT_PEAK = 1247.0e12 / 6     # six bf16 products per fp32 product (the ceiling of the split-mode GEMMs)
CHUNK_BYTES = 1 << 30          # fp32 scores the baseline holds at a time


def _linkpred_tool():
    spec = importlib.util.spec_from_file_location("bench_linkpred", os.path.join(ROOT, "tools", "bench_linkpred.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def plan(configs, queries: int, scale: float):
    shapes = []
    for s in _linkpred_tool().plan(configs, [1], scale):
        Q = min(int(queries), s["E"])
        shapes.append({"config": s["config"], "scale": scale, "n_src": s["n_src"], "n_dst": s["n_dst"], "E": s["E"],
                       "F": s["F"], "Q": Q, "flop": 2 * Q * s["n_dst"] * s["F"],
                       "score_bytes_not_materialised": 4 * Q * s["n_dst"],
                       "baseline_chunk_rows": max(1, CHUNK_BYTES // (4 * s["n_dst"]))})
    return shapes


def _baseline(torch, z_src, z_dst, pos, chunk_rows, pairs=None):
    """Chunked scores in torch.  ``pairs`` = (query index, destination, per-chunk offsets) of the known pairs to mask
    (sorted by query, the positives' own destinations left out), or None for the unfiltered ranks."""
    Q, n_dst = int(pos.size(1)), int(z_dst.size(0))
    gt = torch.empty(Q, dtype=torch.int32, device=pos.device)
    eq = torch.empty(Q, dtype=torch.int32, device=pos.device)
    for i, lo in enumerate(range(0, Q, chunk_rows)):
        hi = min(Q, lo + chunk_rows)
        sc = z_src[pos[0, lo:hi]] @ z_dst.T
        thr = sc.gather(1, pos[1, lo:hi, None])
        if pairs is not None:
            a, b = pairs[2][i], pairs[2][i + 1]
            sc[pairs[0][a:b] - lo, pairs[1][a:b]] = float("-inf")
        gt[lo:hi] = (sc > thr).sum(1)
        eq[lo:hi] = (sc == thr).sum(1) - 1   # the positive's own entry
    return gt, eq


def _known_pairs(torch, pos_q, rowptr, col, chunk_rows):
    """(query index, destination) of every known neighbour of every query's source other than its own destination,
    sorted by query, with the offsets of the baseline's chunks."""
    Q = int(pos_q.size(1))
    rp = rowptr.long()
    beg, deg = rp[pos_q[0]], rp[pos_q[0] + 1] - rp[pos_q[0]]
    qi = torch.repeat_interleave(torch.arange(Q, device=pos_q.device), deg)
    first = torch.cumsum(deg, 0) - deg
    c = col.long()[beg[qi] + (torch.arange(qi.numel(), device=qi.device) - first[qi])]
    keep = c != pos_q[1][qi]
    qi, c = qi[keep], c[keep]
    bounds = torch.arange(0, Q + chunk_rows, chunk_rows, device=qi.device).clamp(max=Q)
    return qi, c, torch.searchsorted(qi, bounds).tolist()


def split_graphs(n_src, n_dst, E, graphs, seed, device="cpu"):
    """tools/bench_linkpred.py's cut of a shape into ``graphs`` equal graphs, positives sorted by graph."""
    return _linkpred_tool().split_graphs(n_src, n_dst, E, graphs, seed, device)


def run_graphs(torch, shape, graphs, repeats, warmup, target_ms, seed=1234):
    """The ``--graphs G`` measurements of one shape: the relation cut into G equal graphs, the queries Q positives
    sorted by graph (every 128-query block then covers about n_dst / G destinations), the known edges the whole
    relation; ``link_full_ranks`` with ``segments=`` against the same call without it on the same tensors, unfiltered
    and filtered, alternating in one run."""
    lp = _linkpred_tool()
    from hgin.linkpred import LinkSegments, link_full_ranks
    dev = "cuda"
    n_src, n_dst, E, F, Q = (shape[x] for x in ("n_src", "n_dst", "E", "F", "Q"))
    known, batch_src, batch_dst = split_graphs(n_src, n_dst, E, graphs, seed, dev)
    seg = LinkSegments(batch_src, batch_dst, graphs)
    pick = (torch.arange(Q, dtype=torch.long, device=dev) * E) // Q   # Q positives spread over every graph, in order
    pos = known[:, pick].contiguous()
    g = torch.Generator(device=dev).manual_seed(seed)
    z_src = torch.randn(n_src, F, generator=g, device=dev) * 0.1
    z_dst = torch.randn(n_dst, F, generator=g, device=dev) * 0.1
    paths = {"unsegmented_unfiltered": lambda _: link_full_ranks(z_src, z_dst, pos),
             "segmented_unfiltered": lambda _: link_full_ranks(z_src, z_dst, pos, segments=seg),
             "unsegmented_filtered": lambda _: link_full_ranks(z_src, z_dst, pos, known),
             "segmented_filtered": lambda _: link_full_ranks(z_src, z_dst, pos, known, segments=seg)}
    for _ in range(warmup):
        for fn in paths.values():
            fn(0)
    torch.cuda.synchronize()
    inner = {name: lp._inner_for(torch, fn, target_ms) for name, fn in paths.items()}
    times = {name: [] for name in paths}
    for _ in range(repeats):      # the paths alternate
        for name, fn in paths.items():
            times[name].append(lp._timed(torch, fn, inner[name], 0))
    out = dict(shape, graphs=graphs, queries="sorted by graph")
    for name in paths:
        out[name] = dict(lp._stats(times[name]), inner=inner[name])
    for kind in ("unfiltered", "filtered"):
        a, b = out["segmented_" + kind], out["unsegmented_" + kind]
        out[f"segmented_over_unsegmented_{kind}"] = a["median_ms"] / b["median_ms"]
        out[f"segmented_faster_beyond_spread_{kind}"] = a["max_ms"] < b["min_ms"]
    del z_src, z_dst, pos, known
    torch.cuda.empty_cache()
    return out


def run_shape(torch, shape, repeats, warmup, target_ms, seed=1234):
    lp = _linkpred_tool()
    from hgin.linkpred import _known_csr, link_full_ranks
    dev = "cuda"
    n_src, n_dst, E, F, Q = (shape[x] for x in ("n_src", "n_dst", "E", "F", "Q"))
    g = torch.Generator(device=dev).manual_seed(seed)
    known = torch.stack([torch.randint(0, n_src, (E,), generator=g, device=dev),
                         torch.randint(0, n_dst, (E,), generator=g, device=dev)])
    pos = known[:, :Q].contiguous()
    z_src = torch.randn(n_src, F, generator=g, device=dev) * 0.1
    z_dst = torch.randn(n_dst, F, generator=g, device=dev) * 0.1
    chunk = shape["baseline_chunk_rows"]
    rowptr, col = _known_csr(known, n_src, n_dst)
    pairs = _known_pairs(torch, pos, rowptr, col, chunk)
    out = dict(shape, known_pairs_masked=int(pairs[0].numel()))

    paths = {"fused_unfiltered": lambda _: link_full_ranks(z_src, z_dst, pos),
             "fused_filtered": lambda _: link_full_ranks(z_src, z_dst, pos, known),
             "torch_unfiltered": lambda _: _baseline(torch, z_src, z_dst, pos, chunk),
             "torch_filtered": lambda _: _baseline(torch, z_src, z_dst, pos, chunk, pairs)}
    res = {}
    for _ in range(warmup):
        for name, fn in paths.items():
            res[name] = fn(0)
    torch.cuda.synchronize()
    for kind in ("unfiltered", "filtered"):
        f, t = res["fused_" + kind], res["torch_" + kind]
        out[f"queries_counted_differently_{kind}"] = int(((f[0] != t[0]) | (f[1] != t[1])).sum())
    inner = {name: lp._inner_for(torch, fn, target_ms) for name, fn in paths.items()}
    times = {name: [] for name in paths}
    for _ in range(repeats):      # the paths alternate
        for name, fn in paths.items():
            times[name].append(lp._timed(torch, fn, inner[name], 0))
    for name in paths:
        out[name] = dict(lp._stats(times[name]), inner=inner[name])
    for kind in ("unfiltered", "filtered"):
        f, t = out["fused_" + kind], out["torch_" + kind]
        rate = shape["flop"] / (f["median_ms"] * 1e-3)
        f.update(fp32_equivalent_tflops=rate / 1e12, fraction_of_f32_mfma_peak=rate / F32_MFMA_PEAK)
        out[f"torch_over_fused_{kind}"] = t["median_ms"] / f["median_ms"]
        out[f"fused_faster_beyond_spread_{kind}"] = f["max_ms"] < t["min_ms"]
    del z_src, z_dst, pos, known, pairs
    torch.cuda.empty_cache()
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--configs", default="cfg2,cfg3")
    ap.add_argument("--queries", type=int, default=65536)
    ap.add_argument("--scale", type=float, default=1.0, help="multiply every node / edge count (tiny runs)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--target-ms", type=float, default=30.0, help="device time of one timed repeat, at least")
    ap.add_argument("--graphs", type=int, default=1,
                    help="cut every shape into G equal graphs, queries sorted by graph, and time link_full_ranks with "
                         "segments= against the same call without (include/hgin.h A19); 1: today's measurements")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.repeats < 5:
        ap.error("--repeats must be at least 5")
    if args.queries < 1 or args.warmup < 1:
        ap.error("--queries and --warmup must be at least 1")
    if args.graphs < 1:
        ap.error("--graphs must be at least 1")
    shapes = plan(args.configs.split(","), args.queries, args.scale)
    for s in shapes:
        print("plan:", json.dumps(s), file=sys.stderr)

    import torch
    if not torch.cuda.is_available():
        print("bench_linkrank: no HIP device is visible; the link-ranking path has no CPU fallback", file=sys.stderr)
        return 2
    from hgin import _lib
    _lib.lib()
    if args.graphs > 1:
        results = [run_graphs(torch, s, args.graphs, args.repeats, args.warmup, args.target_ms) for s in shapes]
        doc = {"tool": "tools/bench_linkrank.py", "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
               "warmup": args.warmup, "graphs": args.graphs, "shapes": results}
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(doc, indent=1) + "\n")
        print(json.dumps(doc))
        return 0
    results = [run_shape(torch, s, args.repeats, args.warmup, args.target_ms) for s in shapes]
    flags = [r[f"fused_faster_beyond_spread_{k}"] for r in results for k in ("unfiltered", "filtered")]
    doc = {"tool": "tools/bench_linkrank.py", "device": torch.cuda.get_device_name(0),
           "f32_mfma_peak_flop_per_s": F32_MFMA_PEAK, "split_peak_flop_per_s": SPLIT_PEAK,
           "arithmetic": "v_mfma_f32_32x32x2_f32", "repeats": args.repeats, "warmup": args.warmup, "shapes": results,
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
