#!/usr/bin/env python3
"""Time ``hgin.link_split`` (include/hgin.h A21) on the ('path', 'uses', 'link') relation of CONFIGS[cfg] and its
flipped reverse against the obvious torch formulation on the same tensors, on one GPU in one process.

Two things are timed per shape and ``--disjoint`` value:
  (a) fused   ``link_split(graph, REL_PL, val, test, disjoint, seed)``: two part launches (forward and reverse
              relation), six stable selections of the forward relation ({0}, {0,1}, {0,1,2}, {1}, {2}, {3}; with
              disjoint = 0 parts {0,1} and {1} need none) and three of the reverse one, the host reads of the counts
              included;
  (b) torch   ``torch.rand`` masks over the edge positions, then ``edge_index[:, mask]`` and ``mask.nonzero()`` for the
              same selections and ``rev[:, mask]`` for the reverse relation's.  This is a split by position:
              it does not hold every copy of a pair out (tests/test_gpu_linksplit.py), it is here as the cost a user
              pays today.
Both get the same edge tensors, are warmed up per shape and alternate; every timed repeat is ``inner`` calls between two
HIP events.  Reported per case: median / min / max of the repeats, torch / fused, whether the fused path is faster than
torch by more than the spread (its slowest repeat under torch's fastest) or slower by more than it, and for the fused path
the bytes its kernels move by design (computed from E and the part counts) over the median: an end-to-end rate that
includes the eight to eleven host reads, not a kernel's share of peak.  No ratio is promised: the exit status is 0 when the run completed.
There is no CPU fallback: without a HIP device the tool prints the plan and fails.

    python tools/bench_linksplit.py --out profiles/linksplit/linksplit_bench.json
    python tools/bench_linksplit.py --configs cfg1 --scale 0.5          # a tiny run
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

HBM_PEAK = 8.0e12      # MI355X HBM3E, bytes / s (datasheet)


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def plan(configs, scale: float, disjoints=(0.0, 0.3), val=0.1, test=0.1):
    from hgin.data import CONFIGS, scaled_config
    shapes = []
    for name in configs:
        cfg = CONFIGS[name] if scale == 1.0 else scaled_config(CONFIGS[name], scale)
        shapes.append(dict(config=cfg.name, n_src=cfg.n_path, n_dst=cfg.n_link, E=cfg.e_pl, val=val, test=test,
                           disjoints=[float(d) for d in disjoints]))
    return shapes


def designed_bytes(E: int, counts, disjoint: float) -> int:
    """Bytes the fused path's kernels read and write by design: per relation one part launch (16 B read, 1 B written per
    edge); per selection 1 B per edge in the count, 1 + 16 B per edge in the scatter (tiles without a kept edge read
    less: not modelled) and 24 B per kept edge; tile counts and offsets are noise."""
    size = lambda parts: sum(counts[p] for p in parts)  # noqa: E731
    fwd = [(0,), (0, 1, 2), (2,), (3,)] + ([(0, 1), (1,)] if disjoint > 0 else [])
    rev = [(0,), (0, 1, 2)] + ([(0, 1)] if disjoint > 0 else [])
    total = 2 * E * 17
    for parts in fwd + rev:
        total += E * 18 + 24 * size(parts)
    return total


def _torch_split(torch, ei, rev, val, test, disjoint, gen):
    """The split a user writes today: masks from ``torch.rand`` over the edge positions."""
    E = ei.size(1)
    r = torch.rand(E, device=ei.device, generator=gen)
    is_test = r < test
    is_val = (r < test + val) & ~is_test
    held = is_test | is_val
    if disjoint > 0:
        is_sup = (torch.rand(E, device=ei.device, generator=gen) < disjoint) & ~held
    else:
        is_sup = torch.zeros_like(held)
    msg = ~(held | is_sup)
    graphs = [msg, msg | is_sup, ~is_test] if disjoint > 0 else [msg, ~is_test]     # val graph = train graph at 0
    masks = graphs + [is_val, is_test] + ([is_sup] if disjoint > 0 else [])
    out = [(ei[:, m], m.nonzero().flatten()) for m in masks]
    out += [rev[:, m] for m in graphs]
    return out


def run_shape(torch, shape, repeats, warmup, target_ms, seed=1234):
    lp = _tool("bench_linkpred")
    import hgin
    from hgin.data import REL_LP, REL_PL, HeteroGraph
    dev = "cuda"
    n_src, n_dst, E, val, test = (shape[x] for x in ("n_src", "n_dst", "E", "val", "test"))
    g = torch.Generator(device=dev).manual_seed(seed)
    ei = torch.stack([torch.randint(0, n_src, (E,), generator=g, device=dev),
                      torch.randint(0, n_dst, (E,), generator=g, device=dev)])
    rev = ei.flip(0).contiguous()
    one = torch.zeros(1, 1, device=dev)
    graph = HeteroGraph({"path": one, "link": one}, {REL_PL: ei, REL_LP: rev}, one.flatten(),
                        {"path": one.flatten().long(), "link": one.flatten().long()})
    out = dict(shape, cases={})
    for disjoint in shape["disjoints"]:
        paths = {"fused": lambda step: hgin.link_split(graph, REL_PL, val=val, test=test, disjoint=disjoint, seed=step),
                 "torch": lambda step: _torch_split(torch, ei, rev, val, test, disjoint, g)}
        for _ in range(warmup):
            for fn in paths.values():
                fn(0)
        torch.cuda.synchronize()
        sp = hgin.link_split(graph, REL_PL, val=val, test=test, disjoint=disjoint, seed=0)
        assert torch.equal(sp.train_graph.edge_index[REL_LP], sp.train_graph.edge_index[REL_PL].flip(0))
        case = {"disjoint": disjoint, "counts": list(sp.counts), "fused_bytes": designed_bytes(E, sp.counts, disjoint)}
        del sp
        inner = {name: lp._inner_for(torch, fn, target_ms) for name, fn in paths.items()}
        times = {name: [] for name in paths}
        for _ in range(repeats):      # the paths alternate
            for name, fn in paths.items():
                times[name].append(lp._timed(torch, fn, inner[name], 1))
        for name in paths:
            case[name] = dict(lp._stats(times[name]), inner=inner[name])
            print(f"{shape['config']} disjoint {disjoint}: {name}: median {case[name]['median_ms']:.3f} ms",
                  file=sys.stderr, flush=True)
        f, t = case["fused"], case["torch"]
        rate = case["fused_bytes"] / (f["median_ms"] * 1e-3)
        f.update(end_to_end_bytes_per_s=rate, fraction_of_hbm_peak=rate / HBM_PEAK)
        case["torch_over_fused"] = t["median_ms"] / f["median_ms"]
        case["fused_faster_beyond_spread"] = f["max_ms"] < t["min_ms"]
        case["fused_slower_beyond_spread"] = f["min_ms"] > t["max_ms"]
        out["cases"][f"disjoint_{disjoint:g}"] = case
        torch.cuda.empty_cache()
    del ei, rev, graph
    torch.cuda.empty_cache()
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--configs", default="cfg2,cfg3")
    ap.add_argument("--disjoint", default="0,0.3", help="comma-separated disjoint fractions, each timed")
    ap.add_argument("--scale", type=float, default=1.0, help="multiply every node / edge count (tiny runs)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--target-ms", type=float, default=30.0, help="device time of one timed repeat, at least")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.repeats < 5:
        ap.error("--repeats must be at least 5")
    if args.warmup < 1:
        ap.error("--warmup must be at least 1")
    shapes = plan(args.configs.split(","), args.scale, [float(d) for d in args.disjoint.split(",")])
    for s in shapes:
        print("plan:", json.dumps(s), file=sys.stderr)

    import torch
    if not torch.cuda.is_available():
        print("bench_linksplit: no HIP device is visible; the split kernels have no CPU fallback", file=sys.stderr)
        return 2
    from hgin import _lib
    _lib.lib()
    results = [run_shape(torch, s, args.repeats, args.warmup, args.target_ms) for s in shapes]
    doc = {"tool": "tools/bench_linksplit.py", "device": torch.cuda.get_device_name(0),
           "hbm_peak_bytes_per_s": HBM_PEAK, "repeats": args.repeats, "warmup": args.warmup, "shapes": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))
    return 0


if __name__ == "__main__":
    sys.exit(main())
