#!/usr/bin/env python3
"""Time the fused sampled link loss (A13) against the unfused ``link_loss`` (A10 + A11 + torch BCE), and the ranking
kernel (A14), on one GPU in one process.

Shapes: the ('path', 'uses', 'link') relation of CONFIGS[cfg] (n_path sources, n_link destinations, e_pl positives,
F = the config's hidden width), k negatives per positive.  Both paths get identical inputs (same positives, same
embeddings, same seed and offsets), run forward + backward, are warmed up per shape and alternate; every timed
repeat is ``inner`` iterations between two HIP events (inner chosen from the warm-up so that a repeat is tens of
milliseconds).  Reported per shape: median / min / max of the repeats for both paths, their ratio, whether the fused
path is faster by more than the spread (its slowest repeat under link_loss's fastest), the fused forward alone with
its algorithmic bytes and fraction of the 8 TB/s HBM peak, and the ranking kernel.  A path that runs out of memory is
recorded as such.  There is no CPU fallback: without a HIP device the tool prints the plan and fails.

``--objective`` (include/hgin.h A17) adds the softmax / bpr / selfadv epilogues: for each one the fused forward +
backward against ``link_loss`` with the same objective, timed like the bce pair and alternating with it in the same
repeat loop, reported under the shape's "objectives" with the ratio to the fused bce step of the same run ("all" runs
bce too, whose rows are produced as without the option).

``--hard M`` (include/hgin.h A18) times the given-negative path instead, per shape in one run with the paths
alternating: the fused step with k uniform + M given negatives (random in-range destinations) against the fused step
with k + M uniform negatives (the same pair count, through the entry points that existed before A18); the same pair
with the M negatives mined by ``hard_negatives`` from the (random) embeddings; each step's destination side alone
(forward + the sort of the step's negatives + ``k_link_bwd_dst``: only z_dst asks for a gradient); and the mining call
alone.  Mining sweeps every destination for every distinct source, so the mined pair uses positives whose sources come
from the first ``--mine-sources`` source rows (the random-given pair keeps the shape's own positives).

``--graphs G`` (include/hgin.h A19; default 1: everything above, unchanged) cuts every shape into G equal graphs with
the positives sorted by graph and times the fused step with ``segments=`` against the same step without it, on the
same tensors, alternating in one run.

``--filter`` (include/hgin.h A20; composes with ``--graphs``) times the fused forward + backward of the loss with
``known`` = the positives (every draw taken from its source's non-neighbours) against the same call without it, on the
same tensors, alternating in one run; with ``--graphs G`` both calls carry ``segments=``.

    python tools/bench_linkpred.py --out profiles/linkpred/linkpred_bench.json
    python tools/bench_linkpred.py --k 1 --hard 4 --out profiles/linkpred/linkhard_bench.json
    python tools/bench_linkpred.py --objective all --out profiles/linkpred/linkobj_bench.json
    python tools/bench_linkpred.py --graphs 8      # profiles/linkseg/linkrank_seg_bench.json, "loss_step"
    python tools/bench_linkpred.py --filter [--graphs 8]      # profiles/linkfilt/linkfilt_bench.json
    python tools/bench_linkpred.py --configs cfg1 --scale 0.1 --k 1      # a tiny run
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "gnn-link-prediction_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

HBM_PEAK = 8.0e12          # bytes / s
OBJECTIVES = ["bce", "softmax", "bpr", "selfadv"]
DECODER_HBM_FRACTION = 0.73   # the existing dot-product decoder's recorded fraction


def fwd_algorithmic_bytes(E: int, k: int, F: int) -> int:
    """Source rows once, destination rows once per pair, coefficient and negative-pair writes, index reads."""
    rows = E * F * 4 + (1 + k) * E * F * 4
    writes = (1 + k) * E * 4 + 2 * E * k * 8
    index_reads = 2 * E * 8
    return rows + writes + index_reads


def rank_algorithmic_bytes(E: int, k: int, F: int) -> int:
    return E * F * 4 + (1 + k) * E * F * 4 + 2 * E * 8 + 2 * E * 4


def objectives_of(arg: str):
    """The objectives one --objective value asks for, in the order of the C ABI's codes."""
    if arg == "all":
        return list(OBJECTIVES)
    if arg not in OBJECTIVES:
        raise SystemExit(f"--objective must be one of {', '.join(OBJECTIVES)} or all, got {arg!r}")
    return [arg]


def plan(configs, ks, scale: float):
    from hgin.data import CONFIGS, scaled_config
    shapes = []
    for name in configs:
        cfg = CONFIGS[name]
        if scale != 1.0:
            cfg = scaled_config(cfg, scale)
        for k in ks:
            E, F = cfg.e_pl, cfg.hidden
            if E * k >= 2**31:
                raise SystemExit(f"{name}: E * k = {E * k} does not fit the kernels' 2^31 limit")
            shapes.append({"config": name, "scale": scale, "n_src": cfg.n_path, "n_dst": cfg.n_link, "E": E, "F": F,
                           "k": k, "fwd_algorithmic_bytes": fwd_algorithmic_bytes(E, k, F),
                           "rank_algorithmic_bytes": rank_algorithmic_bytes(E, k, F)})
    return shapes


def _stats(ms):
    med = statistics.median(ms)
    return {"median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "spread": (max(ms) - min(ms)) / med,
            "repeats_ms": ms}


def _timed(torch, fn, inner, first_step):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(inner):
        fn(first_step + i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def _inner_for(torch, fn, target_ms):
    fn(0)
    torch.cuda.synchronize()
    t = _timed(torch, fn, 1, 1)
    return max(1, int(math.ceil(target_ms / max(t, 1e-3))))


def run_shape(torch, shape, repeats, warmup, target_ms, seed=1234, objectives=("bce",)):
    from hgin.linkpred import link_loss, link_ranks, sampled_link_loss
    dev = "cuda"
    n_src, n_dst, E, F, k = (shape[x] for x in ("n_src", "n_dst", "E", "F", "k"))
    g = torch.Generator(device=dev).manual_seed(seed)
    pos = torch.stack([torch.randint(0, n_src, (E,), generator=g, device=dev),
                       torch.randint(0, n_dst, (E,), generator=g, device=dev)])
    z_src = (torch.randn(n_src, F, generator=g, device=dev) * 0.1).requires_grad_(True)
    z_dst = (torch.randn(n_dst, F, generator=g, device=dev) * 0.1).requires_grad_(True)

    def step_of(loss_fn, objective):
        # bce goes through the call without the argument, as every caller before the objectives existed
        kw = {} if objective == "bce" else {"objective": objective}

        def fn(step):
            z_src.grad = z_dst.grad = None
            loss_fn(z_src, z_dst, pos, k, seed, step * E * k, **kw).backward()
        return fn

    def fwd_only(step):
        with torch.no_grad():
            sampled_link_loss(z_src, z_dst, pos, k, seed, step * E * k)

    def rank_only(step):
        link_ranks(z_src, z_dst, pos, k, seed, step * E * k)

    fused = {o: step_of(sampled_link_loss, o) for o in objectives}
    base = {o: step_of(link_loss, o) for o in objectives}
    out = dict(shape)
    base_ok = True
    try:
        for s in range(warmup):
            for o in objectives:
                fused[o](s)
                base[o](s)
        torch.cuda.synchronize()
    except torch.OutOfMemoryError:
        base_ok = False
        z_src.grad = z_dst.grad = None
        torch.cuda.empty_cache()
        for s in range(warmup):
            for o in objectives:
                fused[o](s)
        torch.cuda.synchronize()
    inner_f = {o: _inner_for(torch, fused[o], target_ms) for o in objectives}
    inner_b = {o: _inner_for(torch, base[o], target_ms) if base_ok else 0 for o in objectives}
    t_f, t_b, step = {o: [] for o in objectives}, {o: [] for o in objectives}, warmup
    for _ in range(repeats):      # every path of every objective alternates
        for o in objectives:
            t_f[o].append(_timed(torch, fused[o], inner_f[o], step))
            if base_ok:
                t_b[o].append(_timed(torch, base[o], inner_b[o], step))
        step += max(max(inner_f.values()), max(inner_b.values()))

    def pair(o):
        res = {"fused": dict(_stats(t_f[o]), inner=inner_f[o])}
        if base_ok:
            res["link_loss"] = dict(_stats(t_b[o]), inner=inner_b[o])
            res["link_loss_over_fused"] = res["link_loss"]["median_ms"] / res["fused"]["median_ms"]
            res["fused_faster_beyond_spread"] = res["fused"]["max_ms"] < res["link_loss"]["min_ms"]
        else:
            res["link_loss"] = {"error": "out of memory"}
        return res

    if "bce" in objectives:
        out.update(pair("bce"))
    others = [o for o in objectives if o != "bce"]
    if others:
        out["objectives"] = {o: pair(o) for o in others}
        if "bce" in objectives:   # the same run, the same box: the epilogue's cost over the bce step
            for o in others:
                out["objectives"][o]["fused_over_fused_bce"] = (out["objectives"][o]["fused"]["median_ms"]
                                                               / out["fused"]["median_ms"])
    z_src.grad = z_dst.grad = None
    if "bce" in objectives:
        for name, fn, nbytes in (("fused_forward", fwd_only, shape["fwd_algorithmic_bytes"]),
                                 ("rank", rank_only, shape["rank_algorithmic_bytes"])):
            inner = _inner_for(torch, fn, target_ms)
            st = _stats([_timed(torch, fn, inner, warmup + r * inner) for r in range(repeats)])
            st.update(inner=inner, algorithmic_bytes=nbytes,
                      hbm_fraction=nbytes / (st["median_ms"] * 1e-3) / HBM_PEAK)
            out[name] = st
        out["decoder_hbm_fraction_recorded"] = DECODER_HBM_FRACTION
    del z_src, z_dst, pos
    torch.cuda.empty_cache()
    return out


def run_hard(torch, shape, M, repeats, warmup, target_ms, mine_sources, seed=1234):
    """The ``--hard M`` measurements of one shape (module docstring)."""
    from hgin.linkpred import hard_negatives, sampled_link_loss
    dev = "cuda"
    n_src, n_dst, E, F, k = (shape[x] for x in ("n_src", "n_dst", "E", "F", "k"))
    g = torch.Generator(device=dev).manual_seed(seed)
    pos = torch.stack([torch.randint(0, n_src, (E,), generator=g, device=dev),
                       torch.randint(0, n_dst, (E,), generator=g, device=dev)])
    q = min(n_src, mine_sources)
    pos_m = torch.stack([torch.randint(0, q, (E,), generator=g, device=dev), pos[1].clone()])
    z_src = torch.randn(n_src, F, generator=g, device=dev) * 0.1
    z_dst = torch.randn(n_dst, F, generator=g, device=dev) * 0.1
    given = torch.randint(0, n_dst, (E, M), generator=g, device=dev, dtype=torch.int32)

    def mine(step):
        return hard_negatives(z_src, z_dst, pos_m, M, seed=seed, offset=step * E * M)

    mined = mine(0)
    torch.cuda.synchronize()
    counts = torch.bincount(mined.reshape(-1).long(), minlength=n_dst)
    out = dict(shape, hard=M, mine_sources=q,
               mined_distinct_destinations=int((counts > 0).sum()), mined_max_pairs_per_destination=int(counts.max()),
               uniform_expected_pairs_per_destination=E * M / n_dst)

    def step_of(p, kk, neg_dst, src_grad):
        kw = {} if neg_dst is None else {"neg_dst": neg_dst}

        def fn(step):
            a, b = z_src.requires_grad_(src_grad), z_dst.requires_grad_(True)
            a.grad = b.grad = None
            sampled_link_loss(a, b, p, kk, seed, step * E * kk, **kw).backward()
        return fn

    paths = {"given_random": step_of(pos, k, given, True), "uniform": step_of(pos, k + M, None, True),
             "given_mined": step_of(pos_m, k, mined, True), "uniform_mined_pos": step_of(pos_m, k + M, None, True),
             "given_random_dst_only": step_of(pos, k, given, False),
             "uniform_dst_only": step_of(pos, k + M, None, False),
             "given_mined_dst_only": step_of(pos_m, k, mined, False),
             "uniform_mined_pos_dst_only": step_of(pos_m, k + M, None, False), "mining": mine}
    for s in range(warmup):
        for name, fn in paths.items():
            if name != "mining":
                fn(s)
    torch.cuda.synchronize()
    inner = {name: 1 if name == "mining" else _inner_for(torch, fn, target_ms) for name, fn in paths.items()}
    times, step = {name: [] for name in paths}, warmup
    for _ in range(repeats):      # every path alternates
        for name, fn in paths.items():
            times[name].append(_timed(torch, fn, inner[name], step))
        step += max(inner.values())
    for name in paths:
        out[name] = dict(_stats(times[name]), inner=inner[name])
    for a, b in (("given_random", "uniform"), ("given_mined", "uniform_mined_pos"),
                 ("given_random_dst_only", "uniform_dst_only"), ("given_mined_dst_only", "uniform_mined_pos_dst_only")):
        out[f"{a}_over_{b}"] = out[a]["median_ms"] / out[b]["median_ms"]
        out[f"{a}_within_spread_of_{b}"] = out[a]["min_ms"] <= out[b]["max_ms"] and out[b]["min_ms"] <= out[a]["max_ms"]
    z_src.grad = z_dst.grad = None
    del z_src, z_dst, pos, pos_m, given, mined
    torch.cuda.empty_cache()
    return out


def split_graphs(n_src: int, n_dst: int, E: int, graphs: int, seed: int, device="cpu"):
    """A shape cut into ``graphs`` equal graphs (the first n % graphs blocks one row longer), as a collated batch
    lays them out: (pos int64 [2, E], batch_src int64 [n_src], batch_dst int64 [n_dst]).  Graph e * graphs // E owns
    positive e, so the positives come sorted by graph; source and destination are uniform inside the graph's blocks."""
    import torch
    if not 1 <= graphs <= min(n_src, n_dst):
        raise SystemExit(f"--graphs must be in [1, min(n_src, n_dst)] = [1, {min(n_src, n_dst)}], got {graphs}")
    g = torch.Generator(device=device).manual_seed(seed)

    def blocks(n):
        sizes = torch.tensor([n // graphs + (i < n % graphs) for i in range(graphs)], dtype=torch.long, device=device)
        ptr = torch.zeros(graphs + 1, dtype=torch.long, device=device)
        ptr[1:] = torch.cumsum(sizes, 0)
        return sizes, ptr

    (ss, sp), (ds, dp) = blocks(n_src), blocks(n_dst)
    ge = (torch.arange(E, dtype=torch.long, device=device) * graphs) // max(E, 1)
    u = torch.rand(2, E, generator=g, device=device, dtype=torch.float64)
    src = sp[ge] + torch.minimum((u[0] * ss[ge]).long(), ss[ge] - 1)
    dst = dp[ge] + torch.minimum((u[1] * ds[ge]).long(), ds[ge] - 1)
    ids = torch.arange(graphs, dtype=torch.long, device=device)
    return torch.stack([src, dst]), torch.repeat_interleave(ids, ss), torch.repeat_interleave(ids, ds)


def run_graphs(torch, shape, graphs, repeats, warmup, target_ms, seed=1234):
    """The ``--graphs G`` measurements of one shape: the shape cut into G equal graphs, positives sorted by graph, the
    fused forward + backward step with ``segments=`` against the same step without it on the same tensors, the paths
    alternating in one run."""
    from hgin.linkpred import LinkSegments, sampled_link_loss
    dev = "cuda"
    n_src, n_dst, E, F, k = (shape[x] for x in ("n_src", "n_dst", "E", "F", "k"))
    pos, batch_src, batch_dst = split_graphs(n_src, n_dst, E, graphs, seed, dev)
    seg = LinkSegments(batch_src, batch_dst, graphs)
    g = torch.Generator(device=dev).manual_seed(seed)
    z_src = (torch.randn(n_src, F, generator=g, device=dev) * 0.1).requires_grad_(True)
    z_dst = (torch.randn(n_dst, F, generator=g, device=dev) * 0.1).requires_grad_(True)

    def step_of(kw):
        def fn(step):
            z_src.grad = z_dst.grad = None
            sampled_link_loss(z_src, z_dst, pos, k, seed, step * E * k, **kw).backward()
        return fn

    paths = {"unsegmented": step_of({}), "segmented": step_of({"segments": seg})}
    for s in range(warmup):
        for fn in paths.values():
            fn(s)
    torch.cuda.synchronize()
    inner = {name: _inner_for(torch, fn, target_ms) for name, fn in paths.items()}
    times, step = {name: [] for name in paths}, warmup
    for _ in range(repeats):      # the paths alternate
        for name, fn in paths.items():
            times[name].append(_timed(torch, fn, inner[name], step))
        step += max(inner.values())
    out = dict(shape, graphs=graphs, positives="sorted by graph")
    for name in paths:
        out[name] = dict(_stats(times[name]), inner=inner[name])
    a, b = out["segmented"], out["unsegmented"]
    out["segmented_over_unsegmented"] = a["median_ms"] / b["median_ms"]
    out["segmented_within_spread_of_unsegmented"] = a["min_ms"] <= b["max_ms"] and b["min_ms"] <= a["max_ms"]
    z_src.grad = z_dst.grad = None
    del z_src, z_dst, pos
    torch.cuda.empty_cache()
    return out


def run_filter(torch, shape, graphs, repeats, warmup, target_ms, seed=1234):
    """The ``--filter`` measurements of one shape: the fused forward + backward step with ``known`` = the positives
    against the same step without it, on the same tensors (cut into ``graphs`` equal graphs and carrying ``segments=``
    when graphs > 1), the paths alternating in one run.  Also recorded: the known rows' lengths and the share of the
    unfiltered step's draws that are known edges of their source."""
    from hgin.linkpred import LinkSegments, _known_csr, sampled_link_loss
    dev = "cuda"
    n_src, n_dst, E, F, k = (shape[x] for x in ("n_src", "n_dst", "E", "F", "k"))
    g = torch.Generator(device=dev).manual_seed(seed)
    kw = {}
    if graphs > 1:
        pos, batch_src, batch_dst = split_graphs(n_src, n_dst, E, graphs, seed, dev)
        kw["segments"] = LinkSegments(batch_src, batch_dst, graphs)
    else:
        pos = torch.stack([torch.randint(0, n_src, (E,), generator=g, device=dev),
                           torch.randint(0, n_dst, (E,), generator=g, device=dev)])
    z_src = (torch.randn(n_src, F, generator=g, device=dev) * 0.1).requires_grad_(True)
    z_dst = (torch.randn(n_dst, F, generator=g, device=dev) * 0.1).requires_grad_(True)

    def step_of(extra):
        def fn(step):
            z_src.grad = z_dst.grad = None
            sampled_link_loss(z_src, z_dst, pos, k, seed, step * E * k, **kw, **extra).backward()
        return fn

    paths = {"unfiltered": step_of({}), "filtered": step_of({"known": pos})}
    for s in range(warmup):
        for fn in paths.values():
            fn(s)
    torch.cuda.synchronize()
    inner = {name: _inner_for(torch, fn, target_ms) for name, fn in paths.items()}
    times, step = {name: [] for name in paths}, warmup
    for _ in range(repeats):      # the paths alternate
        for name, fn in paths.items():
            times[name].append(_timed(torch, fn, inner[name], step))
        step += max(inner.values())
    rowptr, _ = _known_csr(pos, n_src, n_dst)
    deg = (rowptr[1:] - rowptr[:-1])[pos[0]].double()
    plain = sampled_link_loss(z_src, z_dst, pos, k, seed, 0, **kw)
    filt = sampled_link_loss(z_src, z_dst, pos, k, seed, 0, known=pos, **kw)
    edge_keys = torch.unique(pos[0] * n_dst + pos[1])

    def known_share(loss):
        neg = loss.grad_fn.saved_tensors[1]
        return float(torch.isin(neg[0] * n_dst + neg[1], edge_keys).double().mean())

    out = dict(shape, graphs=graphs, known="the positives", known_row_mean=float(deg.mean()),
               known_row_max=int(deg.max()), unfiltered_draws_known_share=known_share(plain),
               filtered_draws_known_share=known_share(filt))
    for name in paths:
        out[name] = dict(_stats(times[name]), inner=inner[name])
    a, b = out["filtered"], out["unfiltered"]
    out["filtered_over_unfiltered"] = a["median_ms"] / b["median_ms"]
    out["filtered_within_spread_of_unfiltered"] = a["min_ms"] <= b["max_ms"] and b["min_ms"] <= a["max_ms"]
    z_src.grad = z_dst.grad = None
    del z_src, z_dst, pos
    torch.cuda.empty_cache()
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--configs", default="cfg2,cfg3")
    ap.add_argument("--graphs", type=int, default=1,
                    help="cut every shape into G equal graphs, positives sorted by graph, and time the fused step with "
                         "segments= against the same step without (include/hgin.h A19); 1: today's measurements")
    ap.add_argument("--filter", action="store_true",
                    help="time the fused step with known = the positives against the same step without it "
                         "(include/hgin.h A20); composes with --graphs")
    ap.add_argument("--k", default="1,4")
    ap.add_argument("--scale", type=float, default=1.0, help="multiply every node / edge count (tiny runs)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--target-ms", type=float, default=30.0, help="device time of one timed repeat, at least")
    ap.add_argument("--objective", default="bce", help="bce, softmax, bpr, selfadv or all (include/hgin.h A17)")
    ap.add_argument("--hard", type=int, default=None,
                    help="time k uniform + M given / mined negatives against k + M uniform ones (include/hgin.h A18)")
    ap.add_argument("--mine-sources", type=int, default=65536, help="--hard: distinct sources of the mined positives")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.repeats < 5:
        ap.error("--repeats must be at least 5")
    if args.hard is not None and not 1 <= args.hard <= 128:
        ap.error("--hard must be in [1, 128]")
    if args.graphs < 1:
        ap.error("--graphs must be at least 1")
    if args.filter and (args.hard is not None or args.objective != "bce"):
        ap.error("--filter composes with --graphs only")
    objectives = objectives_of(args.objective)
    shapes = plan(args.configs.split(","), [int(v) for v in args.k.split(",")], args.scale)
    for s in shapes:
        print("plan:", json.dumps(s), file=sys.stderr)

    import torch
    if not torch.cuda.is_available():
        print("bench_linkpred: no HIP device is visible; the link-prediction path has no CPU fallback", file=sys.stderr)
        return 2
    from hgin import _lib
    _lib.lib()
    if args.filter:
        results = [run_filter(torch, s, args.graphs, args.repeats, args.warmup, args.target_ms) for s in shapes]
        doc = {"tool": "tools/bench_linkpred.py", "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
               "warmup": args.warmup, "filter": True, "graphs": args.graphs, "shapes": results}
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(doc, indent=1) + "\n")
        print(json.dumps(doc))
        return 0
    if args.graphs > 1:
        results = [run_graphs(torch, s, args.graphs, args.repeats, args.warmup, args.target_ms) for s in shapes]
        doc = {"tool": "tools/bench_linkpred.py", "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
               "warmup": args.warmup, "graphs": args.graphs, "shapes": results}
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(doc, indent=1) + "\n")
        print(json.dumps(doc))
        return 0
    if args.hard is not None:
        results = [run_hard(torch, s, args.hard, args.repeats, args.warmup, args.target_ms, args.mine_sources)
                   for s in shapes]
        doc = {"tool": "tools/bench_linkpred.py", "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
               "warmup": args.warmup, "hard": args.hard, "shapes": results}
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(doc, indent=1) + "\n")
        print(json.dumps(doc))
        return 0
    results = [run_shape(torch, s, args.repeats, args.warmup, args.target_ms, objectives=objectives) for s in shapes]
    pairs = [r for r in results if "link_loss" in r] + [p for r in results for p in r.get("objectives", {}).values()]
    both = [p for p in pairs if "error" not in p["link_loss"]]
    doc = {"tool": "tools/bench_linkpred.py", "device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK,
           "repeats": args.repeats, "warmup": args.warmup, "objectives": objectives, "shapes": results,
           "fused_faster_at_every_shape_both_ran": all(p["fused_faster_beyond_spread"] for p in both)}
    text = json.dumps(doc)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    print(text)
    return 0 if doc["fused_faster_at_every_shape_both_ran"] else 1


if __name__ == "__main__":
    sys.exit(main())
