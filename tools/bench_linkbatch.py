#!/usr/bin/env python3
"""Time neighbour-sampled link-prediction mini-batches (include/hgin.h A22) on CONFIGS[cfg], on one GPU in one process.

Two comparisons per config, B positives of ('path', 'uses', 'link') and k uniform negatives each per batch:
  (a) the batch itself: ``hgin.link_neighbor_batch`` (seed check, per hop the HIP offsets / picks / candidate test /
      relabel and torch's ``unique``, then the ``x`` / ``y`` / ``batch`` row gathers) against a plain torch formulation
      of the same rule's shape on the same CSR tensors: every CSR position of a frontier row gets a random key, a sort by
      (row, key) keeps the first f of each row, ``unique`` + ``searchsorted`` relabel, the same row gathers.  The torch
      path's local rows are in id order, not hop-major, and its picks are not reproducible from (seed, batch number); it
      is here as the cost a user pays today.  Host reads per batch are stated in the output (``host_reads``).
  (b) the optimizer step: ``hgin.link_minibatch_step`` on the sampled subgraph against ``hgin.link_train_step`` on the
      whole graph with the same B positives as ``pos=`` (the encoder then still convolves every edge), same model, same
      predictor, same optimizer.  Reported with the subgraph's rows per type, edges per relation and edges convolved.
The paths alternate inside one run, every shape is warmed up, every timed repeat is ``inner`` calls between two HIP
events; per path: median / min / max over the repeats, the ratio of the medians and whether the new path is faster (or
slower) than the other by more than the spread (its slowest repeat under the other's fastest).  No ratio is promised:
the exit status is 0 when the run completed.  Not measured: HetroGAT subgraphs, hub-heavy (Zipf) graphs, training to
convergence.  There is no CPU fallback: without a HIP device the tool prints the plan and fails.

    python tools/bench_linkbatch.py --out profiles/linkbatch/linkbatch_bench.json
    python tools/bench_linkbatch.py --configs cfg1 --batch 64            # a tiny run

``--exclude`` times the batch without its own target edges (include/hgin.h A25) at the same shapes instead, all paths
alternating in one run: ``hgin.link_neighbor_batch_excl`` against ``hgin.link_neighbor_batch`` on the same tensors,
both against the only way there was before (``torch.isin`` masks the batch's pairs out of both relations'
``edge_index``, a fresh ``NeighborSampler`` builds its CSRs on the result), and ``hgin.link_minibatch_step`` with and
without ``LinkPredictor(exclude_targets=True)``:

    python tools/bench_linkbatch.py --exclude --out profiles/linkexcl/linkexcl_bench.json
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

FANOUTS = {2: [10, 5], 3: [10, 5, 5]}      # by model depth: cfg2 has two layers, cfg3 three


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def plan(configs, batch: int, k: int):
    from hgin.data import CONFIGS
    shapes = []
    for name in configs:
        cfg = CONFIGS[name]
        shapes.append(dict(config=cfg.name, B=batch, k=k, fanouts=FANOUTS.get(cfg.layers, [10] + [5] * (cfg.layers - 1)),
                           nodes=cfg.nodes, conv_edges=cfg.conv_edges, hidden=cfg.hidden, layers=cfg.layers))
    return shapes


def _torch_batch(torch, graph, csr64, relations, fanouts, seeds, gen):
    """The batch a user writes in torch today (see the module docstring).  csr64 = {relation: (rowptr, col, perm) int64}."""
    types = list(graph.x.keys())
    dev = next(iter(seeds.values())).device
    empty = torch.empty(0, dtype=torch.int64, device=dev)
    n_id = {t: (torch.unique(seeds[t]) if t in seeds else empty) for t in types}
    frontier = dict(n_id)
    picked = {r: [] for r in relations}
    for f in fanouts:
        reached = {t: [] for t in types}
        for r in relations:
            fr = frontier[r[2]]
            if fr.numel() == 0:
                continue
            rowptr, col, perm = csr64[r]
            start = rowptr[fr]
            deg = rowptr[fr + 1] - start
            first = torch.cumsum(deg, 0) - deg
            row = torch.repeat_interleave(torch.arange(fr.numel(), device=dev), deg)
            slot = torch.arange(row.numel(), device=dev)
            key = (row << 32) | torch.randint(0, 2**32, (row.numel(),), device=dev, generator=gen)
            order = torch.argsort(key)                       # by row, then by the random key
            keep = order[(slot - first[row]) < f]            # the first f of every row (row[order] == row)
            keep = torch.sort(keep).values                   # back to ascending CSR position
            at = start[row[keep]] + (keep - first[row[keep]])
            src = col[at]
            picked[r].append((src, fr[row[keep]], perm[at]))
            reached[r[0]].append(src)
        frontier = {}
        for t in types:
            if reached[t]:
                both = torch.unique(torch.cat([n_id[t]] + reached[t]))
                old = n_id[t]
                if old.numel():
                    at = torch.searchsorted(old, both).clamp(max=old.numel() - 1)
                    frontier[t] = both[old[at] != both]
                else:
                    frontier[t] = both
                n_id[t] = both
            else:
                frontier[t] = empty
    edge_index, e_id = {}, {}
    for r in relations:
        if picked[r]:
            src, dst, eid = (torch.cat(c) for c in zip(*picked[r]))
            edge_index[r] = torch.stack([torch.searchsorted(n_id[r[0]], src), torch.searchsorted(n_id[r[2]], dst)])
            e_id[r] = eid
        else:
            edge_index[r], e_id[r] = torch.empty((2, 0), dtype=torch.int64, device=dev), empty
    x = {t: graph.x[t][n_id[t]] for t in types}
    y = graph.y[n_id["path"]]
    batch = {t: graph.batch[t][n_id[t]] for t in types}
    return x, edge_index, y, batch, n_id, e_id


def run_shape(torch, shape, repeats, warmup, target_ms, seed=1234):
    lp = _tool("bench_linkpred")
    import hgin
    from hgin import ops
    from hgin.data import CONFIGS, CONV_RELATIONS, REL_PL, synthetic_graph
    from hgin.linkpred import sample_negative_dst
    dev = "cuda"
    cfg = CONFIGS[shape["config"]]
    B, k, fanouts = shape["B"], shape["k"], shape["fanouts"]
    graph = synthetic_graph(cfg, seed=0, device=dev)
    gen = torch.Generator(device=dev).manual_seed(seed)
    all_pos = graph.edge_index[REL_PL]
    n_dst = cfg.n_link
    sampler = hgin.NeighborSampler(graph, fanouts=fanouts, relations=CONV_RELATIONS, seed=seed)
    csr64 = {}
    for r in CONV_RELATIONS:
        c = ops.relation_graph(graph.edge_index[r], graph.x[r[0]].size(0), graph.x[r[2]].size(0)).csr
        csr64[r] = (c.rowptr.long(), c.col.long(), c.perm.long())

    def batch_of(step):
        idx = torch.randint(0, all_pos.size(1), (B,), device=dev, generator=gen)
        pos = all_pos[:, idx].contiguous()
        neg = sample_negative_dst(B * k, n_dst, seed, step * B * k, dev).view(B, k)
        return pos, neg

    def fused(step):
        pos, neg = batch_of(step)
        return hgin.link_neighbor_batch(sampler, REL_PL, pos, neg, offset=step)

    def plain(step):
        pos, neg = batch_of(step)
        seeds = {"path": pos[0], "link": torch.cat([pos[1], neg.reshape(-1).long()])}
        return _torch_batch(torch, graph, csr64, CONV_RELATIONS, fanouts, seeds, gen)

    out = dict(shape)
    # ---- (a) the batch ------------------------------------------------------------------------------
    paths = {"hip": fused, "torch": plain}
    for _ in range(warmup):
        for fn in paths.values():
            fn(0)
    torch.cuda.synchronize()
    sub = fused(1).sub
    sizes = {"rows": {t: int(v.numel()) for t, v in sub.n_id.items()},
             "edges": {"__".join(r): int(e.size(1)) for r, e in sub.graph.edge_index.items()}}
    sizes["edges_convolved"] = sum(sizes["edges"].values())
    t_rows = {t: int(v.numel()) for t, v in plain(1)[4].items()}
    case = {"subgraph": sizes, "torch_rows": t_rows,
            "host_reads": {"hip": f"1 (seed range) + {len(fanouts)} (a hop's edge counts) + the size read inside "
                                  f"torch.unique: {len(sub.n_id)} for the seeds, up to {len(sub.n_id)} per hop",
                           "torch": "per hop and relation the size reads of repeat_interleave and of the boolean "
                                    "selection, per hop and type those of unique and of the frontier mask"}}
    inner = {name: lp._inner_for(torch, fn, target_ms) for name, fn in paths.items()}
    times = {name: [] for name in paths}
    for _ in range(repeats):          # the paths alternate
        for name, fn in paths.items():
            times[name].append(lp._timed(torch, fn, inner[name], 1))
    for name in paths:
        case[name] = dict(lp._stats(times[name]), inner=inner[name])
        print(f"{cfg.name} batch: {name}: median {case[name]['median_ms']:.3f} ms", file=sys.stderr, flush=True)
    case["torch_over_hip"] = case["torch"]["median_ms"] / case["hip"]["median_ms"]
    case["hip_faster_beyond_spread"] = case["hip"]["max_ms"] < case["torch"]["min_ms"]
    case["hip_slower_beyond_spread"] = case["hip"]["min_ms"] > case["torch"]["max_ms"]
    out["batch"] = case
    del sub
    # ---- (b) the optimizer step ---------------------------------------------------------------------
    torch.manual_seed(1997)
    model = hgin.HetroGIN(**cfg.model_kwargs({"link": cfg.f_link, "path": cfg.f_path, "node": cfg.f_node})).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    pred = hgin.LinkPredictor(model, REL_PL, k=k, seed=seed)

    def mini(step):
        return hgin.link_minibatch_step(model, opt, sampler, pred, batch_of(step)[0], step)

    def full(step):
        return hgin.link_train_step(model, opt, graph, pred, step, pos=batch_of(step)[0])

    paths = {"minibatch": mini, "full_graph": full}
    for _ in range(warmup):
        for fn in paths.values():
            fn(0)
    torch.cuda.synchronize()
    inner = {name: lp._inner_for(torch, fn, target_ms) for name, fn in paths.items()}
    times = {name: [] for name in paths}
    for _ in range(repeats):
        for name, fn in paths.items():
            times[name].append(lp._timed(torch, fn, inner[name], 1))
    case = {"edges_convolved": {"minibatch": sizes["edges_convolved"], "full_graph": cfg.conv_edges}}
    for name in paths:
        case[name] = dict(lp._stats(times[name]), inner=inner[name])
        print(f"{cfg.name} step: {name}: median {case[name]['median_ms']:.3f} ms", file=sys.stderr, flush=True)
    case["full_over_minibatch"] = case["full_graph"]["median_ms"] / case["minibatch"]["median_ms"]
    case["minibatch_faster_beyond_spread"] = case["minibatch"]["max_ms"] < case["full_graph"]["min_ms"]
    case["minibatch_slower_beyond_spread"] = case["minibatch"]["min_ms"] > case["full_graph"]["max_ms"]
    out["step"] = case
    del model, opt, pred, sampler, graph, csr64
    torch.cuda.empty_cache()
    return out


def _alternate(torch, lp, paths, repeats, warmup, target_ms, label):
    """{name: stats} of the callables ``paths``, alternating inside every repeat."""
    for _ in range(warmup):
        for fn in paths.values():
            fn(0)
    torch.cuda.synchronize()
    inner = {name: lp._inner_for(torch, fn, target_ms) for name, fn in paths.items()}
    times = {name: [] for name in paths}
    for _ in range(repeats):
        for name, fn in paths.items():
            times[name].append(lp._timed(torch, fn, inner[name], 1))
    out = {}
    for name in paths:
        out[name] = dict(lp._stats(times[name]), inner=inner[name])
        print(f"{label}: {name}: median {out[name]['median_ms']:.3f} ms [{out[name]['min_ms']:.3f} - "
              f"{out[name]['max_ms']:.3f}]", file=sys.stderr, flush=True)
    return out


def _beyond(a, b):
    """a against b: 'faster' / 'slower' when the whole spread of a lies on one side of b's, else 'inside'."""
    if a["max_ms"] < b["min_ms"]:
        return "faster"
    return "slower" if a["min_ms"] > b["max_ms"] else "inside"


def run_exclude(torch, shape, repeats, warmup, target_ms, seed=1234):
    """--exclude: what keeping a batch's own target edges out of its neighbourhood costs (include/hgin.h A25).  The
    positives are edges of the graph, so every batch has B pairs to exclude in path -> link and B in link -> path."""
    lp = _tool("bench_linkpred")
    import hgin
    from hgin.data import CONFIGS, CONV_RELATIONS, REL_LP, REL_PL, HeteroGraph, synthetic_graph
    from hgin.linkpred import sample_negative_dst
    dev = "cuda"
    cfg = CONFIGS[shape["config"]]
    B, k, fanouts = shape["B"], shape["k"], shape["fanouts"]
    graph = synthetic_graph(cfg, seed=0, device=dev)
    gen = torch.Generator(device=dev).manual_seed(seed)
    all_pos = graph.edge_index[REL_PL]
    n_dst = cfg.n_link
    sampler = hgin.NeighborSampler(graph, fanouts=fanouts, relations=CONV_RELATIONS, seed=seed)

    def batch_of(step):
        idx = torch.randint(0, all_pos.size(1), (B,), device=dev, generator=gen)
        pos = all_pos[:, idx].contiguous()
        neg = sample_negative_dst(B * k, n_dst, seed, step * B * k, dev).view(B, k)
        return pos, neg

    def plain(step):
        pos, neg = batch_of(step)
        return hgin.link_neighbor_batch(sampler, REL_PL, pos, neg, offset=step)

    def excl(step):
        pos, neg = batch_of(step)
        return hgin.link_neighbor_batch_excl(sampler, REL_PL, pos, neg, offset=step)

    def rebuild(step):
        # the only way before A25: mask the batch's pairs out of both relations and build a sampler on what is left
        pos, neg = batch_of(step)
        keys = pos[0] * n_dst + pos[1]
        pl, lp_ = graph.edge_index[REL_PL], graph.edge_index[REL_LP]
        ei = dict(graph.edge_index)
        ei[REL_PL] = pl[:, ~torch.isin(pl[0] * n_dst + pl[1], keys)]
        ei[REL_LP] = lp_[:, ~torch.isin(lp_[1] * n_dst + lp_[0], keys)]
        fresh = hgin.NeighborSampler(HeteroGraph(graph.x, ei, graph.y, graph.batch), fanouts=fanouts,
                                     relations=CONV_RELATIONS, seed=seed)
        return hgin.link_neighbor_batch(fresh, REL_PL, pos, neg, offset=step)

    out = dict(shape)
    # the three batches of one step agree on what they are: the excluded one holds no target edge, the rebuilt one is
    # the same subgraph (same rows, same edges; its e_id counts positions of the masked lists)
    pos, neg = batch_of(1)
    a = hgin.link_neighbor_batch(sampler, REL_PL, pos, neg, offset=1).sub
    b = hgin.link_neighbor_batch_excl(sampler, REL_PL, pos, neg, offset=1).sub
    e = b.graph.edge_index[REL_PL]
    back = b.n_id["path"][e[0]] * n_dst + b.n_id["link"][e[1]]
    ea = a.graph.edge_index[REL_PL]
    held = a.n_id["path"][ea[0]] * n_dst + a.n_id["link"][ea[1]]
    keys = pos[0] * n_dst + pos[1]
    out["check"] = {"target_edges_in_plain_batch": int(torch.isin(held, keys).sum()),
                    "target_edges_in_excluded_batch": int(torch.isin(back, keys).sum()),
                    "edges_plain": int(sum(v.size(1) for v in a.graph.edge_index.values())),
                    "edges_excluded": int(sum(v.size(1) for v in b.graph.edge_index.values()))}
    del a, b
    case = _alternate(torch, lp, {"plain": plain, "excl": excl, "rebuild": rebuild}, repeats, warmup, target_ms,
                      f"{cfg.name} batch")
    case["excl_over_plain"] = case["excl"]["median_ms"] / case["plain"]["median_ms"]
    case["rebuild_over_excl"] = case["rebuild"]["median_ms"] / case["excl"]["median_ms"]
    case["excl_vs_plain"] = _beyond(case["excl"], case["plain"])
    case["excl_vs_rebuild"] = _beyond(case["excl"], case["rebuild"])
    out["batch"] = case

    torch.manual_seed(1997)
    model = hgin.HetroGIN(**cfg.model_kwargs({"link": cfg.f_link, "path": cfg.f_path, "node": cfg.f_node})).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    pred = hgin.LinkPredictor(model, REL_PL, k=k, seed=seed)
    pred_x = hgin.LinkPredictor(model, REL_PL, k=k, seed=seed, exclude_targets=True)

    def step_plain(step):
        return hgin.link_minibatch_step(model, opt, sampler, pred, batch_of(step)[0], step)

    def step_excl(step):
        return hgin.link_minibatch_step(model, opt, sampler, pred_x, batch_of(step)[0], step)

    case = _alternate(torch, lp, {"plain": step_plain, "exclude_targets": step_excl}, repeats, warmup, target_ms,
                      f"{cfg.name} step")
    case["excl_over_plain"] = case["exclude_targets"]["median_ms"] / case["plain"]["median_ms"]
    case["excl_vs_plain"] = _beyond(case["exclude_targets"], case["plain"])
    out["step"] = case
    del model, opt, pred, pred_x, sampler, graph
    torch.cuda.empty_cache()
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--configs", default="cfg2,cfg3")
    ap.add_argument("--batch", type=int, default=4096, help="positives per batch")
    ap.add_argument("--k", type=int, default=4, help="uniform negatives per positive")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--target-ms", type=float, default=200.0, help="device time of one timed repeat, at least")
    ap.add_argument("--out", default=None)
    ap.add_argument("--exclude", action="store_true",
                    help="time link_neighbor_batch_excl / exclude_targets (A25) against the plain batch and against "
                         "masking the pairs out of the graph and rebuilding the sampler")
    args = ap.parse_args(argv)
    if args.repeats < 5:
        ap.error("--repeats must be at least 5")
    if args.warmup < 1:
        ap.error("--warmup must be at least 1")
    shapes = plan(args.configs.split(","), args.batch, args.k)
    for s in shapes:
        print("plan:", json.dumps(s), file=sys.stderr)

    import torch
    if not torch.cuda.is_available():
        print("bench_linkbatch: no HIP device is visible; the sampling kernels have no CPU fallback", file=sys.stderr)
        return 2
    from hgin import _lib
    _lib.lib()
    run = run_exclude if args.exclude else run_shape
    results = [run(torch, s, args.repeats, args.warmup, args.target_ms) for s in shapes]
    doc = {"tool": "tools/bench_linkbatch.py" + (" --exclude" if args.exclude else ""),
           "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
           "warmup": args.warmup, "not_measured": ["HetroGAT subgraphs", "hub-heavy (Zipf) graphs",
                                                   "training to convergence"], "shapes": results}
    if args.exclude:
        doc["not_measured"] += ["batches whose pairs are not edges of the graph", "batch_full_loss",
                                "the accuracy effect of the exclusion"]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))
    return 0


if __name__ == "__main__":
    sys.exit(main())
