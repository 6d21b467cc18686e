"""Times the sampled counts (RAND-ESU) on one MI355X against their host twin and against the exact device census.

Shapes: Syn_1827-shaped (1827 graphs), COX2-shaped x64 (29 888 molecules) and a dense set on which the exact census
takes seconds: --dense_graphs ER graphs of --dense_nodes nodes and --dense_edges edges from ``generators.generate``
(seed 0, host twin).  Schedules: the uniform one and leaf-only (1, 1, 1, f) at f = 1, 0.1, 0.01, 0.001; the 30 classes of
2..5 nodes, --replicas replicas, graph-level tallies.  Per shape and schedule the device's tallies are first compared
with the twin's bit for bit; then min / median / max of --repeat runs of the device call (HIP events around
``sampled_tallies_device``, uploads and the per-graph reduction included), of the twin on --threads threads (host
clock) and, per shape, of the exact device census (``canonical_counts_device``).  A call that takes longer than
--once_above seconds is timed once.  Where the twin would visit more than --twin_budget kept subsets it runs -- and is
compared -- on the first graphs of the set only (``twin_graphs``), and the ratio to the device scales its time by the
kept subsets of the whole set over those of the slice (``kept_subsets_set_over_twin_graphs``).  Next to each time: the
observed relative error of the per-graph totals of the 5-node classes (mean over the graphs that hold any) and the mean
reported stderr / estimate of the same totals.  One JSON line per measurement.

    python tools/bench_sampled_counts.py [--shapes syn cox2 dense] [--repeat 5] [--threads 16]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FRACTIONS = (1.0, 0.1, 0.01, 0.001)


def summary(xs):
    xs = sorted(xs)
    return {"min_s": xs[0], "median_s": xs[len(xs) // 2], "max_s": xs[-1], "runs": len(xs)}


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--shapes", nargs="+", default=["syn", "cox2", "dense"], choices=("syn", "cox2", "dense"))
    p.add_argument("--repeat", type=int, default=5)
    p.add_argument("--threads", type=int, default=16)
    p.add_argument("--replicas", type=int, default=16)
    p.add_argument("--once_above", type=float, default=5.0)
    p.add_argument("--twin_budget", type=float, default=2e10)
    p.add_argument("--dense_graphs", type=int, default=64)
    p.add_argument("--dense_nodes", type=int, default=200)
    p.add_argument("--dense_edges", type=int, default=4000)
    args = p.parse_args(argv)
    import torch
    from desco_amd import generators, sampling, synthetic
    from desco_amd import groundtruth as gt
    assert torch.cuda.is_available(), "bench_sampled_counts needs an MI355X"
    R, seed = args.replicas, 0
    classes = [(n, list(e)) for k in (2, 3, 4, 5) for n, e in gt.census_classes(k)]
    sizes = np.array([n for n, _ in classes])
    five = np.flatnonzero(sizes == 5)

    def shape(name):
        if name == "syn":
            return "syn_1827_shaped", synthetic.syn_1827_shaped(1827)
        if name == "cox2":
            return "cox2_shaped_x64", synthetic.cox2_shaped(467).replicate(64)
        G = args.dense_graphs
        return (f"dense: {G} x ER(n={args.dense_nodes}, m={args.dense_edges}), generators.generate seed 0",
                generators.generate(["ER"] * G, [args.dense_nodes] * G, [args.dense_edges] * G, seed=0, backend="host"))

    def device_call(g, **kw):
        return sampling.sampled_tallies_device(g, classes, replicas=R, seed=seed, **kw)

    for key in args.shapes:
        name, g = shape(key)
        base = {"shape": name, "graphs": g.num_graphs, "nodes": g.num_nodes, "edges": g.num_directed_edges // 2,
                "replicas": R}
        # ---- the exact device census -------------------------------------------------------------------------------------
        exact = gt.canonical_counts_device(g, classes)               # (warm-up, and the truth of the error columns)
        node_graph = torch.from_numpy(g.node_graph_ids()).to(exact.device)
        exact_g = torch.zeros((g.num_graphs, len(classes)), dtype=torch.int64, device=exact.device) \
            .index_add_(0, node_graph, exact).cpu().numpy().astype(np.float64)
        exact5 = exact_g[:, five].sum(axis=1)
        del exact
        ts = []
        for _ in range(args.repeat):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = gt.canonical_counts_device(g, classes)
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) * 1e-3)
            del out
        exact_s = summary(ts)["median_s"]
        print(json.dumps({**base, "what": "exact device census (HIP events, uploads included)", **summary(ts),
                          "five_node_subsets": float(exact5.sum())}), flush=True)
        # ---- the schedules ---------------------------------------------------------------------------------------------------
        for kind in ("uniform", "leaf-only"):
            for f in FRACTIONS:
                if kind == "leaf-only" and f == 1.0:
                    continue                                         # (the same schedule as uniform 1)
                kw = dict(fraction=f) if kind == "uniform" else dict(probs=(1.0, 1.0, 1.0, f))
                _, probs, w = sampling.schedule(5, **kw)
                w5 = w[5]
                # the twin's work: the kept subsets it will visit.  Above --twin_budget it runs on the first graphs only
                kept = R * (exact_g / w[sizes]).sum(axis=1)
                twin_graphs = g.num_graphs
                if kept.sum() > args.twin_budget:
                    twin_graphs = int(max(1, np.searchsorted(np.cumsum(kept), args.twin_budget)))
                gh = g if twin_graphs == g.num_graphs else g.subset(0, twin_graphs)
                host_t, limit = [], args.repeat
                while len(host_t) < limit:
                    t0 = time.perf_counter()
                    ref = sampling.sampled_tallies(gh, classes, replicas=R, seed=seed, backend="host",
                                                   num_threads=args.threads, **kw)
                    host_t.append(time.perf_counter() - t0)
                    if host_t[-1] > args.once_above:
                        limit = 1
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                got = device_call(g, **kw)                           # (warm-up, and the comparison)
                b.record()
                torch.cuda.synchronize()
                warm = a.elapsed_time(b) * 1e-3
                assert torch.equal(got.cpu()[:, :twin_graphs], ref), f"{name} {kind} {f}: the kernel and the twin differ"
                tot = got.cpu().numpy()[:, :, five].sum(axis=2).astype(np.float64) * w5          # [R, G]
                del got
                est, se = tot.mean(axis=0), tot.std(axis=0, ddof=1) / np.sqrt(R)
                has = exact5 > 0
                with np.errstate(divide="ignore", invalid="ignore"):
                    rel_err = float(np.mean(np.abs(est[has] - exact5[has]) / exact5[has]))
                    ok = has & (est > 0)
                    rel_se = float(np.mean(se[ok] / est[ok])) if ok.any() else float("nan")
                dev_t = []
                for _ in range(1 if warm > args.once_above else args.repeat):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    out = device_call(g, **kw)
                    b.record()
                    torch.cuda.synchronize()
                    dev_t.append(a.elapsed_time(b) * 1e-3)
                    del out
                row = {**base, "schedule": kind, "fraction": f, "bit_identical": True,
                       "rel_err_5node_totals": rel_err, "stderr_over_estimate": rel_se,
                       "graphs_with_zero_estimate": int((has & (est == 0)).sum())}
                scale = float(kept.sum() / max(kept[:twin_graphs].sum(), 1.0))
                print(json.dumps({**row, "side": f"host twin, {args.threads} threads", **summary(host_t),
                                  "twin_graphs": twin_graphs, "kept_subsets_set_over_twin_graphs": scale}), flush=True)
                print(json.dumps({**row, "side": "device (HIP events, uploads included)", **summary(dev_t),
                                  "vs_twin_median": summary(host_t)["median_s"] * scale / summary(dev_t)["median_s"],
                                  "vs_exact_census_median": exact_s / summary(dev_t)["median_s"]}), flush=True)


if __name__ == "__main__":
    main()
