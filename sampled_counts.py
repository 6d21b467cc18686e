"""Sampled subgraph counts: RAND-ESU estimates with error bars for the queries of the requested sizes.

For every data set named in --datasets the graph-level counts of the connected graph-atlas patterns of --query_size
are estimated from --replicas sampled walks of the exact census's enumeration tree (desco_amd.sampling; schedule:
--fraction, the uniform one, or --probs p2 p3 .., one probability per level).  One row per (graph, query) goes to
``sampled-counts_<i>.csv`` under --output_dir, <i> being the first free number: dataset, graph, query, estimate, stderr
and, with --compare_exact, the exact count.  --compare_exact also prints norm-MSE and MAE by query size -- the figures
main.py prints for the model -- and the wall time of the sampled and of the exact call.

    python sampled_counts.py --datasets Syn_1827 COX2 --fraction 0.01 --replicas 16 --compare_exact
"""
import argparse
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--datasets", nargs="+", default=["Syn_1827"], help="names desco_amd.data.load_data knows")
    s = p.add_mutually_exclusive_group()
    s.add_argument("--fraction", type=float, default=None,
                   help="uniform schedule: a subset of the largest size survives with this probability (default 0.01)")
    s.add_argument("--probs", type=float, nargs="+", default=None,
                   help="explicit schedule: the probabilities of the levels 2, 3, .. up to the largest query size")
    p.add_argument("--replicas", type=int, default=16)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--query_size", type=int, nargs="+", default=[3, 4, 5], help="sizes in 2..6 (6: host only)")
    p.add_argument("--noninduced", action="store_true", help="non-induced counts (canonical_counts(induced=False))")
    p.add_argument("--backend", choices=("auto", "host", "device"), default="auto")
    p.add_argument("--compare_exact", action="store_true", help="also run the exact census and print the errors")
    p.add_argument("--output_dir", default=os.path.join("results", "sampled"))
    p.add_argument("--data_root", default="data", help="folder of the raw data sets")
    return p.parse_args(argv)


def first_free(output_dir: str, stem: str) -> str:
    i = 0
    while os.path.exists(os.path.join(output_dir, f"{stem}_{i}.csv")):
        i += 1
    return os.path.join(output_dir, f"{stem}_{i}.csv")


def _sync():
    import torch
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def main(argv=None) -> dict:
    args = parse_args(argv)
    from desco_amd import analysis, groundtruth, sampling
    from desco_amd.data import load_data
    sizes = sorted(set(args.query_size))
    queries = [q for k in sizes for q in groundtruth.census_classes(k)]
    groupby = [[i for i, (n, _) in enumerate(queries) if n == k] for k in sizes]
    schedule = dict(probs=args.probs) if args.probs is not None else \
        dict(fraction=0.01 if args.fraction is None else args.fraction)
    os.makedirs(args.output_dir, exist_ok=True)
    path = first_free(args.output_dir, "sampled-counts")
    result = {"csv": path, "datasets": {}}
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["dataset", "graph", "query", "estimate", "stderr"] + (["exact"] if args.compare_exact else []))
        for name in args.datasets:
            graphs = load_data(name, root_folder=args.data_root)
            _sync()
            t0 = time.perf_counter()
            est = sampling.estimate_counts(graphs, queries, replicas=args.replicas, seed=args.seed,
                                           backend=args.backend, induced=not args.noninduced, **schedule)
            _sync()
            t_sampled = time.perf_counter() - t0
            print(f"{name}: {graphs.num_graphs} graphs, {len(queries)} queries of sizes {sizes}, {args.replicas} "
                  f"replicas, level probabilities {np.round(est.probs, 6).tolist()} ({est.last_backend}): "
                  f"{t_sampled:.3f} s")
            info = {"sampled_seconds": t_sampled, "backend": est.last_backend}
            exact = None
            if args.compare_exact:
                t0 = time.perf_counter()
                nodes = groundtruth.canonical_counts(graphs, queries, backend=args.backend,
                                                     induced=not args.noninduced).numpy()
                t_exact = time.perf_counter() - t0
                cs = np.concatenate([np.zeros((1, nodes.shape[1])), np.cumsum(nodes, axis=0)])
                exact = cs[graphs.graph_ptr[1:]] - cs[graphs.graph_ptr[:-1]]
                with np.errstate(divide="ignore", invalid="ignore"):
                    nmse = analysis.norm_mse(est.estimate, exact, groupby)
                    mae = analysis.mae(est.estimate, exact, groupby)
                print(f"{name}: exact census {t_exact:.3f} s")
                for k, a, b in zip(sizes, nmse, mae):
                    print(f"  size {k}: norm MSE {a:.4e}, MAE {b:.4e}")
                info.update(exact_seconds=t_exact, norm_mse=nmse, mae=mae)
            table = est.table()
            for i in range(len(table["graph"])):
                row = [name, int(table["graph"][i]), int(table["query"][i]), repr(float(table["estimate"][i])),
                       repr(float(table["stderr"][i]))]
                if exact is not None:
                    row.append(int(exact[table["graph"][i], table["query"][i]]))
                w.writerow(row)
            result["datasets"][name] = info
    print(f"wrote {path}")
    return result


if __name__ == "__main__":
    main()
