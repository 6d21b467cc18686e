"""Data set comparison: graphlet correlation distances between a training set and target sets.

For every graph of every set named in --targets the --k nearest graphs of --train by graphlet correlation distance
(desco_amd.comparison: Spearman correlations of the orbit columns --orbits over a graph's nodes, Euclidean distance of
their upper triangles) go to ``gcd-nearest_<i>.csv`` under --output_dir: target set, target graph, rank, training graph,
distance.  ``gcd-datasets_<i>.csv`` holds the distances between the sets as wholes -- all nodes of a set as one segment
-- for the training set and every target set.  <i> is the first free number.  Count / mean / std / min / quartiles /
max of the nearest distance are printed per target set.

    python dataset_comparison.py --train Syn_1827_train --targets Syn_1827_test COX2 --k 5
"""
import argparse
import csv
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--train", default="Syn_1827", help="a name desco_amd.data.load_data knows")
    p.add_argument("--targets", nargs="+", default=["COX2"], help="names desco_amd.data.load_data knows")
    p.add_argument("--orbits", choices=("gcd11", "all4", "all5"), default="gcd11")
    p.add_argument("--k", type=int, default=5, help="nearest training graphs per target graph")
    p.add_argument("--noninduced", action="store_true", help="non-induced orbit counts (orbit_counts(induced=False))")
    p.add_argument("--no_dummy_row", action="store_true", help="leave the extra row of ones out of every segment")
    p.add_argument("--backend", choices=("auto", "host", "device"), default="auto")
    p.add_argument("--output_dir", default=os.path.join("results", "comparison"))
    p.add_argument("--data_root", default="data", help="folder of the raw data sets")
    return p.parse_args(argv)


def first_free(output_dir: str, stems) -> int:
    i = 0
    while any(os.path.exists(os.path.join(output_dir, f"{stem}_{i}.csv")) for stem in stems):
        i += 1
    return i


def summary(values: np.ndarray) -> dict:
    if len(values) == 0:
        return {"count": 0}
    q = np.percentile(values, [25, 50, 75])
    return {"count": int(len(values)), "mean": float(values.mean()), "std": float(values.std()),
            "min": float(values.min()), "25%": float(q[0]), "50%": float(q[1]), "75%": float(q[2]),
            "max": float(values.max())}


def main(argv=None) -> dict:
    args = parse_args(argv)
    from desco_amd import comparison
    from desco_amd.data import load_data
    kw = dict(orbits=args.orbits, induced=not args.noninduced, dummy_row=not args.no_dummy_row, backend=args.backend)
    train = load_data(args.train, root_folder=args.data_root)
    train_gcm = comparison.graphlet_correlation(train, **kw)
    print(f"{args.train}: {train.num_graphs} graphs, {len(train_gcm.columns)} orbit columns ({args.orbits}), "
          f"matrices by {comparison.last_backend}")
    k = max(1, min(args.k, train.num_graphs))
    os.makedirs(args.output_dir, exist_ok=True)
    i = first_free(args.output_dir, ("gcd-nearest", "gcd-datasets"))
    near_path = os.path.join(args.output_dir, f"gcd-nearest_{i}.csv")
    sets_path = os.path.join(args.output_dir, f"gcd-datasets_{i}.csv")
    result = {"nearest_csv": near_path, "datasets_csv": sets_path, "targets": {}}
    sets = [train]
    with open(near_path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["target_set", "target_graph", "rank", "train_graph", "distance"])
        for name in args.targets:
            graphs = load_data(name, root_folder=args.data_root)
            sets.append(graphs)
            gcm = comparison.graphlet_correlation(graphs, **kw)
            idx, dist = comparison.nearest(train_gcm, gcm, k=k, backend=args.backend)
            for g in range(graphs.num_graphs):
                for r in range(k):
                    w.writerow([name, g, r, int(idx[g, r]), repr(float(dist[g, r]))])
            s = summary(dist[:, 0])
            result["targets"][name] = s
            print(f"{name}: nearest distance to {args.train} ({comparison.last_backend}): " +
                  ", ".join(f"{key} {val:.6g}" for key, val in s.items()))
    names = [args.train] + list(args.targets)
    d = comparison.dataset_gcd(sets, **kw)
    result["dataset_distances"] = d
    with open(sets_path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["set"] + names)
        for a, row in zip(names, d):
            w.writerow([a] + [repr(float(v)) for v in row])
    print(f"data set distances ({comparison.last_backend}):")
    for a, row in zip(names, d):
        print(f"  {a:>24s} " + " ".join(f"{v:9.4f}" for v in row))
    print(f"wrote {near_path} and {sets_path}")
    return result


if __name__ == "__main__":
    main()
