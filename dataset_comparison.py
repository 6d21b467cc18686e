"""Data set comparison: graphlet correlation distances between a training set and target sets.

For every graph of every set named in --targets the --k nearest graphs of --train by graphlet correlation distance
(desco_amd.comparison: Spearman correlations of the orbit columns --orbits over a graph's nodes, Euclidean distance of
their upper triangles) go to ``gcd-nearest_<i>.csv`` under --output_dir: target set, target graph, rank, training graph,
distance.  ``gcd-datasets_<i>.csv`` holds the distances between the sets as wholes -- all nodes of a set as one segment
-- for the training set and every target set.  <i> is the first free number.  Count / mean / std / min / quartiles /
max of the nearest distance are printed per target set.

--measure gdda (or both) does the same with the graphlet degree distribution agreement, which unlike the correlation
distance sees magnitude (two complete graphs of different sizes are at correlation distance 0): the --k training
graphs of largest agreement per target graph go to ``gdda-nearest_<i>.csv`` (..., agreement), the agreements between the
sets as wholes to ``gdda-datasets_<i>.csv``, over the orbit columns all5 unless --orbits says otherwise.

    python dataset_comparison.py --train Syn_1827_train --targets Syn_1827_test COX2 --k 5 [--measure both]
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
    p.add_argument("--measure", choices=("gcd", "gdda", "both"), default="gcd",
                   help="graphlet correlation distance, graphlet degree distribution agreement, or both")
    p.add_argument("--orbits", choices=("gcd11", "all4", "all5"), default=None,
                   help="default: gcd11 for the correlation distance, all5 for the distribution agreement")
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


def _gcd_tables(args, comparison, names, sets, i, result):
    kw = dict(orbits=args.orbits or "gcd11", induced=not args.noninduced, dummy_row=not args.no_dummy_row,
              backend=args.backend)
    train = sets[0]
    train_gcm = comparison.graphlet_correlation(train, **kw)
    print(f"{args.train}: {train.num_graphs} graphs, {len(train_gcm.columns)} orbit columns ({kw['orbits']}), "
          f"matrices by {comparison.last_backend}")
    k = max(1, min(args.k, train.num_graphs))
    near_path = os.path.join(args.output_dir, f"gcd-nearest_{i}.csv")
    sets_path = os.path.join(args.output_dir, f"gcd-datasets_{i}.csv")
    result.update({"nearest_csv": near_path, "datasets_csv": sets_path, "targets": {}})
    with open(near_path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["target_set", "target_graph", "rank", "train_graph", "distance"])
        for name, graphs in zip(names[1:], sets[1:]):
            gcm = comparison.graphlet_correlation(graphs, **kw)
            idx, dist = comparison.nearest(train_gcm, gcm, k=k, backend=args.backend)
            for g in range(graphs.num_graphs):
                for r in range(k):
                    w.writerow([name, g, r, int(idx[g, r]), repr(float(dist[g, r]))])
            s = summary(dist[:, 0])
            result["targets"][name] = s
            print(f"{name}: nearest distance to {args.train} ({comparison.last_backend}): " +
                  ", ".join(f"{key} {val:.6g}" for key, val in s.items()))
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


def _gdda_tables(args, comparison, names, sets, i, result):
    kw = dict(orbits=args.orbits or "all5", induced=not args.noninduced, backend=args.backend)
    train = sets[0]
    train_gdd = comparison.graphlet_distribution(train, **kw)
    print(f"{args.train}: {train.num_graphs} graphs, {len(train_gdd.columns)} orbit columns ({kw['orbits']}), "
          f"degree distributions by {comparison.last_backend}")
    k = max(1, min(args.k, train.num_graphs))
    near_path = os.path.join(args.output_dir, f"gdda-nearest_{i}.csv")
    sets_path = os.path.join(args.output_dir, f"gdda-datasets_{i}.csv")
    result.update({"gdda_nearest_csv": near_path, "gdda_datasets_csv": sets_path, "gdda_targets": {}})
    with open(near_path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["target_set", "target_graph", "rank", "train_graph", "agreement"])
        for name, graphs in zip(names[1:], sets[1:]):
            gdd = comparison.graphlet_distribution(graphs, **kw)
            idx, agree = comparison.gdd_nearest(train_gdd, gdd, k=k, backend=args.backend)
            for g in range(graphs.num_graphs):
                for r in range(k):
                    w.writerow([name, g, r, int(idx[g, r]), repr(float(agree[g, r]))])
            s = summary(agree[:, 0])
            result["gdda_targets"][name] = s
            print(f"{name}: nearest agreement with {args.train} ({comparison.last_backend}): " +
                  ", ".join(f"{key} {val:.6g}" for key, val in s.items()))
    d = comparison.dataset_gdda(sets, **kw)
    result["dataset_agreements"] = d
    with open(sets_path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["set"] + names)
        for a, row in zip(names, d):
            w.writerow([a] + [repr(float(v)) for v in row])
    print(f"data set agreements ({comparison.last_backend}):")
    for a, row in zip(names, d):
        print(f"  {a:>24s} " + " ".join(f"{v:9.4f}" for v in row))
    print(f"wrote {near_path} and {sets_path}")


def main(argv=None) -> dict:
    args = parse_args(argv)
    from desco_amd import comparison
    from desco_amd.data import load_data
    names = [args.train] + list(args.targets)
    sets = [load_data(name, root_folder=args.data_root) for name in names]
    os.makedirs(args.output_dir, exist_ok=True)
    stems = [stem for on, pair in ((args.measure != "gdda", ("gcd-nearest", "gcd-datasets")),
                                   (args.measure != "gcd", ("gdda-nearest", "gdda-datasets"))) if on for stem in pair]
    i = first_free(args.output_dir, stems)
    result = {}
    if args.measure != "gdda":
        _gcd_tables(args, comparison, names, sets, i, result)
    if args.measure != "gcd":
        _gdda_tables(args, comparison, names, sets, i, result)
    return result


if __name__ == "__main__":
    main()
