"""Expressiveness bounds of the model families on data sets: colour classes and the error floors they force.

For every data set named in --datasets and every view in --views the canonical neighborhoods are refined for --rounds
rounds (desco_amd.expressiveness: the HIP kernel or its host twin) and the exact canonical counts of the queries of
--query_size (groundtruth.canonical_counts) are laid over the classes: neighborhoods that no --rounds-layer model of the
family can tell apart but whose counts differ force an error on it.  One table, ``expressiveness_<i>.csv`` with the first
free <i> under --output_dir: data set, level, view, rounds, sets, classes, then per query ``ambiguous_sets``,
``ambiguous_classes``, ``mse_floor`` and ``norm_mse_floor`` (log2(1 + count) space, the neighborhood loss's).  "plain"
reads the restricted neighborhoods ablation_gnns.py trains on, "hetero" and "shmp" those of main.py (--restricted /
--no-restricted override); --graphs adds the whole-graph level for "plain" and "shmp" (the ablation_wo_canonical.py
setting).  A floor is a lower bound for that depth and family, not a prediction; the classes are exact up to a 64-bit
hash collision.  A summary grouped by query size is printed.

    python expressiveness.py --datasets COX2 Syn_1827 --graphs --output_dir results/expressiveness
"""
import argparse
import csv
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HEAD_COLUMNS = ["dataset", "level", "view", "rounds", "sets", "classes"]
QUERY_COLUMNS = ["ambiguous_sets", "ambiguous_classes", "mse_floor", "norm_mse_floor"]


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--datasets", nargs="+", default=["Syn_1827"], help="names desco_amd.data.load_data knows")
    p.add_argument("--depth", type=int, default=4)
    p.add_argument("--rounds", type=int, default=8)
    p.add_argument("--views", nargs="+", default=["plain", "hetero", "shmp"], choices=("plain", "hetero", "shmp"))
    p.add_argument("--query_size", nargs="+", type=int, default=[3, 4, 5])
    p.add_argument("--graphs", action="store_true", help="add the whole-graph level (plain and shmp)")
    p.add_argument("--restricted", dest="restricted", action="store_true", default=None,
                   help="restricted neighborhoods for every view (default: for plain only)")
    p.add_argument("--no-restricted", dest="restricted", action="store_false")
    p.add_argument("--backend", choices=("auto", "host", "device"), default="auto")
    p.add_argument("--output_dir", default=os.path.join("results", "expressiveness"))
    p.add_argument("--data_root", default="data", help="folder of the raw data sets")
    return p.parse_args(argv)


def first_free(output_dir: str, stem: str) -> str:
    i = 0
    while os.path.exists(os.path.join(output_dir, f"{stem}_{i}.csv")):
        i += 1
    return os.path.join(output_dir, f"{stem}_{i}.csv")


def rows_of(name, graphs, args, query_ids, queries) -> list:
    """[(head dict, ErrorFloor)]: one per (level, view) of a data set"""
    from desco_amd import expressiveness as X
    out, truth_at = [], {}
    for view in args.views:
        restricted = (view == "plain") if args.restricted is None else args.restricted
        classes = X.neighborhood_classes(graphs, args.depth, args.rounds, view, restricted, backend=args.backend)
        if restricted not in truth_at:                     # both definitions list the same canonical nodes
            truth_at[restricted] = X.neighborhood_truth(graphs, classes, queries, backend=args.backend)
        head = {"dataset": name, "level": "neighborhood" + ("/restricted" if restricted else ""), "view": view,
                "rounds": args.rounds, "sets": classes.num_sets, "classes": classes.num_classes}
        out.append((head, X.error_floor(classes, truth_at[restricted])))
        print(f"  {head['level']:<24s}{view:<8s}{classes.num_sets:>10d} sets{classes.num_classes:>10d} classes "
              f"({classes.last_backend})", flush=True)
    if args.graphs:
        truth = X.graph_truth(graphs, queries, backend=args.backend)
        for view in (v for v in args.views if v != "hetero"):
            classes = X.graph_classes(graphs, args.rounds, view, backend=args.backend)
            head = {"dataset": name, "level": "graph", "view": view, "rounds": args.rounds, "sets": classes.num_sets,
                    "classes": classes.num_classes}
            out.append((head, X.error_floor(classes, truth)))
            print(f"  {'graph':<24s}{view:<8s}{classes.num_sets:>10d} sets{classes.num_classes:>10d} classes "
                  f"({classes.last_backend})", flush=True)
    return out


def write_csv(path: str, query_ids, rows) -> int:
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow([""] + HEAD_COLUMNS + [f"{c}_{q}" for q in query_ids for c in QUERY_COLUMNS])
        for k, (head, floor) in enumerate(rows):
            line = [k] + [head[c] for c in HEAD_COLUMNS]
            for r in floor.table(query_ids):
                line += [r["ambiguous_sets"], r["ambiguous_classes"], repr(r["mse_floor"]), repr(r["norm_mse_floor"])]
            w.writerow(line)
    return len(rows)


def summarise(rows, query_ids, sizes) -> None:
    """per (level, view) and query size: ambiguous sets of the worst query, mean mse / norm-mse floor over the size's queries"""
    print("{:<10s}{:<24s}{:<8s}{:>6s}{:>16s}{:>14s}{:>16s}".format("dataset", "level", "view", "size", "ambiguous_sets",
                                                                   "mse_floor", "norm_mse_floor"))
    for head, floor in rows:
        for size in sorted(set(sizes)):
            cols = [k for k, s in enumerate(sizes) if s == size]
            nm = floor.norm_mse_floor[cols]
            print("{:<10s}{:<24s}{:<8s}{:>6d}{:>16d}{:>14.3e}{:>16.3e}".format(
                head["dataset"], head["level"], head["view"], size, int(floor.ambiguous_sets[cols].max()),
                float(floor.mse_floor[cols].mean()), float(np.nanmean(nm)) if np.isfinite(nm).any() else float("nan")))


def main(argv=None) -> str:
    args = parse_args(argv)
    from desco_amd.data import gen_query_ids, graph_atlas_plus, load_data
    query_ids = gen_query_ids(query_size=args.query_size)
    queries = [graph_atlas_plus(i) for i in query_ids]
    sizes = [q.number_of_nodes() for q in queries]
    rows = []
    for name in args.datasets:
        graphs = load_data(name, root_folder=args.data_root)
        print(f"{name}: {graphs.num_graphs} graphs, {graphs.num_nodes} nodes, {len(queries)} queries", flush=True)
        rows += rows_of(name, graphs, args, query_ids, queries)
    os.makedirs(args.output_dir, exist_ok=True)
    path = first_free(args.output_dir, "expressiveness")
    print(f"wrote {write_csv(path, query_ids, rows)} rows to {path}")
    summarise(rows, query_ids, sizes)
    return path


if __name__ == "__main__":
    main()
