"""Data-set coverage statistics: seven graph features per canonical neighborhood (and, with --graphs, per graph).

For every data set named in --datasets the canonical neighborhoods are built at --depth and each one's largest
connected component is measured: clustering, shortest_path_length, diameter, density, num_nodes, num_edges, avg_degree
(the values nx.average_clustering, nx.average_shortest_path_length, nx.diameter and nx.density return on it).  The
rows of all data sets go to ``neighborhood-features_<i>.csv`` under --output_dir, <i> being the first free number;
--graphs also writes ``graph-features_<i>.csv`` with the same columns for whole graphs.  Per data set and column the
usual summary (count, mean, std, min, quartiles, max) is printed.

    python dataset_statistics.py --datasets Syn_1827 COX2 --depth 4 --output_dir results/statistics
"""
import argparse
import csv
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HEADER = ["", "dataset", "clustering", "shortest_path_length", "diameter", "density", "num_nodes", "num_edges",
          "avg_degree"]
INT_COLUMNS = ("diameter", "num_nodes", "num_edges")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--datasets", nargs="+", default=["Syn_1827"], help="names desco_amd.data.load_data knows")
    p.add_argument("--depth", type=int, default=4, help="neighborhood radius")
    p.add_argument("--restricted", action="store_true",
                   help="the homogeneous ablation's neighborhoods (BFS that only steps onto smaller ids)")
    p.add_argument("--graphs", action="store_true", help="also write graph-features_<i>.csv (whole graphs)")
    p.add_argument("--output_dir", default=os.path.join("results", "statistics"))
    p.add_argument("--backend", choices=("auto", "host", "device"), default="auto")
    p.add_argument("--data_root", default="data", help="folder of the raw data sets")
    return p.parse_args(argv)


def first_free(output_dir: str, stem: str) -> str:
    i = 0
    while os.path.exists(os.path.join(output_dir, f"{stem}_{i}.csv")):
        i += 1
    return os.path.join(output_dir, f"{stem}_{i}.csv")


def write_csv(path: str, tables) -> int:
    """tables: [(dataset name, {column: array})]; one CSV, a running index in the first column.  Returns the rows."""
    row = 0
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(HEADER)
        for name, table in tables:
            cols = [table[c] for c in HEADER[2:]]
            for k in range(len(cols[0])):
                w.writerow([row, name] + [int(c[k]) if h in INT_COLUMNS else repr(float(c[k]))
                                          for h, c in zip(HEADER[2:], cols)])
                row += 1
    return row


def describe(title: str, table) -> None:
    print(title)
    print("  {:<22s}{:>9s}{:>12s}{:>12s}{:>10s}{:>10s}{:>10s}{:>10s}{:>10s}".format(
        "", "count", "mean", "std", "min", "25%", "50%", "75%", "max"))
    for c in HEADER[2:]:
        x = np.asarray(table[c], dtype=np.float64)
        if len(x) == 0:
            print(f"  {c:<22s}{0:>9d}")
            continue
        q = np.percentile(x, [25, 50, 75])
        std = float(np.std(x, ddof=1)) if len(x) > 1 else float("nan")
        print("  {:<22s}{:>9d}{:>12.5f}{:>12.5f}{:>10.4g}{:>10.4g}{:>10.4g}{:>10.4g}{:>10.4g}".format(
            c, len(x), float(x.mean()), std, float(x.min()), q[0], q[1], q[2], float(x.max())))


def main(argv=None) -> dict:
    args = parse_args(argv)
    from desco_amd import analysis
    from desco_amd.data import load_data
    neigh, whole = [], []
    for name in args.datasets:
        graphs = load_data(name, root_folder=args.data_root)
        stats = analysis.neighborhood_statistics(graphs, depth=args.depth, restricted=args.restricted,
                                                 backend=args.backend)
        neigh.append((name, stats.table()))
        describe(f"{name}: {len(stats)} neighborhoods at depth {args.depth} ({analysis.last_stats_backend})",
                 neigh[-1][1])
        if args.graphs:
            gstats = analysis.graph_statistics(graphs, backend=args.backend)
            whole.append((name, gstats.table()))
            describe(f"{name}: {len(gstats)} graphs ({analysis.last_stats_backend})", whole[-1][1])
    os.makedirs(args.output_dir, exist_ok=True)
    out = {"neighborhood": first_free(args.output_dir, "neighborhood-features")}
    rows = write_csv(out["neighborhood"], neigh)
    print(f"wrote {rows} rows to {out['neighborhood']}")
    if args.graphs:
        out["graph"] = first_free(args.output_dir, "graph-features")
        rows = write_csv(out["graph"], whole)
        print(f"wrote {rows} rows to {out['graph']}")
    return out


if __name__ == "__main__":
    main()
