"""Motif significance: z-scores of the connected query graphs against degree-preserving null models.

For every data set named in --datasets the connected graphs of --query_size nodes are counted (exact census; with
--noninduced the non-induced counts) in every graph and in --replicas rewired copies of it (double edge switches,
--swaps_per_edge attempts per edge, every node keeps its degree), and per graph and query the mean and the standard
deviation of the null counts, the z-score, the significance profile and the empirical p-values are written to
``motif-zscores_<i>.csv`` under --output_dir, <i> being the first free number; the same for the data set's totals goes
to ``motif-zscores-dataset_<i>.csv`` and is printed.

    python motif_significance.py --datasets Syn_1827 COX2 --replicas 100 --output_dir results/motifs
"""
import argparse
import csv
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

VALUES = ["real", "mean", "std", "z", "profile", "p_over", "p_under"]
HEADER = ["", "dataset", "graph", "query", "query_nodes", "query_edges"] + VALUES
DATASET_HEADER = ["", "dataset", "query", "query_nodes", "query_edges"] + VALUES


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--datasets", nargs="+", default=["Syn_1827"], help="names desco_amd.data.load_data knows")
    p.add_argument("--replicas", type=int, default=100, help="rewired copies per graph (at least 2)")
    p.add_argument("--swaps_per_edge", type=int, default=10, help="switch attempts per edge of a chain")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--query_size", type=int, nargs="+", default=[3, 4, 5], choices=(2, 3, 4, 5))
    p.add_argument("--noninduced", action="store_true", help="non-induced counts instead of induced ones")
    p.add_argument("--backend", choices=("auto", "host", "device"), default="auto")
    p.add_argument("--output_dir", default=os.path.join("results", "motifs"))
    p.add_argument("--data_root", default="data", help="folder of the raw data sets")
    return p.parse_args(argv)


def first_free(output_dir: str, stem: str) -> str:
    i = 0
    while os.path.exists(os.path.join(output_dir, f"{stem}_{i}.csv")):
        i += 1
    return os.path.join(output_dir, f"{stem}_{i}.csv")


def _cell(name, value):
    return int(value) if name == "real" else repr(float(value))


def write_csv(path: str, header, tables, queries) -> int:
    """tables: [(dataset name, {column: array})]; one CSV, a running index in the first column.  Returns the rows."""
    row = 0
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(header)
        for name, table in tables:
            for k in range(len(table["query"])):
                q = int(table["query"][k])
                lead = [row, name] + ([int(table["graph"][k])] if "graph" in header else [])
                edges = " ".join(f"{a}-{b}" for a, b in queries[q][1])
                w.writerow(lead + [q, queries[q][0], edges] + [_cell(c, table[c][k]) for c in VALUES])
                row += 1
    return row


def describe(title: str, table, queries) -> None:
    print(title)
    print("  {:>5s} {:>5s} {:>14s} {:>14s} {:>12s} {:>9s} {:>8s} {:>8s} {:>8s}".format(
        "query", "nodes", "real", "mean", "std", "z", "profile", "p_over", "p_under"))
    for k, q in enumerate(table["query"]):
        print("  {:>5d} {:>5d} {:>14d} {:>14.2f} {:>12.3f} {:>9.3f} {:>8.4f} {:>8.4f} {:>8.4f}".format(
            int(q), queries[int(q)][0], int(table["real"][k]), table["mean"][k], table["std"][k], table["z"][k],
            table["profile"][k], table["p_over"][k], table["p_under"][k]))


def main(argv=None) -> dict:
    args = parse_args(argv)
    from desco_amd import motifs
    from desco_amd.data import load_data
    from desco_amd.groundtruth import census_classes
    queries = [(k, tuple(e)) for k in sorted(set(args.query_size)) for _, e in census_classes(k)]
    per_graph, totals = [], []
    for name in args.datasets:
        graphs = load_data(name, root_folder=args.data_root)
        res = motifs.motif_significance(graphs, queries, replicas=args.replicas, swaps_per_edge=args.swaps_per_edge,
                                        seed=args.seed, induced=not args.noninduced, backend=args.backend)
        per_graph.append((name, res.table()))
        totals.append((name, res.dataset_table()))
        describe(f"{name}: {graphs.num_graphs} graphs, {args.replicas} replicas, "
                 f"{'non-induced' if args.noninduced else 'induced'} counts ({res.last_backend})", totals[-1][1], queries)
    os.makedirs(args.output_dir, exist_ok=True)
    out = {"graphs": first_free(args.output_dir, "motif-zscores"),
           "dataset": first_free(args.output_dir, "motif-zscores-dataset")}
    rows = write_csv(out["graphs"], HEADER, per_graph, queries)
    print(f"wrote {rows} rows to {out['graphs']}")
    rows = write_csv(out["dataset"], DATASET_HEADER, totals, queries)
    print(f"wrote {rows} rows to {out['dataset']}")
    return out


if __name__ == "__main__":
    main()
