"""k-core and k-truss decomposition of data sets: core number per node, support and truss number per edge.

For every data set named in --datasets every graph is peeled (desco_amd.decomposition: the HIP kernel or its host twin)
and three tables are written under --output_dir, each with the first free number <i>: ``node-core_<i>.csv`` (graph,
node, degree, core, node_truss = the largest truss number among the node's edges), ``edge-truss_<i>.csv`` (graph, u, v,
support = triangles through the edge, truss) and ``graph-decomposition_<i>.csv`` (degeneracy, max_truss,
nodes_in_top_core, edges_in_top_truss, triangles per graph).  Node ids are local to their graph.  Per data set and
column the usual summary (count, mean, std, min, quartiles, max) is printed.

    python graph_decomposition.py --datasets Syn_1827 COX2 --output_dir results/decomposition
"""
import argparse
import csv
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NODE_COLUMNS = ["graph", "node", "degree", "core", "node_truss"]
EDGE_COLUMNS = ["graph", "u", "v", "support", "truss"]
GRAPH_COLUMNS = ["graph", "degeneracy", "max_truss", "nodes_in_top_core", "edges_in_top_truss", "triangles"]


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--datasets", nargs="+", default=["Syn_1827"], help="names desco_amd.data.load_data knows")
    p.add_argument("--backend", choices=("auto", "host", "device"), default="auto")
    p.add_argument("--output_dir", default=os.path.join("results", "decomposition"))
    p.add_argument("--data_root", default="data", help="folder of the raw data sets")
    return p.parse_args(argv)


def first_free(output_dir: str, stem: str) -> str:
    i = 0
    while os.path.exists(os.path.join(output_dir, f"{stem}_{i}.csv")):
        i += 1
    return os.path.join(output_dir, f"{stem}_{i}.csv")


def tables(graphs, res) -> dict:
    """The three tables of one data set, {name: {column: int array}}."""
    node_graph = graphs.node_graph_ids()
    first = graphs.graph_ptr[:-1]
    edge_graph = node_graph[res.rows[:, 0]]
    return {
        "node": {"graph": node_graph, "node": np.arange(graphs.num_nodes) - first[node_graph],
                 "degree": np.diff(graphs.rowptr), "core": res.core, "node_truss": res.node_truss},
        "edge": {"graph": edge_graph, "u": res.rows[:, 0] - first[edge_graph], "v": res.rows[:, 1] - first[edge_graph],
                 "support": res.support, "truss": res.truss},
        "graph": res.graph_table(),
    }


def write_csv(path: str, columns, named_tables) -> int:
    """named_tables: [(dataset name, {column: array})]; one CSV, a running index in the first column.  Returns the rows."""
    row = 0
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["", "dataset"] + columns)
        for name, table in named_tables:
            cols = [table[c] for c in columns]
            for k in range(len(cols[0])):
                w.writerow([row, name] + [int(c[k]) for c in cols])
                row += 1
    return row


def describe(title: str, columns, table) -> None:
    print(title)
    print("  {:<22s}{:>9s}{:>12s}{:>12s}{:>10s}{:>10s}{:>10s}{:>10s}{:>10s}".format(
        "", "count", "mean", "std", "min", "25%", "50%", "75%", "max"))
    for c in columns:
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
    from desco_amd import decomposition
    from desco_amd.data import load_data
    per = {"node": [], "edge": [], "graph": []}
    for name in args.datasets:
        graphs = load_data(name, root_folder=args.data_root)
        res = decomposition.decompose(graphs, backend=args.backend)
        t = tables(graphs, res)
        for kind in per:
            per[kind].append((name, t[kind]))
        print(f"{name}: {graphs.num_graphs} graphs, {graphs.num_nodes} nodes, {len(res.truss)} edges "
              f"({res.last_backend})")
        describe("  nodes", NODE_COLUMNS[2:], t["node"])
        describe("  edges", EDGE_COLUMNS[3:], t["edge"])
        describe("  graphs", GRAPH_COLUMNS[1:], t["graph"])
    os.makedirs(args.output_dir, exist_ok=True)
    out = {"node": first_free(args.output_dir, "node-core"), "edge": first_free(args.output_dir, "edge-truss"),
           "graph": first_free(args.output_dir, "graph-decomposition")}
    for kind, columns in (("node", NODE_COLUMNS), ("edge", EDGE_COLUMNS), ("graph", GRAPH_COLUMNS)):
        rows = write_csv(out[kind], columns, per[kind])
        print(f"wrote {rows} rows to {out[kind]}")
    return out


if __name__ == "__main__":
    main()
