"""Clique census of data sets: the exact number of k-cliques of every graph, and through every node, for k up to --kmax.

For every data set named in --datasets the cliques of every graph are counted by pivoting (desco_amd.cliques: the HIP
kernels or their host twins) and ``graph-cliques_<i>.csv`` (graph, omega = the clique number, k1 .. k<kmax>) is written
under --output_dir; with --nodes also ``node-cliques_<i>.csv`` (graph, node, core, k1 .. k<kmax> = the k-cliques that
contain the node).  <i> is the first free number; node ids are local to their graph.  Per data set, omega and every
column get the usual summary (count, mean, std, min, quartiles, max).

    python clique_census.py --datasets Syn_1827 COX2 --kmax 8 --nodes --output_dir results/cliques
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from graph_decomposition import describe, first_free, write_csv  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--datasets", nargs="+", default=["Syn_1827"], help="names desco_amd.data.load_data knows")
    p.add_argument("--kmax", type=int, default=8, help="count the cliques of 1 .. kmax nodes (at most 64)")
    p.add_argument("--nodes", action="store_true", help="also write the per-node table")
    p.add_argument("--backend", choices=("auto", "host", "device"), default="auto")
    p.add_argument("--output_dir", default=os.path.join("results", "cliques"))
    p.add_argument("--data_root", default="data", help="folder of the raw data sets")
    return p.parse_args(argv)


def main(argv=None) -> dict:
    args = parse_args(argv)
    from desco_amd import cliques
    from desco_amd.data import load_data
    ks = [f"k{k}" for k in range(1, args.kmax + 1)]
    graph_columns, node_columns = ["graph", "omega"] + ks, ["graph", "node", "core"] + ks
    per = {"graph": [], "node": []}
    for name in args.datasets:
        graphs = load_data(name, root_folder=args.data_root)
        res = cliques.clique_census(graphs, kmax=args.kmax, nodes=args.nodes, backend=args.backend)
        table = res.graph_table()
        per["graph"].append((name, table))
        print(f"{name}: {graphs.num_graphs} graphs, {graphs.num_nodes} nodes, kmax {args.kmax} ({res.last_backend})")
        describe("  graphs", graph_columns[1:], table)
        if args.nodes:
            node_graph = graphs.node_graph_ids()
            nodes = {"graph": node_graph, "node": np.arange(graphs.num_nodes) - graphs.graph_ptr[:-1][node_graph],
                     "core": cliques.peel_order(graphs, backend=args.backend)[1]}
            nodes.update({c: res.node_cliques[:, k] for k, c in enumerate(ks)})
            per["node"].append((name, nodes))
            describe("  nodes", node_columns[2:], nodes)
    os.makedirs(args.output_dir, exist_ok=True)
    out = {"graph": first_free(args.output_dir, "graph-cliques")}
    if args.nodes:
        out["node"] = first_free(args.output_dir, "node-cliques")
    for kind, columns in (("graph", graph_columns), ("node", node_columns)):
        if kind in out:
            rows = write_csv(out[kind], columns, per[kind])
            print(f"wrote {rows} rows to {out[kind]}")
    return out


if __name__ == "__main__":
    main()
