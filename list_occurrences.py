"""List the occurrences of one query in data sets: the node tuples of every copy, not just their number.

For every data set named in --datasets every occurrence of the query (--atlas_id: a graph-atlas pattern; --edges: an
edge list such as "0-1 1-2 2-0") is listed by the matcher (desco_amd.occurrences: the HIP kernel or its host twin) and
``occurrences_<i>.csv`` (data set, graph, v0 .. v<k-1> = the image of every query node, local to its graph) is written
under --output_dir; <i> is the first free number.  By default an occurrence is an INDUCED subgraph isomorphic to the
query; --noninduced lists every copy of the query's edges.  Per data set the occurrences per graph get the usual summary
(count, mean, std, min, quartiles, max).  More than --max_rows occurrences are streamed into the CSV chunk by chunk.

    python list_occurrences.py --datasets COX2 --edges "0-1 1-2 2-3 3-4 4-5 5-0" --output_dir results/occurrences
"""
import argparse
import csv
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from graph_decomposition import describe, first_free  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--datasets", nargs="+", default=["COX2"], help="names desco_amd.data.load_data knows")
    q = p.add_mutually_exclusive_group(required=True)
    q.add_argument("--atlas_id", type=int, help="the query: a graph-atlas id (connected, 2..7 nodes)")
    q.add_argument("--edges", help='the query: its edges, "0-1 1-2 ..." (nodes 0..k-1, connected, 2..16 nodes)')
    p.add_argument("--noninduced", action="store_true", help="list copies of the query's edges, induced or not")
    p.add_argument("--max_rows", type=int, default=1 << 26, help="rows listed at a time; more are streamed in chunks")
    p.add_argument("--backend", choices=("auto", "host", "device", "vf2"), default="auto")
    p.add_argument("--use_node_feature", action="store_true", help="not supported: occurrences are unlabelled")
    p.add_argument("--output_dir", default=os.path.join("results", "occurrences"))
    p.add_argument("--data_root", default="data", help="folder of the raw data sets")
    args = p.parse_args(argv)
    if args.use_node_feature:
        p.error("--use_node_feature: labelled queries are not listed (only unlabelled occurrences are); "
                "canonical_counts_labelled counts them")
    return args


def read_query(args):
    if args.atlas_id is not None:
        from desco_amd.data import graph_atlas_plus
        g = graph_atlas_plus(args.atlas_id)
        return g.number_of_nodes(), sorted(tuple(sorted(e)) for e in g.edges())
    edges = [tuple(int(x) for x in e.split("-")) for e in args.edges.split()]
    if not edges or any(len(e) != 2 for e in edges):
        raise SystemExit('--edges: expected "a-b c-d ..."')
    return max(max(e) for e in edges) + 1, edges


def main(argv=None) -> dict:
    args = parse_args(argv)
    from desco_amd import occurrences
    from desco_amd.data import load_data
    k, edges = query = read_query(args)
    induced = not args.noninduced
    os.makedirs(args.output_dir, exist_ok=True)
    path = first_free(args.output_dir, "occurrences")
    columns = ["graph"] + [f"v{a}" for a in range(k)]
    row = 0
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["", "dataset"] + columns)
        for name in args.datasets:
            graphs = load_data(name, root_folder=args.data_root)
            per_graph = np.zeros(graphs.num_graphs, dtype=np.int64)
            common = dict(induced=induced, backend=args.backend, max_rows=args.max_rows)
            try:
                chunks = [occurrences.list_occurrences(graphs, query, **common)]
            except ValueError as e:
                if "iter_occurrences" not in str(e):
                    raise
                chunks = occurrences.iter_occurrences(graphs, query, **common)      # above max_rows: stream
            num_chunks = 0
            for occ in chunks:
                t = occ.table()
                cols = [t[c] for c in columns]
                for i in range(len(occ)):
                    w.writerow([row, name] + [int(c[i]) for c in cols])
                    row += 1
                per_graph += np.bincount(t["graph"], minlength=graphs.num_graphs)
                num_chunks += 1
            mode = "induced" if induced else "non-induced"
            print(f"{name}: {graphs.num_graphs} graphs, {graphs.num_nodes} nodes; query of {k} nodes, {len(edges)} edges, "
                  f"{mode}: {int(per_graph.sum())} occurrences in {num_chunks} chunk(s) ({occurrences.last_backend})")
            describe("  per graph", ["occurrences"], {"occurrences": per_graph})
    print(f"wrote {row} rows to {path}")
    return {"occurrences": path, "rows": row}


if __name__ == "__main__":
    main()
