#!/usr/bin/env python3
"""Generate partition_homo_golden.json by running the REFERENCE's own get_neigh_canonical (data.py:353-372, which
calls k_neigh_canonical data.py:341-350) on the graphs of partition_golden.json plus the 5-cycle 3-5-0-1-2-3.

Run ONLY where the reference is available (read-only), next to make_golden.py:
    cd tests/golden && python -B make_partition_homo_golden.py
The output is data: per depth and graph, the node set of every node's restricted neighborhood, the anchor (the one node
whose node_feature is 1) and the number of its edges.  No reference source is copied.
"""
import json
import os

import networkx as nx

import _ref_import

HERE = os.path.dirname(os.path.abspath(__file__))
DEPTHS = (0, 1, 2, 4)
FIVE_CYCLE = {"name": "cycle5_3_5_0_1_2", "n": 6, "edges": [[3, 5], [5, 0], [0, 1], [1, 2], [2, 3]]}


def main():
    ref_data = _ref_import.load()[0]
    with open(os.path.join(HERE, "partition_golden.json")) as f:
        base = json.load(f)["graphs"]
    graphs = [FIVE_CYCLE] + [{"name": g["name"], "n": g["n"], "edges": g["edges"]} for g in base]
    out = {"depths": list(DEPTHS), "graphs": []}
    for g in graphs:
        G = nx.Graph()
        G.add_nodes_from(range(g["n"]))
        G.add_edges_from(tuple(e) for e in g["edges"])
        per_depth = {}
        for depth in DEPTHS:
            nodes, num_edges = [], []
            for v in G.nodes:
                ng = ref_data.get_neigh_canonical(G, v, depth)
                anchors = [int(u) for u in ng.nodes if float(ng.nodes[u]["node_feature"][0]) == 1.0]
                assert anchors == [int(v)]
                nodes.append(sorted(int(u) for u in ng.nodes))
                num_edges.append(int(ng.number_of_edges()))
            per_depth[str(depth)] = {"nodes": nodes, "num_edges": num_edges}
        out["graphs"].append({"name": g["name"], "n": g["n"], "edges": g["edges"], "neighs": per_depth})
    with open(os.path.join(HERE, "partition_homo_golden.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))


if __name__ == "__main__":
    main()
