#!/usr/bin/env python3
"""Ground truth of LARGE queries (7..12 nodes): the device matcher (csrc/groundtruth_match_dev.hip) against the host
matcher at 16 threads -- developer tool.  Two legs: the COX2-shaped set with path, ring and fused-ring queries of
7..12 nodes, and a slice of the Syn_1827-shaped set with 7-node queries.  Prints seconds per leg (device: upload,
plan and download included; median of --repeat runs after one warm-up); the results are compared bit for bit.
Nothing is asserted about speed."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import networkx as nx
import torch

from desco_amd import synthetic
from desco_amd.groundtruth import canonical_counts_match, canonical_counts_match_device, match_plan


def fused_rings(rings):
    """`rings` 6-rings fused in a row along shared edges (2: 10 nodes, the naphthalene skeleton)."""
    g = nx.cycle_graph(6)
    a, b = 5, 0
    for _ in range(rings - 1):
        n = g.number_of_nodes()
        nx.add_path(g, [b, n, n + 1, n + 2, n + 3, a])
        a, b = n + 2, n + 1
    return g


def legs(syn_graphs):
    cox2 = synthetic.WORKLOADS["cox2"]()
    q_cox2 = {"P7": nx.path_graph(7), "P9": nx.path_graph(9), "P12": nx.path_graph(12), "C7": nx.cycle_graph(7),
              "C8": nx.cycle_graph(8), "C10": nx.cycle_graph(10), "C12": nx.cycle_graph(12),
              "fused6x2 (10)": fused_rings(2)}
    syn = synthetic.WORKLOADS["syn_1827"]().subset(300, 300 + syn_graphs)
    q_syn = {"P7": nx.path_graph(7), "C7": nx.cycle_graph(7), "K1,6": nx.star_graph(6),
             "tree7": nx.balanced_tree(2, 2), "tri-bridge-C4": nx.Graph([(0, 1), (1, 2), (2, 0), (2, 3), (3, 4), (4, 5),
                                                                          (5, 6), (6, 3)])}
    return [("cox2", cox2, q_cox2), (f"syn_1827[300:{300 + syn_graphs}]", syn, q_syn)]


def timed(fn, repeat):
    fn()
    times = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--syn_graphs", type=int, default=120, help="graphs of the Syn_1827-shaped slice")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--host_only", action="store_true")
    args = ap.parse_args()
    for name, gs, qs in legs(args.syn_graphs):
        queries = list(qs.values())
        anchors = int(match_plan(queries)[1])
        t_host, host = timed(lambda: canonical_counts_match(gs, queries, backend="host", num_threads=args.threads),
                             args.repeat)
        print(f"{name}: {gs.num_graphs} graphs, {gs.num_nodes} nodes, {gs.num_directed_edges // 2} edges; "
              f"{len(queries)} queries ({', '.join(qs)}), {anchors} anchors, {float(host.sum()):.3e} matched subgraphs")
        print(f"  host ({args.threads} threads): {t_host:.4f} s")
        if args.host_only:
            continue

        def dev():
            out = canonical_counts_match_device(gs, queries).cpu()
            torch.cuda.synchronize()
            return out
        t_dev, got = timed(dev, args.repeat)
        print(f"  device: {t_dev:.4f} s   host / device {t_host / t_dev:.2f}x   identical: "
              f"{torch.equal(got.double(), host)}")


if __name__ == "__main__":
    main()
