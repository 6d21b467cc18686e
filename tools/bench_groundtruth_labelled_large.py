#!/usr/bin/env python3
"""Ground truth of LABELLED large queries (--use_node_feature, 7..10 nodes): networkx VF2 with node_match (what
``canonical_counts_labelled`` did for such queries before the labelled matcher), the host labelled matcher at 16
threads and the device labelled matcher (csrc/groundtruth_match_dev.hip) -- developer tool.  Input: the COX2-shaped
set with two seeded one-hot labels and the F = 2 expansions of P7, C8 and the 10-node fused-ring query (128 + 256 +
1024 labelled queries).  Prints the class count, the record count, launched versus live waves and seconds per backend
(label ids, classes, plan, upload and download included; median of --repeat runs after one warm-up); the results are compared bit
for bit.  VF2 runs once, on the first --vf2_graphs graphs and the first --vf2_queries queries of every expansion, and
its time is also given scaled to the whole input.  Nothing is asserted about speed."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import networkx as nx
import numpy as np
import torch

from desco_amd import groundtruth as GT
from desco_amd import synthetic
from desco_amd.data import add_node_feat_to_networkx
from desco_amd.graphs import GraphSet
from bench_groundtruth_large import fused_rings, timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=0, help="graphs of the COX2-shaped set (0: all)")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--vf2_graphs", type=int, default=8)
    ap.add_argument("--vf2_queries", type=int, default=8, help="labelled copies per expansion in the VF2 run")
    ap.add_argument("--host_only", action="store_true")
    args = ap.parse_args()
    plain = synthetic.WORKLOADS["cox2"]()
    if args.graphs:
        plain = plain.subset(0, args.graphs)
    graphs = plain.edge_lists()
    rng = np.random.default_rng(11)
    gs = GraphSet.from_edge_lists(graphs, node_feat=[np.eye(2, dtype=np.float32)[rng.integers(2, size=n)]
                                                      for n, _ in graphs])
    eye = np.eye(2).tolist()
    blocks = {"P7": nx.path_graph(7), "C8": nx.cycle_graph(8), "fused6x2 (10)": fused_rings(2)}
    expansions = [add_node_feat_to_networkx(q, eye, "feat") for q in blocks.values()]
    queries = [g for ex in expansions for g in ex]
    t0 = time.perf_counter()
    lab = GT._Labelled(gs, queries, "feat")
    plan, _ = GT._match_plan_labelled(lab)
    t_prep = time.perf_counter() - t0
    launched, live = GT.labelled_match_waves(gs, lab, plan)
    E = int(gs.col.shape[0])
    print(f"cox2: {gs.num_graphs} graphs, {gs.num_nodes} nodes, {E // 2} edges, 2 labels; {len(queries)} labelled queries "
          f"(F = 2 expansions of {', '.join(blocks)}), {int(plan[0])} classes, {int(plan[1])} records in {int(plan[2])} "
          f"buckets (largest {int(plan[3])})")
    print(f"  device waves: launched {launched} = {E} entries x {int(plan[3])}, live {live} "
          f"({100.0 * live / max(launched, 1):.1f}%); entries x records would be {E * int(plan[1])}")
    print(f"  label ids, classes and plan (host, part of both times below): {t_prep:.4f} s")

    sub = gs.subset(0, min(args.vf2_graphs, gs.num_graphs))
    sub_q = [g for ex in expansions for g in ex[:args.vf2_queries]]
    t0 = time.perf_counter()
    vf2 = GT.canonical_counts_labelled(sub, sub_q, backend="vf2")
    t_vf2 = time.perf_counter() - t0
    scale = (gs.num_nodes / sub.num_nodes) * (len(queries) / len(sub_q))
    print(f"  vf2 (first {sub.num_graphs} graphs, first {args.vf2_queries} copies of each expansion = {len(sub_q)} "
          f"queries): {t_vf2:.3f} s; scaled by nodes x queries to the whole input: {t_vf2 * scale:.0f} s")
    same = torch.equal(GT.canonical_counts_match_labelled(sub, sub_q, backend="host", num_threads=args.threads), vf2)
    print(f"  host matcher on the VF2 subset identical to VF2: {same}")

    t_host, host = timed(lambda: GT.canonical_counts_match_labelled(gs, queries, backend="host",
                                                                    num_threads=args.threads), args.repeat)
    print(f"  host ({args.threads} threads): {t_host:.4f} s   {float(host.sum()):.3e} matched labelled subgraphs")
    if args.host_only:
        return

    t_dev, got = timed(lambda: GT.canonical_counts_match_labelled(gs, queries, backend="device"), args.repeat)
    print(f"  device (the same CPU result: expanded and converted on the device, downloaded): {t_dev:.4f} s   "
          f"host / device {t_host / t_dev:.2f}x   identical: {torch.equal(got, host)}")

    def on_device():
        out = GT.canonical_counts_match_labelled_device(gs, queries)
        torch.cuda.synchronize()
        return out
    t_on, got = timed(on_device, args.repeat)
    print(f"  device, result left on the device ([N, Q] int64): {t_on:.4f} s   identical: "
          f"{torch.equal(got.cpu().double(), host)}")


if __name__ == "__main__":
    main()
