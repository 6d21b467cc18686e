#!/usr/bin/env python3
"""Time the data-set statistics of all canonical neighborhoods at depth 4 on the Syn_1827-shaped set and on the
COX2-shaped set replicated 64 times: the device kernel against the host twin, and networkx for scale.

Per workload:
  1. the partition is built on the GPU and stays there; the node sets and their word buckets are assembled on the device;
  2. one device pass and one host pass (16 threads) are compared BIT FOR BIT (integers and the fp64 field) -- a
     difference ends the run;
  3. the device is timed with HIP events around the statistics launches alone (min / median / max of 5);
  4. the host twin is timed on 16 threads (min / median / max of 5; fewer when one pass takes more than --host_budget
     seconds, the number of passes is reported);
  5. networkx (connected_components, density, average_clustering, average_shortest_path_length, diameter: what the
     reference's script calls) is timed on a FIXED sample of 200 neighborhoods, evenly spaced over the set, and
     multiplied by B / 200.  That figure is an EXTRAPOLATION -- linear in the number of neighborhoods, although the
     cost per neighborhood is not uniform -- and is labelled so.
One JSON line per workload.  There is no time gate.

    python tools/bench_neigh_stats.py [--workloads syn_1827 cox2x64] [--reps 5] [--threads 16]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def spread(xs):
    xs = sorted(xs)
    return {"min": xs[0], "median": float(np.median(xs)), "max": xs[-1], "n": len(xs)}


def networkx_sample(graphs, set_ptr, set_nodes, sample):
    """seconds networkx needs for the neighborhoods ``sample`` (graph construction not counted)"""
    import networkx as nx
    total = 0.0
    for b in sample:
        mem = set_nodes[set_ptr[b]:set_ptr[b + 1]]
        inside = set(int(v) for v in mem)
        H = nx.Graph()
        H.add_nodes_from(sorted(inside))
        for v in mem:
            for w in graphs.col[graphs.rowptr[v]:graphs.rowptr[v + 1]]:
                if int(w) in inside and v < w:
                    H.add_edge(int(v), int(w))
        t = time.perf_counter()
        C = H.subgraph(max(nx.connected_components(H), key=len))
        nx.density(C), nx.average_clustering(C), nx.average_shortest_path_length(C), nx.diameter(C)
        total += time.perf_counter() - t
    return total


def run(name, graphs, args):
    import torch
    from desco_amd import analysis
    from desco_amd.partition import build_partition_device
    dev = torch.device("cuda")
    part = build_partition_device(graphs, args.depth)
    set_ptr, set_nodes = analysis.neighborhood_sets_device(part, graphs)
    launches, over = analysis.device_buckets(set_ptr)
    assert over.numel() == 0, f"{name}: {over.numel()} neighborhoods above {analysis.DEVICE_SET_LIMIT} members"
    rowptr_d, col_d = torch.from_numpy(graphs.rowptr).to(dev), torch.from_numpy(graphs.col).to(dev)
    S = part.num_neigh
    out_i = torch.zeros((S, 6), dtype=torch.int64, device=dev)
    out_f = torch.zeros(S, dtype=torch.float64, device=dev)

    def device_pass():
        for w, ids in launches:
            analysis.subgraph_stats_launch(rowptr_d, col_d, graphs.num_nodes, set_ptr, set_nodes, ids, w, out_i, out_f)

    device_pass()
    torch.cuda.synchronize()
    sp, sn = set_ptr.cpu().numpy(), set_nodes.cpu().numpy()
    host_times = []
    t = time.perf_counter()
    h_i, h_f = analysis._stats_host(graphs, sp, sn, args.threads)
    host_times.append(time.perf_counter() - t)
    d_i, d_f = out_i.cpu().numpy(), out_f.cpu().numpy()
    if not (np.array_equal(d_i, h_i) and d_f.tobytes() == h_f.tobytes()):
        bad = np.nonzero((d_i != h_i).any(axis=1) | (d_f.view(np.int64) != h_f.view(np.int64)))[0]
        raise SystemExit(f"{name}: device and host differ in {len(bad)} of {S} rows, first {bad[:5].tolist()}")
    dev_times = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        device_pass()
        e1.record()
        e1.synchronize()
        dev_times.append(e0.elapsed_time(e1) * 1e-3)
    while len(host_times) < args.reps and host_times[0] <= args.host_budget:
        t = time.perf_counter()
        analysis._stats_host(graphs, sp, sn, args.threads)
        host_times.append(time.perf_counter() - t)
    sample = np.unique(np.linspace(0, S - 1, min(200, S)).astype(np.int64))
    nx_s = networkx_sample(graphs, sp, sn, sample) if not args.no_networkx else float("nan")
    sizes = np.diff(sp)
    print(json.dumps({
        "workload": name, "depth": args.depth, "neighborhoods": int(S), "set_members": int(sp[-1]),
        "largest_set": int(sizes.max()), "launches": [[w, int(ids.numel())] for w, ids in launches],
        "bit_identical_to_host": True,
        "device_seconds": spread(dev_times), "host_threads": args.threads, "host_seconds": spread(host_times),
        "networkx_sample_neighborhoods": int(len(sample)), "networkx_sample_seconds": nx_s,
        "networkx_seconds_EXTRAPOLATED_linearly_from_the_sample": nx_s * S / len(sample),
    }), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--workloads", nargs="+", default=["cox2x64", "syn_1827"], choices=["cox2x64", "syn_1827"])
    p.add_argument("--depth", type=int, default=4)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--threads", type=int, default=16)
    p.add_argument("--host_budget", type=float, default=20.0,
                   help="repeat the host pass only when one pass stays below this many seconds")
    p.add_argument("--no_networkx", action="store_true")
    args = p.parse_args()
    import torch
    from desco_amd import synthetic
    if not torch.cuda.is_available():
        raise SystemExit("bench_neigh_stats needs the MI355X: the device kernel has no CPU fallback")
    for name in args.workloads:
        graphs = synthetic.cox2_shaped().replicate(64) if name == "cox2x64" else synthetic.syn_1827_shaped()
        run(name, graphs, args)


if __name__ == "__main__":
    main()
