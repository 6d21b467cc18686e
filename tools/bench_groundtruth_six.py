#!/usr/bin/env python3
"""Exact counts of 6-node queries: the device walk at depth six (``groundtruth.canonical_counts6_device``,
csrc/groundtruth6_dev.hip) against its host twin (``canonical_counts(backend="host")``, the OpenMP enumerator of the
same commit) -- developer tool, and the measurement behind ``groundtruth.AUTO_USES_DEVICE6``.  On the COX2-shaped set
x64 and on the Syn_1827-shaped set:

  induced      all 112 connected 6-node classes as queries (one walk on either side)
  non-induced  ONE 6-node column (the 6-path), which needs the census of all 112 classes and the int64 transform

Outputs are compared bit for bit first; then min / median / max seconds of --repeat runs after one warm-up.  The device
call is timed by HIP events around the whole call: uploads, the class table, every slice's launch and wait.  The host
twin runs on --threads threads.  A host call on the whole Syn set takes minutes, so the tool times the largest prefix of
its graphs (doubling from --syn_start) whose host call stays within --host_cap seconds, and names it.  Rates are
connected 6-node subsets per second (the sum of the induced result).  Nothing is asserted about speed.

Variants tried while the kernel was written (table in global memory or as a byte copy in LDS under persistent
workgroups; the tally with and without the per-loop run) are not in the tree: DESIGN.md 4.6 has their figures, taken
with this tool."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from desco_amd import synthetic
from desco_amd.groundtruth import canonical_counts, canonical_counts6_device, census_classes

PATH6 = (6, [(i, i + 1) for i in range(5)])


def timed_host(fn, repeat):
    fn()
    times = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return (min(times), statistics.median(times), max(times)), out


def timed_device(fn, repeat):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeat):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop) / 1e3)
    return (min(times), statistics.median(times), max(times)), out


def fmt(t):
    return "min {:.4f}  median {:.4f}  max {:.4f} s".format(*t)


def host_prefix(gs, queries, threads, start, cap):
    """the largest prefix of graphs (doubling from ``start``) whose host call stays within ``cap`` seconds"""
    g, best = min(start, gs.num_graphs), None
    while True:
        t0 = time.perf_counter()
        canonical_counts(gs.subset(0, g), queries, backend="host", num_threads=threads)
        dt = time.perf_counter() - t0
        if dt > cap and best is not None:
            return best
        best = g
        if g == gs.num_graphs or 2.2 * dt > cap:        # (subsets grow about in step with the graphs)
            return best
        g = min(2 * g, gs.num_graphs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--skip_host", action="store_true", help="device only (no comparison); --syn_graphs names the prefix")
    ap.add_argument("--cox2_copies", type=int, default=64)
    ap.add_argument("--host_cap", type=float, default=6.0, help="seconds one host call on the Syn prefix may take")
    ap.add_argument("--syn_start", type=int, default=32)
    ap.add_argument("--syn_graphs", type=int, default=0, help="fix the Syn prefix instead of searching it")
    args = ap.parse_args()
    six = [(k, list(e)) for k, e in census_classes(6)]
    syn = synthetic.WORKLOADS["syn_1827"]()
    if args.syn_graphs:
        g = min(args.syn_graphs, syn.num_graphs)
    elif args.skip_host:
        g = syn.num_graphs
    else:
        g = host_prefix(syn, six, args.threads, args.syn_start, args.host_cap)
    sets = [(f"cox2 x{args.cox2_copies}", synthetic.WORKLOADS["cox2"]().replicate(args.cox2_copies)),
            (f"syn_1827, first {g} of {syn.num_graphs} graphs (host cap {args.host_cap:g} s)", syn.subset(0, g))]
    verdict = []
    for name, gs in sets:
        print(f"{name}: {gs.num_graphs} graphs, {gs.num_nodes} nodes, {gs.num_directed_edges // 2} edges", flush=True)
        for label, queries, induced in (("induced, 112 classes", six, True), ("non-induced, 1 column", [PATH6], False)):
            t_dev, dev = timed_device(lambda: canonical_counts6_device(gs, queries, induced=induced), args.repeat)
            if induced:
                subsets = int(dev.sum())
                print(f"  {subsets} connected 6-node subsets", flush=True)
            print(f"  {label:24s} device     {fmt(t_dev)}   {subsets / t_dev[1]:.3e} subsets/s", flush=True)
            if args.skip_host:
                continue
            t_host, host = timed_host(lambda: canonical_counts(gs, queries, backend="host", num_threads=args.threads,
                                                               induced=induced), args.repeat)
            same = torch.equal(dev.cpu().double(), host)
            print(f"  {label:24s} host ({args.threads:2d})  {fmt(t_host)}   {subsets / t_host[1]:.3e} subsets/s", flush=True)
            print(f"  {label:24s} device == host: {same}   host / device (median) {t_host[1] / t_dev[1]:.2f}x",
                  flush=True)
            verdict.append(same and t_dev[1] < t_host[1])
    if verdict:
        print("device ahead of the host twin, bit for bit, on every line:", all(verdict))


if __name__ == "__main__":
    main()
