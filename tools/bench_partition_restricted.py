#!/usr/bin/env python3
"""Restricted neighborhoods (developer tool): the device builder's second mode (build_partition_device(restricted=True):
the homogeneous ablation's k_neigh_canonical neighborhoods) against its first (the ball / id filter / component of
get_neigh_hetero) on the same sets, same card, same build.

    tools/bench_partition_restricted.py [--repeats 7] [--workloads syn_1827:1,cox2:64] [--depth 4] [--json FILE]

A build is a host clock around ``build_partition_device`` (uploads of the CSR, count pass, scan, the read-back of the four
totals, fill pass) ending in ``torch.cuda.synchronize()``, after a warm-up; median / min / max of the repeats.  The
restricted result is compared bit for bit with the host builder's first (``--no-check`` skips that), and the neighborhood
/ row / edge counts of both definitions are printed."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from desco_amd import synthetic
from desco_amd.partition import build_partition, build_partition_device


def mmm(v):
    return {"min": round(min(v), 5), "median": round(statistics.median(v), 5), "max": round(max(v), 5), "n": len(v)}


def timed(gs, depth, device, restricted, repeats):
    build_partition_device(gs, depth, device, restricted=restricted)            # warm-up
    torch.cuda.synchronize(device)
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        p = build_partition_device(gs, depth, device, restricted=restricted)
        torch.cuda.synchronize(device)
        out.append(time.perf_counter() - t0)
    return p, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--workloads", default="syn_1827:1,cox2:64")
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    result = {}
    for item in args.workloads.split(","):
        wl, rep = item.split(":")
        gs = synthetic.WORKLOADS[wl]().replicate(int(rep))
        pr, tr = timed(gs, args.depth, device, True, args.repeats)
        pb, tb = timed(gs, args.depth, device, False, args.repeats)
        if not args.no_check:
            host = build_partition(gs, args.depth, restricted=True)
            for f in ("neigh_index", "indicator", "count_ptr", "count_orig", "vrowptr", "vcol"):
                assert np.array_equal(getattr(pr, f), getattr(host, f)), f
        r = {"graphs": gs.num_graphs, "nodes": gs.num_nodes, "directed_edges": gs.num_directed_edges, "depth": args.depth,
             "restricted": {"build_s": mmm(tr), "neighborhoods": pr.num_neigh, "rows": pr.num_rows, "edges": pr.num_edges},
             "ball": {"build_s": mmm(tb), "neighborhoods": pb.num_neigh, "rows": pb.num_rows, "edges": pb.num_edges}}
        result[item] = r
        print(f"{item}: {gs.num_graphs} graphs, {gs.num_nodes} nodes, depth {args.depth}")
        for k in ("restricted", "ball"):
            print(f"  {k:10s} build {r[k]['build_s']['median'] * 1e3:8.2f} ms (min {r[k]['build_s']['min'] * 1e3:.2f}, max "
                  f"{r[k]['build_s']['max'] * 1e3:.2f}, n {args.repeats})  {r[k]['neighborhoods']} neighborhoods, "
                  f"{r[k]['rows']} rows, {r[k]['edges']} edges", flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
