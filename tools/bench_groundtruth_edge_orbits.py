#!/usr/bin/env python3
"""Exact edge orbit counts (the 69-column edge graphlet degree vector of ``groundtruth.edge_orbit_counts``) -- developer
tool.  On the Syn_1827-shaped set and on the COX2-shaped set x64:

  edge orbit, device   ``edge_orbit_counts_device``: upload, table, entry rows, kernels; the int64 [M, 69] result stays
                       on the device
  edge orbit, host     ``edge_orbit_counts(backend="host")`` with --threads threads
  node orbit, device   ``orbit_counts_device`` (73 columns): the same enumeration with k updates per subset, none of
                       which needs a row look-up
  canonical, device    ``canonical_counts_device`` on the same 30 classes: ONE update per subset -- the enumeration's
                       own cost.  The ratios edge / node orbit and edge / canonical price the tally and the look-ups
  non-induced          the device edge-orbit census plus the transform kernel

The device and host tables are compared bit for bit first; then min / median / max seconds of --repeat runs after one
warm-up.  The column sums are checked against |orbit| x the canonical column sums.  Nothing is asserted about speed."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from desco_amd import synthetic
from desco_amd.groundtruth import (canonical_counts_device, census_classes, edge_orbit_columns, edge_orbit_counts,
                                   edge_orbit_counts_device, edge_orbit_noninduced_matrix, orbit_counts_device)


def timed(fn, repeat):
    fn()
    times = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return (min(times), statistics.median(times), max(times)), out


def fmt(t):
    return "min {:.4f}  median {:.4f}  max {:.4f} s".format(*t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--host_only", action="store_true")
    ap.add_argument("--skip_host", action="store_true")
    ap.add_argument("--cox2_copies", type=int, default=64)
    args = ap.parse_args()
    census = [(k, list(e)) for n in (2, 3, 4, 5) for k, e in census_classes(n)]
    cols = edge_orbit_columns()
    for k in (2, 3, 4, 5):
        edge_orbit_noninduced_matrix(k)            # once per process: not part of any route's time
    sets = [("syn_1827", synthetic.WORKLOADS["syn_1827"]()),
            (f"cox2 x{args.cox2_copies}", synthetic.WORKLOADS["cox2"]().replicate(args.cox2_copies))]

    def dev(fn):
        def run():
            out = fn()
            torch.cuda.synchronize()
            return out
        return run

    for name, gs in sets:
        print(f"{name}: {gs.num_graphs} graphs, {gs.num_nodes} nodes, {gs.num_directed_edges // 2} edges", flush=True)
        host = None
        if not args.skip_host:
            t_host, host = timed(lambda: edge_orbit_counts(gs, backend="host", num_threads=args.threads), args.repeat)
            print(f"  edge orbit, host ({args.threads} threads)  {fmt(t_host)}   {float(host.sum()):.4e} cell updates",
                  flush=True)
        if args.host_only:
            continue
        first = dev(lambda: edge_orbit_counts_device(gs))()
        if host is not None:
            print(f"  device == host: {torch.equal(first.cpu().double(), host)}", flush=True)
        t_edge, eorb = timed(dev(lambda: edge_orbit_counts_device(gs)), args.repeat)
        print(f"  edge orbit, device            {fmt(t_edge)}   repeat == first: {torch.equal(eorb, first)}", flush=True)
        t_orb, _ = timed(dev(lambda: orbit_counts_device(gs)), args.repeat)
        print(f"  node orbit, device            {fmt(t_orb)}", flush=True)
        t_can, can = timed(dev(lambda: canonical_counts_device(gs, census)), args.repeat)
        print(f"  canonical, device (30 cls)    {fmt(t_can)}", flush=True)
        t_non, _ = timed(dev(lambda: edge_orbit_counts_device(gs, induced=False)), args.repeat)
        print(f"  edge orbit non-induced, device {fmt(t_non)}", flush=True)
        print(f"  edge / node orbit (median)  {t_edge[1] / t_orb[1]:.2f}x   edge / canonical  {t_edge[1] / t_can[1]:.2f}x"
              + ("" if host is None else f"   host / device {t_host[1] / t_edge[1]:.2f}x"))
        sums, csums = eorb.sum(0).cpu(), can.sum(0).cpu()
        ok = all(int(sums[j]) == len(mem) * int(csums[qi]) for j, (qi, _, mem) in enumerate(cols))
        print(f"  column sums = |orbit| x canonical sums: {ok}", flush=True)


if __name__ == "__main__":
    main()
