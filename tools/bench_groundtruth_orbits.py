#!/usr/bin/env python3
"""Exact orbit counts (the 73-column graphlet degree vector of ``groundtruth.orbit_counts``) -- developer tool.  On the
Syn_1827-shaped set and on the COX2-shaped set x64:

  orbit, device      ``orbit_counts_device``: upload, table, kernels; the int64 [N, 73] result stays on the device
  canonical, device  ``canonical_counts_device`` on the same 30 classes (the connected graphs of 2..5 nodes): the same
                     enumeration with ONE update per subset where the orbit kernel makes k -- the baseline, so the
                     ratio orbit / canonical prices the tally and cannot be below 1
  orbit, host        ``orbit_counts(backend="host")`` with --threads threads
  non-induced        the device orbit census plus the transform kernel

Prints min / median / max seconds of --repeat runs after one warm-up and compares device and host bit for bit, and the
orbit column sums against |orbit| x the canonical column sums.  Nothing is asserted about speed."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from desco_amd import synthetic
from desco_amd.groundtruth import (canonical_counts_device, census_classes, orbit_columns, orbit_counts,
                                   orbit_counts_device, orbit_noninduced_matrix)


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
    cols = orbit_columns()
    for k in (2, 3, 4, 5):
        orbit_noninduced_matrix(k)                 # once per process: not part of any route's time
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
            t_host, host = timed(lambda: orbit_counts(gs, backend="host", num_threads=args.threads), args.repeat)
            print(f"  orbit, host ({args.threads} threads)   {fmt(t_host)}   {float(host.sum()):.4e} cell updates", flush=True)
        if args.host_only:
            continue
        t_orb, orb = timed(dev(lambda: orbit_counts_device(gs)), args.repeat)
        print(f"  orbit, device               {fmt(t_orb)}", flush=True)
        t_can, can = timed(dev(lambda: canonical_counts_device(gs, census)), args.repeat)
        print(f"  canonical, device (30 cls)  {fmt(t_can)}", flush=True)
        t_non, _ = timed(dev(lambda: orbit_counts_device(gs, induced=False)), args.repeat)
        print(f"  orbit non-induced, device   {fmt(t_non)}", flush=True)
        print(f"  orbit / canonical (median)  {t_orb[1] / t_can[1]:.2f}x"
              + ("" if host is None else f"   host / device {t_host[1] / t_orb[1]:.2f}x"))
        sums, csums = orb.sum(0).cpu(), can.sum(0).cpu()
        ok = all(int(sums[j]) == len(mem) * int(csums[qi]) for j, (qi, _, mem) in enumerate(cols))
        print(f"  column sums = |orbit| x canonical sums: {ok}"
              + ("" if host is None else f"   device == host: {torch.equal(orb.cpu().double(), host)}"), flush=True)


if __name__ == "__main__":
    main()
