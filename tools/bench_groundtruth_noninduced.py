#!/usr/bin/env python3
"""NON-INDUCED ground truth: the census route against the matcher route against the host -- developer tool.  On the
two graph sets of tools/bench_groundtruth_large.py (the COX2-shaped set, a slice of the Syn_1827-shaped set):

  small   the 29 standard queries (3..5 nodes): host census (ESU + numpy int64 transform), host matcher, device
          census + transform kernel, device matcher; the induced ESU call beside them as what the census costs
  large   that tool's queries of 7..12 nodes: host matcher against device matcher, induced beside non-induced.  The
          dense Syn_1827-shaped graphs hold 2.8e10 non-induced occurrences of the five 7-node queries in 120 graphs
          (two minutes on 8 host threads), so this part runs on the first --syn_large_graphs graphs of the slice

Prints seconds per route (device: upload, plan and download included; median of --repeat runs after one warm-up); the
routes are compared bit for bit.  Nothing is asserted about speed."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from bench_groundtruth_large import legs, timed
from desco_amd.data import STANDARD_QUERY_IDS, graph_atlas_plus
from desco_amd.groundtruth import (canonical_counts, canonical_counts_device, canonical_counts_match,
                                   canonical_counts_match_device, noninduced_matrix)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--syn_graphs", type=int, default=120, help="graphs of the Syn_1827-shaped slice")
    ap.add_argument("--syn_large_graphs", type=int, default=8,
                    help="graphs of that slice the 7-node queries are counted in")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--host_only", action="store_true")
    ap.add_argument("--skip_large", action="store_true", help="leave the 7..12-node queries out")
    args = ap.parse_args()
    std = [graph_atlas_plus(i) for i in STANDARD_QUERY_IDS]
    for k in (3, 4, 5):
        noninduced_matrix(k)                       # once per process: not part of any route's time
    nt = args.threads

    def dev(fn):
        def run():
            out = fn().cpu()
            torch.cuda.synchronize()
            return out.double()
        return run

    for name, gs, qs in legs(args.syn_graphs):
        print(f"{name}: {gs.num_graphs} graphs, {gs.num_nodes} nodes, {gs.num_directed_edges // 2} edges")
        routes = [("induced, host ESU", lambda: canonical_counts(gs, std, nt, "host")),
                  ("host census + numpy", lambda: canonical_counts(gs, std, nt, "host", induced=False)),
                  ("host matcher", lambda: canonical_counts_match(gs, std, "host", nt, induced=False))]
        if not args.host_only:
            routes += [("induced, device ESU", dev(lambda: canonical_counts_device(gs, std))),
                       ("device census + transform", dev(lambda: canonical_counts_device(gs, std, induced=False))),
                       ("device matcher", dev(lambda: canonical_counts_match_device(gs, std, induced=False)))]
        want = None
        for label, fn in routes:
            t, out = timed(fn, args.repeat)
            note = ""
            if not label.startswith("induced"):
                want = out if want is None else want
                note = f"   identical: {torch.equal(out, want)}"
            print(f"  small ({len(std)} queries)  {label:28s} {t:9.4f} s   {float(out.sum()):.3e} occurrences{note}")
        if args.skip_large:
            continue
        queries = list(qs.values())
        if name.startswith("syn") and gs.num_graphs > args.syn_large_graphs:
            gs = gs.subset(0, args.syn_large_graphs)
            print(f"  large: the first {gs.num_graphs} graphs, {gs.num_nodes} nodes, {gs.num_directed_edges // 2} edges")
        for induced in (True, False):
            kind = "induced" if induced else "non-induced"
            t_host, host = timed(lambda: canonical_counts_match(gs, queries, "host", nt, induced=induced), args.repeat)
            print(f"  large ({', '.join(qs)})  {kind}: host matcher {t_host:.4f} s   {float(host.sum()):.3e} occurrences")
            if not args.host_only:
                t_dev, got = timed(dev(lambda: canonical_counts_match_device(gs, queries, induced=induced)), args.repeat)
                print(f"      device matcher {t_dev:.4f} s   host / device {t_host / t_dev:.2f}x   identical: "
                      f"{torch.equal(got, host)}")


if __name__ == "__main__":
    main()
