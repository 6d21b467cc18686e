#!/usr/bin/env python3
"""Listing occurrences: the device lister (csrc/occurrences_dev.hip) leg by leg against the host twin at 16 threads --
developer tool.  Two shapes, the Syn_1827-shaped set and the COX2-shaped set x64; queries triangle, 4-cycle, 5-path and
the 5-node house; both modes.  The outputs are first compared bit for bit, then every leg is timed --repeat times and
min / median / max are printed in milliseconds:

  count     the count pass alone (the matcher's existing launches, graphs already uploaded): the yardstick
  emit      the emit launches alone (ptr known, rows allocated)
  order     the ordering sorts alone
  device    the whole list_occurrences_device call, uploads included, by HIP events
  host      the host twin (count pass, scan, listing, ordering) on --threads threads

Nothing is asserted about speed."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from desco_amd import _lib, occurrences, synthetic
from desco_amd import groundtruth as gt

QUERIES = {
    "triangle": (3, [(0, 1), (1, 2), (0, 2)]),
    "C4": (4, [(0, 1), (1, 2), (2, 3), (3, 0)]),
    "P5": (5, [(0, 1), (1, 2), (2, 3), (3, 4)]),
    "house": (5, [(0, 1), (1, 2), (2, 3), (3, 0), (0, 4), (1, 4)]),
}


def event_ms(fn, repeat):
    ts = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts, out


def wall_ms(fn, repeat):
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts, out


def fmt(ts):
    return f"{min(ts):9.2f} {statistics.median(ts):9.2f} {max(ts):9.2f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--syn_graphs", type=int, default=1827)
    ap.add_argument("--cox2_times", type=int, default=64)
    ap.add_argument("--max_rows", type=int, default=1 << 27, help="skip a (shape, query, mode) with more rows")
    ap.add_argument("--queries", nargs="+", default=list(QUERIES))
    ap.add_argument("--host_only", action="store_true")
    args = ap.parse_args()
    shapes = [(f"syn_1827[:{args.syn_graphs}]", synthetic.syn_1827_shaped(args.syn_graphs)),
              (f"cox2 x{args.cox2_times}", synthetic.cox2_shaped().replicate(args.cox2_times))]
    print(f"{'':44s}{'min':>9s} {'median':>9s} {'max':>9s}   (ms, {args.repeat} runs)")
    for sname, gs in shapes:
        print(f"{sname}: {gs.num_graphs} graphs, {gs.num_nodes} nodes, {gs.num_directed_edges // 2} edges")
        for qname in args.queries:
            q = QUERIES[qname]
            for induced in (True, False):
                tag = f"  {qname:9s}{'induced' if induced else 'non-induced':12s}"
                total = int(gt.canonical_counts_match(gs, [q], backend="host", num_threads=args.threads,
                                                      induced=induced).sum())
                if total > args.max_rows:
                    print(f"{tag} {total} rows: above --max_rows, skipped")
                    continue
                host = lambda: occurrences.list_occurrences(gs, q, induced=induced, backend="host",     # noqa: E731
                                                            num_threads=args.threads, max_rows=args.max_rows)
                want = host()
                if args.host_only:
                    print(f"{tag} {total:>11d} rows  host   {fmt(wall_ms(host, args.repeat)[0])}")
                    continue
                dev = lambda: occurrences.list_occurrences_device(gs, q, induced=induced,                 # noqa: E731
                                                                  max_rows=args.max_rows)
                got = dev().cpu()
                same = np.array_equal(got.rows, want.rows) and np.array_equal(got.ptr, want.ptr)
                print(f"{tag} {total:>11d} rows  identical to the host twin: {same}")
                if not same:
                    continue
                s = occurrences._Device(gs, q, induced, "cuda", None)
                L, stream = _lib.lib(), torch.cuda.current_stream()

                def count():
                    gt._sliced(s.d.E, s.slice_entries, stream, lambda e0, e1: _lib.check(
                        L.desco_canonical_counts_match_mode_dev(*s.head, e0, e1, s.counts.data_ptr(), stream.cuda_stream),
                        "desco_canonical_counts_match_mode_dev"))
                rows = torch.empty((total, q[0]), dtype=torch.int32, device="cuda")
                legs = [("count", event_ms(count, args.repeat)[0]),
                        ("emit", event_ms(lambda: s.emit(0, s.d.E, 0, rows), args.repeat)[0]),
                        ("order", event_ms(lambda: occurrences.sort_segments_device(rows), args.repeat)[0]),
                        ("device", event_ms(dev, args.repeat)[0]), ("host", wall_ms(host, args.repeat)[0])]
                for leg, ts in legs:
                    print(f"      {leg:38s}{fmt(ts)}")
                del rows, s
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
