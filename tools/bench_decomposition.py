"""Times the k-core / k-truss decomposition on one MI355X against its host twin.

Workloads: Syn_1827-shaped (1827 graphs) and COX2-shaped x64 (29 888 molecules; they have NO triangles, every truss
number is 2, so that shape times the set-up and the core peel only).  Per workload, only after core, truss, support and
node_truss of the device have been compared with the twin's bit for bit: ``decompose_device`` (HIP events around the
call: uploads, the edge-row map, the launches, node_truss) against the twin on --threads threads (host clock), min /
median / max of --repeat runs after a warm-up; the launches alone (HIP events around the entry point, arrays resident)
with one wave and with four waves per graph for the graphs below ``WAVE_WORDS``, by workspace range; and networkx
(core_number, and k_truss for every k) on a 50-graph sample, extrapolated -- an order of magnitude, no more.  One JSON
line per measurement.

    python tools/bench_decomposition.py [--repeat 5] [--threads 16]
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIELDS = ("core", "truss", "support", "node_truss")


def summary(xs):
    xs = sorted(xs)
    return {"min_s": xs[0], "median_s": xs[len(xs) // 2], "max_s": xs[-1], "runs": len(xs)}


def launches_alone(g, bounds, repeat):
    """Seconds of the entry point alone, the arrays resident: one launch per (ids, max_words) of ``bounds``."""
    import torch
    from desco_amd import _lib, groundtruth as gt
    dev = torch.device("cuda")
    G, N, E = g.num_graphs, g.num_nodes, g.num_directed_edges
    graph_ptr, rowptr, col = gt._put(g.graph_ptr, np.int64, dev), gt._put(g.rowptr, np.int64, dev), gt._put(g.col, np.int32, dev)
    entry_row, M = gt._entry_rows_device(SimpleNamespace(_keep=(graph_ptr, rowptr, col), E=E, N=N, dev=dev))
    core = torch.empty(N, dtype=torch.int32, device=dev)
    truss, support = torch.empty(M, dtype=torch.int32, device=dev), torch.empty(M, dtype=torch.int32, device=dev)
    status = torch.full((G,), -5, dtype=torch.int32, device=dev)
    ids = [(gt._put(i, np.int64, dev), len(i), w) for i, w in bounds]
    stream = torch.cuda.current_stream(dev).cuda_stream
    times = []
    for r in range(repeat + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for ids_d, count, words in ids:
            _lib.check(_lib.lib().desco_core_truss_dev(graph_ptr.data_ptr(), rowptr.data_ptr(), col.data_ptr(), G, M,
                                                       entry_row.data_ptr(), ids_d.data_ptr(), count, words,
                                                       core.data_ptr(), truss.data_ptr() if M else None,
                                                       support.data_ptr() if M else None, status.data_ptr(), stream),
                       "desco_core_truss_dev")
        b.record()
        torch.cuda.synchronize()
        if r:                                                     # (the first run warms up)
            times.append(a.elapsed_time(b) * 1e-3)
    assert all(bool((status[ids_d] == 0).all()) for ids_d, _, _ in ids)
    return times


def networkx_sample(g, sample=50):
    import networkx as nx
    step = max(g.num_graphs // sample, 1)
    picked = list(range(0, g.num_graphs, step))[:sample]
    lists = g.edge_lists() if g.num_graphs <= 4096 else None
    t = 0.0
    for i in picked:
        n, edges = lists[i] if lists else g.subset(i, i + 1).edge_lists()[0]
        h = nx.Graph()
        h.add_nodes_from(range(n))
        h.add_edges_from(edges)
        t0 = time.perf_counter()
        nx.core_number(h)
        k, left = 3, h
        while left.number_of_edges():
            left = nx.k_truss(left, k)
            k += 1
        t += time.perf_counter() - t0
    return t * g.num_graphs / len(picked), len(picked)


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--repeat", type=int, default=5)
    p.add_argument("--threads", type=int, default=16)
    p.add_argument("--skip_networkx", action="store_true")
    args = p.parse_args(argv)
    import torch
    from desco_amd import _lib, decomposition as D, synthetic
    assert torch.cuda.is_available(), "bench_decomposition needs an MI355X"
    workloads = (("syn_1827_shaped", synthetic.syn_1827_shaped(1827)),
                 ("cox2_shaped_x64", synthetic.cox2_shaped(467).replicate(64)))
    for name, g in workloads:
        n, m = D._graph_sizes(g)
        words = D.workspace_words(n, m)
        base = {"workload": name, "graphs": g.num_graphs, "nodes": g.num_nodes, "edges": int(m.sum()),
                "largest_workspace_words": int(words.max())}
        host_t = []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            ref = D._host(g, args.threads, True, True)
            host_t.append(time.perf_counter() - t0)
        got = D.decompose_device(g)                               # (warm-up, and the comparison)
        assert bool((got.status == 0).all()), f"{name}: a graph was refused"
        got = got.cpu()
        assert all(np.array_equal(getattr(got, f), getattr(ref, f)) for f in FIELDS), f"{name}: kernel and twin differ"
        dev_t = []
        for _ in range(args.repeat):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = D.decompose_device(g)
            b.record()
            torch.cuda.synchronize()
            dev_t.append(a.elapsed_time(b) * 1e-3)
            del out
        twin_alone = []                                           # the twin's entry point without rows and node_truss
        c, t, s = (np.zeros(k, dtype=np.int32) for k in (g.num_nodes, len(ref.truss), len(ref.truss)))
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            _lib.check(_lib.lib().desco_core_truss(g.graph_ptr.ctypes.data, g.rowptr.ctypes.data, g.col.ctypes.data,
                                                   g.num_graphs, args.threads, c.ctypes.data, t.ctypes.data,
                                                   s.ctypes.data), "desco_core_truss")
            twin_alone.append(time.perf_counter() - t0)
        assert np.array_equal(c, ref.core) and np.array_equal(t, ref.truss) and np.array_equal(s, ref.support)
        print(json.dumps({**base, "side": f"host twin, {args.threads} threads", **summary(host_t),
                          "entry_point_alone": summary(twin_alone), "max_truss": int(ref.truss.max()),
                          "max_core": int(ref.core.max()), "triangles": int(ref.support.sum()) // 3}), flush=True)
        print(json.dumps({**base, "side": "device (HIP events, uploads included)", **summary(dev_t),
                          "bit_identical": True, "speedup_median": summary(host_t)["median_s"] / summary(dev_t)["median_s"]}),
              flush=True)
        # the launches alone: the buckets of decompose_device, then one wave against four waves per graph
        order = np.argsort(-words, kind="stable").astype(np.int64)
        buckets, lo = [], -1
        for hi in D._BUCKETS:
            mine = order[(words[order] > lo) & (words[order] <= hi)]
            lo = hi
            if len(mine):
                buckets.append((mine, int(words[mine].max())))
        print(json.dumps({**base, "side": "device, launches alone (bucketed as decompose_device)",
                          "launches": len(buckets), **summary(launches_alone(g, buckets, args.repeat))}), flush=True)
        W = D.WAVE_WORDS                                          # where the entry point changes the workgroup shape
        for lo, hi in ((0, W // 4), (W // 4, W // 2), (W // 2, W)):
            small = order[(words[order] > lo) & (words[order] <= hi)]
            if len(small) == 0:
                continue
            for label, bound in (("one wave per graph", hi), ("four waves per graph", W + 4)):
                print(json.dumps({**base, "side": f"device, launch alone, graphs of {lo + 1}..{hi} words, {label}",
                                  "graphs_in_launch": len(small),
                                  **summary(launches_alone(g, [(small, bound)], args.repeat))}), flush=True)
        if not args.skip_networkx:
            t, count = networkx_sample(g)
            print(json.dumps({**base, "side": f"networkx, extrapolated from {count} graphs", "seconds": t}), flush=True)


if __name__ == "__main__":
    main()
