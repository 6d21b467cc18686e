"""Times the clique census on one MI355X against its host twin.

Workloads: Syn_1827-shaped (1827 graphs, a K32 among them) and COX2-shaped x64 (29 888 molecules of degeneracy 2..3: no
triangles, so that shape times the peel, the out-degree plumbing and the launches), each with kmax = 8 and 32.  Per
workload and kmax, only after key, graph_cliques, node_cliques and omega of the device have been compared with the
twin's bit for bit: ``clique_census_device`` (HIP events around the call: uploads, the peel launches, the out-degrees,
the census launches) against the twin on --threads threads (host clock), min / median / max of --repeat runs after a
warm-up.  Then the K32 graph of the first workload alone, both sides, against ``canonical_counts_match`` (host) on the
query K16 for that graph in a child process under --cap seconds: if the matcher does not finish, that is what is
reported, not a number.  One JSON line per measurement.

    python tools/bench_clique_census.py [--repeat 5] [--threads 16] [--cap 20]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIELDS = ("key", "graph_cliques", "node_cliques", "omega")

MATCHER_CHILD = """
import sys, time
sys.path.insert(0, sys.argv[1])
from desco_amd.graphs import GraphSet
from desco_amd.groundtruth import canonical_counts_match
clique = lambda k: (k, [(a, b) for a in range(k) for b in range(a + 1, k)])
t0 = time.perf_counter()
out = canonical_counts_match(GraphSet.from_edge_lists([clique(32)]), [clique(16)], backend="host", num_threads=int(sys.argv[2]))
print(time.perf_counter() - t0, int(out.sum()))
"""


def summary(xs):
    xs = sorted(xs)
    return {"min_s": xs[0], "median_s": xs[len(xs) // 2], "max_s": xs[-1], "runs": len(xs)}


def measure(C, torch, g, kmax, repeat, threads):
    """(twin seconds, device seconds, the twin's result) after the bit-for-bit comparison"""
    host_t = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        ref = C._host(g, kmax, True, threads)
        host_t.append(time.perf_counter() - t0)
    got = C.clique_census_device(g, kmax=kmax)                    # (warm-up, and the comparison)
    assert bool((got.status == 0).all()), "a graph was refused"
    got = got.cpu()
    assert all(np.array_equal(getattr(got, f), getattr(ref, f)) for f in FIELDS), "kernel and twin differ"
    dev_t = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = C.clique_census_device(g, kmax=kmax)
        b.record()
        torch.cuda.synchronize()
        dev_t.append(a.elapsed_time(b) * 1e-3)
        del out
    return host_t, dev_t, ref


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--repeat", type=int, default=5)
    p.add_argument("--threads", type=int, default=16)
    p.add_argument("--cap", type=float, default=20.0, help="seconds the matcher gets for K16 in K32")
    args = p.parse_args(argv)
    import torch
    from desco_amd import cliques as C, synthetic
    assert torch.cuda.is_available(), "bench_clique_census needs an MI355X"
    syn = synthetic.syn_1827_shaped(1827)
    workloads = (("syn_1827_shaped", syn), ("cox2_shaped_x64", synthetic.cox2_shaped(467).replicate(64)))
    k32 = None
    for name, g in workloads:
        for kmax in (8, 32):
            host_t, dev_t, ref = measure(C, torch, g, kmax, args.repeat, args.threads)
            top = C._graph_max(g, C.out_degrees(g, ref.key))
            base = {"workload": name, "kmax": kmax, "graphs": g.num_graphs, "nodes": g.num_nodes,
                    "edges": g.num_directed_edges // 2, "largest_out_degree": int(top.max()),
                    "graphs_per_out_bucket": np.bincount(np.digitize(top, [9, 17, 33]), minlength=4).tolist(),
                    "omega_max": int(ref.omega.max())}
            print(json.dumps({**base, "side": f"host twin, {args.threads} threads", **summary(host_t)}), flush=True)
            print(json.dumps({**base, "side": "device (HIP events, uploads included)", **summary(dev_t),
                              "bit_identical": True,
                              "speedup_median": summary(host_t)["median_s"] / summary(dev_t)["median_s"]}), flush=True)
            if name == "syn_1827_shaped" and k32 is None:
                hit = np.flatnonzero((ref.omega == 32) & (np.diff(g.graph_ptr) == 32))
                k32 = int(hit[0]) if len(hit) else -1
    if k32 is not None and k32 >= 0:
        one = syn.subset(k32, k32 + 1)
        host_t, dev_t, ref = measure(C, torch, one, 32, args.repeat, args.threads)
        base = {"workload": f"K32 alone (graph {k32} of syn_1827_shaped)", "kmax": 32,
                "k16_cliques": int(ref.graph_cliques[0, 15])}
        print(json.dumps({**base, "side": f"host twin, {args.threads} threads", **summary(host_t)}), flush=True)
        print(json.dumps({**base, "side": "device (HIP events, uploads included)", **summary(dev_t), "bit_identical": True}),
              flush=True)
        t0 = time.perf_counter()
        try:
            r = subprocess.run([sys.executable, "-c", MATCHER_CHILD, ROOT, str(args.threads)], capture_output=True,
                               text=True, timeout=args.cap)
            seconds, total = r.stdout.split()
            line = {"seconds": float(seconds), "k16_cliques": int(total), "agrees": int(total) == base["k16_cliques"]}
        except subprocess.TimeoutExpired:
            line = {"finished": False, "cap_s": args.cap, "waited_s": time.perf_counter() - t0}
        print(json.dumps({**base, "side": f"canonical_counts_match (host, {args.threads} threads) on K16", **line}), flush=True)


if __name__ == "__main__":
    main()
