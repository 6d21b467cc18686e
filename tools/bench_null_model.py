"""Times the degree-preserving null model on one MI355X against its host twin.

Workloads: Syn_1827-shaped (1827 graphs) and COX2-shaped x64 (29 888 molecules); 16 replicas, 10 switch attempts per
edge.  Per workload: the rewiring alone (kernel: HIP events around ``rewire_device``; twin: host clock, 16 threads) and
the whole ``motif_significance`` (29 queries; host clock around a call that ends in a device synchronise).  Times are
min / median / max of --repeat runs after a warm-up, and only after the device's col and accepted arrays have been
compared with the twin's bit for bit.  One JSON line per measurement.

    python tools/bench_null_model.py [--repeat 5] [--threads 16] [--skip_host_significance]
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


def summary(xs):
    xs = sorted(xs)
    return {"min_s": xs[0], "median_s": xs[len(xs) // 2], "max_s": xs[-1], "runs": len(xs)}


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--repeat", type=int, default=5)
    p.add_argument("--threads", type=int, default=16)
    p.add_argument("--replicas", type=int, default=16)
    p.add_argument("--swaps_per_edge", type=int, default=10)
    p.add_argument("--skip_host_significance", action="store_true")
    args = p.parse_args(argv)
    import torch
    from desco_amd import motifs, synthetic
    assert torch.cuda.is_available(), "bench_null_model needs an MI355X"
    R, spe, seed = args.replicas, args.swaps_per_edge, 0
    workloads = (("syn_1827_shaped", synthetic.syn_1827_shaped(1827)),
                 ("cox2_shaped_x64", synthetic.cox2_shaped(467).replicate(64)))
    for name, g in workloads:
        n, m = motifs._graph_sizes(g)
        base = {"workload": name, "graphs": g.num_graphs, "nodes": g.num_nodes, "edges": int(m.sum()),
                "replicas": R, "swaps_per_edge": spe, "attempts": int(m.sum()) * spe * R,
                "largest_workspace_words": int(motifs.workspace_words(n, m).max())}
        # ---- rewiring: compare, then time ------------------------------------------------------------------------------
        host_t = []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            ref_col, ref_acc = motifs._rewire_host(g, R, spe, seed, 0, 0, args.threads)
            host_t.append(time.perf_counter() - t0)
        col, acc = motifs.rewire_device(g, R, spe, seed)          # (warm-up, and the comparison)
        assert np.array_equal(col.cpu().numpy(), ref_col) and np.array_equal(acc.cpu().numpy(), ref_acc), \
            f"{name}: the kernel and the twin differ"
        del col, acc
        dev_t = []
        for _ in range(args.repeat):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = motifs.rewire_device(g, R, spe, seed)
            b.record()
            torch.cuda.synchronize()
            dev_t.append(a.elapsed_time(b) * 1e-3)
            del out
        print(json.dumps({**base, "what": "rewire", "side": f"host twin, {args.threads} threads", **summary(host_t),
                          "accepted_fraction": float(ref_acc.sum()) / max(int(m.sum()) * spe * R, 1)}), flush=True)
        print(json.dumps({**base, "what": "rewire", "side": "device (HIP events, uploads included)", **summary(dev_t),
                          "bit_identical": True, "speedup_median": summary(host_t)["median_s"] / summary(dev_t)["median_s"]}),
              flush=True)
        # ---- the whole significance call ---------------------------------------------------------------------------------
        res = motifs.motif_significance(g, None, replicas=R, swaps_per_edge=spe, seed=seed, backend="device",
                                        keep_null=True)       # (warm-up)
        sig_t = []
        for _ in range(args.repeat):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            motifs.motif_significance(g, None, replicas=R, swaps_per_edge=spe, seed=seed, backend="device")
            torch.cuda.synchronize()
            sig_t.append(time.perf_counter() - t0)
        print(json.dumps({**base, "what": "motif_significance", "side": "device", "queries": 29, **summary(sig_t)}),
              flush=True)
        if not args.skip_host_significance:
            t0 = time.perf_counter()
            ref = motifs.motif_significance(g, None, replicas=R, swaps_per_edge=spe, seed=seed, backend="host",
                                            keep_null=True, num_threads=args.threads)
            host_sig = time.perf_counter() - t0
            assert np.array_equal(ref.null, res.null) and np.array_equal(ref.real, res.real), \
                f"{name}: motif_significance differs between device and host"
            print(json.dumps({**base, "what": "motif_significance", "side": f"host, {args.threads} threads",
                              "queries": 29, **summary([host_sig]), "bit_identical": True,
                              "speedup_median": host_sig / summary(sig_t)["median_s"]}), flush=True)


if __name__ == "__main__":
    main()
