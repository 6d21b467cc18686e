"""Times the graphlet correlation matrices and distances on one MI355X against their host twin.

Matrices: the graphs of the Syn_1827-shaped set and of COX2-shaped x64, one segment per graph, for the column sets in
--orbits; the orbit table is computed once (on the device) and is not part of either time.  Distances: a 1827 x 1827
matrix (the Syn_1827-shaped vectors against themselves) and a 29 232 x 467 one (those vectors 16 times over against the
COX2-shaped ones).  Every device output is first compared with the twin's bit for bit; then min / median / max of
--repeat runs: the device by HIP events around the call with its uploads included (the int64 table, or the two vector
arrays, start on the host; "resident" repeats the matrices with the table already on the GPU), the twin on --threads
threads by the host clock.  A call that takes longer than --once_above seconds is timed once.  One JSON line per
measurement, and one for the question the tool was written for: how far the densest graph of the Syn_1827-shaped test
split is from its nearest training graph, against the split's median (one run, no gate).

    python tools/bench_graph_comparison.py [--orbits gcd11 all5] [--repeat 5] [--threads 16]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def summary(xs):
    xs = sorted(xs)
    return {"min_s": xs[0], "median_s": xs[len(xs) // 2], "max_s": xs[-1], "runs": len(xs)}


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--orbits", nargs="+", default=["gcd11", "all5"], choices=("gcd11", "all4", "all5"))
    p.add_argument("--repeat", type=int, default=5)
    p.add_argument("--threads", type=int, default=16)
    p.add_argument("--once_above", type=float, default=5.0)
    args = p.parse_args(argv)
    import torch
    from desco_amd import comparison as cmp
    from desco_amd import groundtruth as gt
    from desco_amd import synthetic
    from desco_amd.data import load_data
    assert torch.cuda.is_available(), "bench_graph_comparison needs an MI355X"

    def host_times(fn):
        ts, limit, out = [], args.repeat, None
        while len(ts) < limit:
            t0 = time.perf_counter()
            out = fn()
            ts.append(time.perf_counter() - t0)
            if ts[-1] > args.once_above:
                limit = 1
        return out, ts

    def device_times(fn):
        out = fn()                                                   # (warm-up, and the comparison)
        ts = []
        for _ in range(args.repeat):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            keep = fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) * 1e-3)
            del keep
        return out, ts

    bits = lambda a: np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a).view(np.int64)  # noqa: E731
    shapes = {"syn_1827_shaped": synthetic.syn_1827_shaped(1827), "cox2_shaped_x64": synthetic.cox2_shaped(467).replicate(64)}
    vectors = {}
    for orbits in args.orbits:
        columns = cmp.orbit_set(orbits)
        for name, g in shapes.items():
            table_d = gt.orbit_counts_device(g, cmp._table_queries(columns), "cuda", True)
            table = table_d.cpu().numpy()
            seg = g.graph_ptr
            base = {"stage": "matrices", "shape": name, "orbits": orbits, "columns": len(columns), "graphs": g.num_graphs,
                    "nodes": g.num_nodes, "largest_segment": int(np.diff(seg).max()) + 1}
            (S, rho), host_t = host_times(lambda: cmp._gcm_host(table, seg, columns, True, args.threads))
            dev, dev_t = device_times(lambda: cmp._gcm_device(torch.from_numpy(table).cuda(), seg, columns, True))
            assert (dev.status == 0).all()
            assert np.array_equal(bits(dev.S), S) and np.array_equal(bits(dev.rho), bits(rho)), f"{name} {orbits}: differ"
            assert np.array_equal(bits(dev.vector()), bits(np.ascontiguousarray(rho[:, np.triu_indices(len(columns), 1)[0],
                                                                                   np.triu_indices(len(columns), 1)[1]])))
            _, res_t = device_times(lambda: cmp._gcm_device(table_d, seg, columns, True))
            print(json.dumps({**base, "bit_identical": True, "side": f"host twin, {args.threads} threads",
                              **summary(host_t)}), flush=True)
            print(json.dumps({**base, "bit_identical": True, "side": "device (HIP events, table upload included)",
                              **summary(dev_t), "vs_twin_median": summary(host_t)["median_s"] / summary(dev_t)["median_s"]}),
                  flush=True)
            print(json.dumps({**base, "bit_identical": True, "side": "device (HIP events, table resident)",
                              **summary(res_t), "vs_twin_median": summary(host_t)["median_s"] / summary(res_t)["median_s"]}),
                  flush=True)
            vectors[(orbits, name)] = dev.vector().cpu().numpy()
            del table_d, dev
        syn, cox = vectors[(orbits, "syn_1827_shaped")], vectors[(orbits, "cox2_shaped_x64")][:467]
        for what, x, y in (("1827 x 1827", syn, syn), ("29232 x 467", np.tile(syn, (16, 1)), cox)):
            base = {"stage": "distances", "shape": what, "orbits": orbits, "P": int(x.shape[1])}
            ref, host_t = host_times(lambda: cmp._gcd_host(x, y, args.threads))
            got, dev_t = device_times(lambda: cmp.gcd_device(x, y))
            assert np.array_equal(bits(got), bits(ref)), f"distances {what} {orbits}: the kernel and the twin differ"
            print(json.dumps({**base, "bit_identical": True, "side": f"host twin, {args.threads} threads",
                              **summary(host_t)}), flush=True)
            print(json.dumps({**base, "bit_identical": True, "side": "device (HIP events, uploads included)",
                              **summary(dev_t), "vs_twin_median": summary(host_t)["median_s"] / summary(dev_t)["median_s"]}),
                  flush=True)
            del got

    # ---- the densest test graph of the Syn_1827-shaped split ---------------------------------------------------------------
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        train, test = load_data("Syn_1827_train"), load_data("Syn_1827_test")
    for orbits in args.orbits:
        a, b = cmp.graphlet_correlation(train, orbits), cmp.graphlet_correlation(test, orbits)
        idx, dist = cmp.nearest(a, b, k=1)
        deg = np.diff(test.rowptr[test.graph_ptr]) / np.maximum(np.diff(test.graph_ptr), 1)
        tdeg = np.diff(train.rowptr[train.graph_ptr]) / np.maximum(np.diff(train.graph_ptr), 1)
        g = int(np.argmax(deg))
        d = dist[:, 0]
        print(json.dumps({"stage": "densest test graph", "orbits": orbits, "train_graphs": train.num_graphs,
                          "test_graphs": test.num_graphs, "graph": g, "nodes": int(np.diff(test.graph_ptr)[g]),
                          "avg_degree": float(deg[g]), "largest_train_avg_degree": float(tdeg.max()),
                          "nearest_train_graph": int(idx[g, 0]), "nearest_train_avg_degree": float(tdeg[idx[g, 0]]),
                          "nearest_distance": float(d[g]), "split_median": float(np.median(d)),
                          "split_mean": float(d.mean()), "split_max": float(d.max()),
                          "test_graphs_farther": int((d > d[g]).sum()), "backend": cmp.last_backend}), flush=True)


if __name__ == "__main__":
    main()
