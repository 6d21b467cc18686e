"""Times the graphlet degree distributions and their agreement on one MI355X against their host twin.

Builder: the graphs of the Syn_1827-shaped set and of COX2-shaped x64, one segment per graph, for the column sets in
--orbits; the orbit table is computed once (on the device) and is not part of either time.  Agreement: the
Syn_1827-shaped train x test split, the 1827 x 1827 matrix of the whole set, and COX2-shaped x64 against the 467
COX2-shaped graphs.  Every device output is first compared with the twin's bit for bit; then min / median / max of
--repeat runs: the device by HIP events around the call with its uploads included (the int64 table, or the lists, start
on the host; "resident" repeats the measurement with them already on the GPU), the twin on --threads threads by the host
clock.  A call that takes longer than --once_above seconds is timed once.  One JSON line per measurement, with the mean
and the largest list length of the shape, and one for the question the tool was written for: what the agreement says
about the densest graph of the Syn_1827-shaped test split -- a complete graph, at graphlet correlation distance 0 from
the complete training graphs -- induced and non-induced (one run, no gate).

    python tools/bench_gdd.py [--orbits all4 all5] [--repeat 5] [--threads 16]
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
    p.add_argument("--orbits", nargs="+", default=["all4", "all5"], choices=("gcd11", "all4", "all5"))
    p.add_argument("--repeat", type=int, default=5)
    p.add_argument("--threads", type=int, default=16)
    p.add_argument("--once_above", type=float, default=5.0)
    p.add_argument("--skip_finding", action="store_true", help="leave the densest-test-graph line out")
    args = p.parse_args(argv)
    import torch
    from desco_amd import comparison as cmp
    from desco_amd import groundtruth as gt
    from desco_amd import synthetic
    from desco_amd.data import load_data
    assert torch.cuda.is_available(), "bench_gdd needs an MI355X"

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

    def report(base, host_t, sides):
        print(json.dumps({**base, "bit_identical": True, "side": f"host twin, {args.threads} threads",
                          **summary(host_t)}), flush=True)
        for side, ts in sides:
            print(json.dumps({**base, "bit_identical": True, "side": side, **summary(ts),
                              "vs_twin_median": summary(host_t)["median_s"] / summary(ts)["median_s"]}), flush=True)

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        train, test = load_data("Syn_1827_train"), load_data("Syn_1827_test")
    syn, cox = synthetic.syn_1827_shaped(1827), synthetic.cox2_shaped(467)
    shapes = {"syn_1827_shaped": syn, "cox2_shaped_x64": cox.replicate(64)}
    for orbits in args.orbits:
        columns = cmp.orbit_set(orbits)
        flat = cmp._table_queries(columns)
        dists = {}
        for name, g in list(shapes.items()) + [("syn_1827_train", train), ("syn_1827_test", test), ("cox2_shaped", cox)]:
            table_d = gt.orbit_counts_device(g, flat, "cuda", True)
            table = table_d.cpu().numpy()
            seg = g.graph_ptr
            if name not in shapes:                                   # an operand of the agreement only
                dists[name] = cmp.GraphletDistribution(*cmp._gdd_host(table, seg, columns, args.threads), seg, columns)
                continue
            (ln, key, val), host_t = host_times(lambda: cmp._gdd_host(table, seg, columns, args.threads))
            dev, dev_t = device_times(lambda: cmp._gdd_device(torch.from_numpy(table).cuda(), seg, columns))
            assert (dev.status == 0).all()
            assert np.array_equal(dev.len.cpu().numpy(), ln) and np.array_equal(bits(dev.key), key), f"{name} {orbits}: differ"
            assert np.array_equal(bits(dev.val), bits(val)), f"{name} {orbits}: differ"
            _, res_t = device_times(lambda: cmp._gdd_device(table_d, seg, columns))
            base = {"stage": "builder", "shape": name, "orbits": orbits, "columns": len(columns), "graphs": g.num_graphs,
                    "nodes": g.num_nodes, "largest_segment": int(np.diff(seg).max()), "mean_list": float(ln.mean()),
                    "largest_list": int(ln.max()), "list_bytes": int(key.nbytes + val.nbytes)}
            report(base, host_t, [("device (HIP events, table upload included)", dev_t),
                                  ("device (HIP events, table resident)", res_t)])
            dists[name] = cmp.GraphletDistribution(ln, key, val, seg, columns)
            del table_d, dev
        for what, x, y in (("train x test split", dists["syn_1827_test"], dists["syn_1827_train"]),
                           ("1827 x 1827", dists["syn_1827_shaped"], dists["syn_1827_shaped"]),
                           ("29888 x 467", dists["cox2_shaped_x64"], dists["cox2_shaped"])):
            base = {"stage": "agreement", "shape": what, "orbits": orbits, "columns": len(columns),
                    "pairs": len(x) * len(y), "mean_list": float((x.len.mean() + y.len.mean()) / 2),
                    "largest_list": int(max(x.len.max(), y.len.max()))}
            (want, _), host_t = host_times(lambda: cmp._gdda_host(x, y, False, args.threads))
            (got, _), dev_t = device_times(lambda: cmp._gdda_device(x.cuda(), x.cuda() if y is x else y.cuda(), False))
            assert np.array_equal(bits(got), bits(want)), f"agreement {what} {orbits}: the kernel and the twin differ"
            xd = x.cuda()
            yd = xd if y is x else y.cuda()
            cmp._seg_on(xd, xd.key.device), cmp._seg_on(yd, yd.key.device)
            _, res_t = device_times(lambda: cmp._gdda_device(xd, yd, False))
            report(base, host_t, [("device (HIP events, uploads included)", dev_t),
                                  ("device (HIP events, lists resident)", res_t)])
            del got, xd, yd

    # ---- the densest test graph of the Syn_1827-shaped split ---------------------------------------------------------------
    if args.skip_finding:
        return
    deg = np.diff(test.rowptr[test.graph_ptr]) / np.maximum(np.diff(test.graph_ptr), 1)
    tdeg = np.diff(train.rowptr[train.graph_ptr]) / np.maximum(np.diff(train.graph_ptr), 1)
    g = int(np.argmax(deg))
    gcm_a, gcm_b = cmp.graphlet_correlation(train, "all5"), cmp.graphlet_correlation(test, "all5")
    gi, gd = cmp.nearest(gcm_a, gcm_b, k=1)
    for induced in (True, False):
        a = cmp.graphlet_distribution(train, "all5", induced)
        b = cmp.graphlet_distribution(test, "all5", induced)
        idx, agree = cmp.gdd_nearest(a, b, k=1)
        best = agree[:, 0]
        with_gcd_nearest = cmp.gdd_agreement(b.rows(g, g + 1), a.rows(int(gi[g, 0]), int(gi[g, 0]) + 1))[0, 0]
        print(json.dumps({"stage": "densest test graph", "orbits": "all5", "induced": induced,
                          "train_graphs": train.num_graphs, "test_graphs": test.num_graphs, "graph": g,
                          "nodes": int(np.diff(test.graph_ptr)[g]), "avg_degree": float(deg[g]),
                          "best_train_graph": int(idx[g, 0]), "best_train_nodes": int(np.diff(train.graph_ptr)[idx[g, 0]]),
                          "best_train_avg_degree": float(tdeg[idx[g, 0]]), "best_agreement": float(best[g]),
                          "split_median": float(np.median(best)), "split_mean": float(best.mean()),
                          "split_min": float(best.min()), "test_graphs_agreeing_less": int((best < best[g]).sum()),
                          "gcd_nearest_train_graph": int(gi[g, 0]), "gcd_nearest_distance": float(gd[g, 0]),
                          "agreement_with_gcd_nearest": float(with_gcd_nearest), "backend": cmp.last_backend}),
              flush=True)


if __name__ == "__main__":
    main()
