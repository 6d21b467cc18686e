#!/usr/bin/env python3
"""Times the synthetic-set generators: the gfx950 kernel (HIP events around the whole call, uploads of the parameter
arrays included), the OpenMP twin, the older stand-in and networkx.  Outputs are compared bit for bit before anything
is timed.  Prints one JSON line.

    python tools/bench_graph_gen.py [--sizes 1827 29232] [--repeat 5] [--threads 16] [--no-device]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from desco_amd import generators as G                      # noqa: E402


def mmm(xs):
    return {"min_ms": round(min(xs), 3), "median_ms": round(float(np.median(xs)), 3), "max_ms": round(max(xs), 3)}


def same(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("graph_ptr", "rowptr", "col", "deg", "status"))


def time_host(spec, threads, repeat):
    out = []
    for _ in range(repeat):
        t = time.perf_counter()
        G._host(spec, threads)
        out.append(1e3 * (time.perf_counter() - t))
    return mmm(out)


def time_device(spec, repeat, **kw):
    dev, ids = torch.device("cuda"), np.arange(spec.G, dtype=np.int64)
    G._device(spec, ids, dev, **kw)                         # warm-up: code object load, LDS attribute
    out = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        G._device(spec, ids, dev, **kw)
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return mmm(out)


def set_figures(graphs):
    from desco_amd import decomposition
    tri = decomposition.decompose(graphs, backend="host", core=False).graph_table()["triangles"]
    n = np.diff(graphs.graph_ptr)
    return {"graphs": int(graphs.num_graphs), "nodes": int(graphs.num_nodes), "edges": int(graphs.num_directed_edges // 2),
            "triangles": int(tri.sum()), "max_degree": int(np.diff(graphs.rowptr).max()),
            "max_workspace_words": int(G.workspace_words(n).max())}


def networkx_sample(fam, n, e, count=50):
    """seconds for `count` graphs of the schedule by networkx's generators, connection and relabel left out"""
    import networkx as nx
    pick = np.linspace(0, len(n) - 1, count).astype(int)
    t = time.perf_counter()
    for i in pick:
        i, f, nn, ee = int(i), int(fam[i]), int(n[i]), int(e[i])
        a, _, t0, t1 = G.family_params(f, nn, ee)
        if f == G.ER:
            nx.gnp_random_graph(nn, t0 / 2 ** 32, seed=i)
        elif f == G.WS and a >= 2:
            nx.connected_watts_strogatz_graph(nn, a, G.WS_P, seed=i)
        elif f in (G.WS, G.RANDOM):
            nx.gnm_random_graph(nn, ee, seed=i)
        elif f == G.BA:
            nx.barabasi_albert_graph(nn, a, seed=i)
        elif f == G.EBA:
            nx.extended_barabasi_albert_graph(nn, a, t0 / 2 ** 32, (t1 - t0) / 2 ** 32, seed=i)
        else:
            nx.powerlaw_cluster_graph(nn, a, t0 / 2 ** 32, seed=i)
    return (time.perf_counter() - t) / count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1827, 29232])
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-device", action="store_true")
    args = ap.parse_args()
    device = torch.cuda.is_available() and not args.no_device
    res = {"threads": args.threads, "repeat": args.repeat, "device": torch.cuda.get_device_name(0) if device else None,
           "sets": {}}
    for size in args.sizes:
        fam, n, e = G.schedule(size, seed=0)
        spec = G._spec(fam, n, e, 0, 0)
        h = G._host(spec, args.threads)
        row = {"host": time_host(spec, args.threads, args.repeat), "host_1_thread": time_host(spec, 1, 1)}
        if device:
            fit = spec.words <= G.DEVICE_MAX_WORDS
            assert fit.all(), "a graph of the schedule is above the device limit"
            for name, kw in (("device", {}), ("device_1_wave", {"waves": 1}), ("device_4_waves", {"waves": 4})):
                d = G._device(spec, np.arange(spec.G, dtype=np.int64), torch.device("cuda"), **kw).cpu()
                assert same(d, h), f"{name}: the kernel and the twin differ on {size} graphs"
                row[name] = time_device(spec, args.repeat, **kw)
            row["per_family"] = {}          # each family's graphs of the schedule alone: which body a launch waits for
            for f, fname in enumerate(G.FAMILIES):
                ids = np.flatnonzero(spec.family == f)
                part = G._Spec(spec.family[ids], spec.n[ids], spec.param[ids], spec.threshold[ids], 0, 0)
                row["per_family"][fname] = {"graphs": int(len(ids)),
                                            "device_median_ms": time_device(part, args.repeat)["median_ms"],
                                            "host_median_ms": time_host(part, args.threads, args.repeat)["median_ms"]}
        if size == 1827:            # (networkx's EBA takes minutes per graph on the general recipe's larger graphs)
            row["networkx_extrapolated_s"] = round(networkx_sample(fam, n, e) * size, 2)
            row["figures"] = set_figures(h.to_graphset())
        res["sets"][str(size)] = row
    from desco_amd import synthetic
    t = time.perf_counter()
    stand_in = synthetic.syn_1827_shaped()
    res["stand_in_1827"] = dict(set_figures(stand_in), seconds=round(time.perf_counter() - t, 3))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
