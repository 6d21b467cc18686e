#!/usr/bin/env python3
"""Whole-graph typed CSR (developer tool): the device builder behind ``GraphBatch`` (desco_graph_tconv_dev: flag, scan,
fill) against its host twin (desco_graph_tconv, OpenMP), and the builder's share of an inference pass of the model
without canonical partition (typed CSR + target embeddings + count head over the set in blocks of --batch graphs).

    tools/bench_graph_tconv.py [--repeats 20] [--workloads syn_1827:1,cox2:64] [--threads 16] [--batch 256] [--json FILE]

Device times are HIP events around ``--inner`` back-to-back builds on the uploaded CSR (one build is tens of
microseconds of kernels; the output allocation is inside, as in ``GraphBatch``), host times a host clock, the pass a
host clock around work that ends in ``torch.cuda.synchronize()``; each after a warm-up, median / min / max of the
repeats.  The two builders' outputs are compared bit for bit first."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from desco_amd import ops, synthetic
from desco_amd.batch import GraphBatch, _graphset_device_csr
from desco_amd.data import STANDARD_QUERY_IDS
from desco_amd.lightning_model import NeighborhoodCountingModel


def mmm(v):
    return {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4), "n": len(v)}


def model(device):
    na = argparse.Namespace(layer_num=8, conv_type="SAGE", use_hetero=True, dropout=0.0, depth=4, lr=1e-4,
                            weight_decay=0.0, use_tconv=True, hidden_dim=64, input_dim=1, batch_size=512,
                            use_canonical=False)
    torch.manual_seed(0)
    nm = NeighborhoodCountingModel(1, 64, na).to_hetero_wo_canonical(True, True).to(device)
    nm.set_queries(STANDARD_QUERY_IDS)
    return nm.eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--workloads", default="syn_1827:1,cox2:64")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    nm = model(device)
    result = {}
    for item in args.workloads.split(","):
        wl, rep = item.split(":")
        gs = synthetic.WORKLOADS[wl]().replicate(int(rep))
        V, E = gs.num_nodes, gs.num_directed_edges
        rowptr, col = _graphset_device_csr(gs, device)

        def build():
            return ops.graph_tconv_dev(rowptr, col, 0, V, 0, E)

        ref = ops.graph_tconv_host(gs.rowptr, gs.col, 0, V, args.threads)             # (also the host warm-up)
        got = build()
        same = bool(np.array_equal(got[0].cpu().numpy(), ref[0]) and np.array_equal(got[1].cpu().numpy(), ref[1]))
        dev_ms, host_ms, host1_ms = [], [], []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.inner):
                build()
            e1.record()
            torch.cuda.synchronize()
            dev_ms.append(e0.elapsed_time(e1) / args.inner)
            t0 = time.perf_counter()
            ops.graph_tconv_host(gs.rowptr, gs.col, 0, V, args.threads)
            host_ms.append(1e3 * (time.perf_counter() - t0))
        for _ in range(3):
            t0 = time.perf_counter()
            ops.graph_tconv_host(gs.rowptr, gs.col, 0, V, 1)
            host1_ms.append(1e3 * (time.perf_counter() - t0))

        def one_pass(prebuilt=None):
            """typed CSR + embeddings + head over the set; ``prebuilt``: batches whose arrays exist already"""
            out = []
            with torch.no_grad():
                for k, g0 in enumerate(range(0, gs.num_graphs, args.batch)):
                    b = prebuilt[k] if prebuilt else GraphBatch(gs, device, g0, min(g0 + args.batch, gs.num_graphs))
                    out.append(nm.graph_to_count(b))
            torch.cuda.synchronize()
            return out

        batches = [GraphBatch(gs, device, g0, min(g0 + args.batch, gs.num_graphs))
                   for g0 in range(0, gs.num_graphs, args.batch)]
        for b in batches:
            b.vrowptr
        one_pass(), one_pass(batches)                                                  # warm-up
        full_ms, model_ms = [], []
        for _ in range(max(3, args.repeats // 4)):                                      # alternating
            t0 = time.perf_counter(); one_pass(); full_ms.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter(); one_pass(batches); model_ms.append(1e3 * (time.perf_counter() - t0))
        r = {"graphs": gs.num_graphs, "nodes": V, "directed_edges": E, "largest_degree": int(np.diff(gs.rowptr).max()),
             "identical": same, "device_build_ms": mmm(dev_ms), f"host_build_{args.threads}_threads_ms": mmm(host_ms),
             "host_build_1_thread_ms": mmm(host1_ms), "batch_graphs": args.batch,
             "inference_pass_with_build_ms": mmm(full_ms), "inference_pass_prebuilt_ms": mmm(model_ms)}
        fm, mm = statistics.median(full_ms), statistics.median(model_ms)
        r["builder_share_of_pass"] = round((fm - mm) / fm, 4)
        result[f"{wl}x{rep}"] = r
        print(f"{wl} x{rep}: " + json.dumps(r), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
