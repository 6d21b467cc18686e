#!/usr/bin/env python3
"""Inference set-up time (developer tool): canonical-partition build, host C++ (OpenMP) vs device builder, and the wall
time of ``InferencePipeline(...)`` construction with the host prologue (``DESCO_DEVICE_PROLOGUE=0``: download, host
slice + degree sort, upload) against the device prologue (``=1``: csrc/batch_dev.hip), alternating, with the stage
split of each.  Every time is a host clock around work that ends in ``torch.cuda.synchronize()``, after one warm-up
build on a small subset.

    tools/bench_partition.py [--repeats 5] [--workloads cox2:64,msrc_imdb:8,syn_1827:2] [--no-host-build] [--json FILE]

On a tree without the device prologue (no ``NeighborhoodPartition.slice_device``) only the host legs run, so the same
script measures the commit before it."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from desco_amd import synthetic
from desco_amd.batch import NeighborhoodBatch
from desco_amd.data import STANDARD_QUERY_IDS
from desco_amd.lightning_model import GossipCountingModel, NeighborhoodCountingModel
from desco_amd.partition import NeighborhoodPartition, build_partition, build_partition_device
from desco_amd.pipeline import InferencePipeline, _split_by_budget

HAS_DEVICE_PROLOGUE = hasattr(NeighborhoodPartition, "slice_device")
FIELDS = ("neigh_index", "indicator", "count_ptr", "count_orig", "vrowptr", "vcol")


def _models(device):
    import argparse as ap
    na = ap.Namespace(layer_num=8, conv_type="SAGE", use_hetero=True, dropout=0.0, depth=4, lr=1e-4, weight_decay=0.0,
                      use_tconv=True, hidden_dim=64, input_dim=1, batch_size=512)
    ga = ap.Namespace(layer_num=2, conv_type="GOSSIP", use_hetero=False, dropout=0.0, lr=1e-3, weight_decay=0.0,
                      hidden_dim=64, batch_size=256)
    torch.manual_seed(0)
    nm = NeighborhoodCountingModel(1, 64, na).to_hetero_old(True, True).to(device)
    gm = GossipCountingModel(1, 64, ga, emb_channels=64, input_pattern_emb=True).to(device)
    nm.set_queries(STANDARD_QUERY_IDS)
    return nm, gm


class _Clock:
    def __init__(self):
        self.stages = {}
        torch.cuda.synchronize()
        self.t = time.perf_counter()

    def lap(self, name):
        torch.cuda.synchronize()
        now = time.perf_counter()
        self.stages[name] = self.stages.get(name, 0.0) + now - self.t
        self.t = now


def stage_split(gs, device, on_device, max_rows=48_000_000):
    """The steps of InferencePipeline.__init__ (one rank, no chunks) one by one, each ended by a synchronize."""
    c = _Clock()
    part = build_partition_device(gs, 4, device)
    c.lap("builder")
    B, G = part.num_neigh, gs.num_graphs
    if on_device:
        from desco_amd import ops
        da = part.device_arrays
        scatter, ngp = ops.neigh_rows_dev(da["neigh_index"], da["graph_ptr"], G)
        c.lap("batch_indices")
        cuts = [0, B] if part.num_rows <= max_rows else _split_by_budget(np.diff(part.count_ptr).astype(np.int64) + 1, max_rows)
        c.lap("downloads")
        blocks = [part.slice_device(a, b).degree_sorted_device() for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
        c.lap("slice_sort")
        batches = [NeighborhoodBatch(blk, device) for blk in blocks]
        c.lap("batch_indices")
    else:
        for f in FIELDS:                       # (already host arrays on a tree without lazy views: then "builder" has them)
            getattr(part, f)
        c.lap("downloads")
        cuts = _split_by_budget(np.diff(part.count_ptr).astype(np.int64) + 1, max_rows)
        blocks = [part.slice(a, b).degree_sorted() for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
        c.lap("slice_sort")
        batches = [NeighborhoodBatch(blk, device) for blk in blocks]
        per_graph = np.bincount(part.neigh_index[:, 0], minlength=G)
        ngp = torch.from_numpy(np.concatenate([[0], np.cumsum(per_graph)]).astype(np.int32)).to(device)
        rows = gs.graph_ptr[part.neigh_index[:, 0]] + part.neigh_index[:, 1]
        scatter = torch.from_numpy(rows.astype(np.int32)).to(device)
        c.lap("batch_indices")
    for b in batches:
        if HAS_DEVICE_PROLOGUE:
            b.device_prologue = on_device
        b.pool_index()
        b.max_count_rows()
    c.lap("first_pool_index")
    for b in batches:
        b.degree_table_index()
    c.lap("degree_table_index(first run, not in the constructor)")
    return {k: round(v, 4) for k, v in c.stages.items()}


def pipeline_time(nm, gm, gs, device, on_device):
    os.environ["DESCO_DEVICE_PROLOGUE"] = "1" if on_device else "0"
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pipe = InferencePipeline(nm, gm, gs, depth=4, device=device, rank=0, world=1)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert getattr(pipe, "device_prologue", False) == (on_device and HAS_DEVICE_PROLOGUE)
    del pipe
    return dt


def mmm(v):
    return {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--workloads", default="cox2:64,msrc_imdb:8,syn_1827:2")
    ap.add_argument("--no-host-build", action="store_true", help="skip the host C++ builder comparison")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    nm, gm = _models(device)
    legs = [False, True] if HAS_DEVICE_PROLOGUE else [False]
    result = {"device_prologue_available": HAS_DEVICE_PROLOGUE, "workloads": {}}
    for item in args.workloads.split(","):
        wl, rep = item.split(":")
        rep = int(rep)
        gs = synthetic.WORKLOADS[wl]().replicate(rep)
        small = gs.subset(0, 8)
        for on in legs:                                  # warm-up (module load, allocator) on a small subset
            pipeline_time(nm, gm, small, device, on)
            stage_split(small, device, on)
        r = {"graphs": gs.num_graphs, "nodes": gs.num_nodes}
        if not args.no_host_build:
            t0 = time.perf_counter(); h = build_partition(gs, 4); th = time.perf_counter() - t0
            torch.cuda.synchronize()
            t0 = time.perf_counter(); d = build_partition_device(gs, 4); torch.cuda.synchronize(); td = time.perf_counter() - t0
            same = all((getattr(h, f) == getattr(d, f)).all() for f in ("count_ptr", "vrowptr", "vcol", "count_orig"))
            r.update(neighborhoods=h.num_neigh, rows=h.num_rows, edges=h.num_edges, host_build_s=round(th, 3),
                     device_build_s=round(td, 3), identical=bool(same))
            del h, d
        times = {on: [] for on in legs}
        for _ in range(max(1, args.repeats)):            # alternating
            for on in legs:
                times[on].append(pipeline_time(nm, gm, gs, device, on))
        for on in legs:
            name = "device_prologue" if on else "host_prologue"
            r[name] = {"pipeline_construction_s": mmm(times[on]), "stages_s": stage_split(gs, device, on)}
        result["workloads"][f"{wl}x{rep}"] = r
        print(f"{wl} x{rep}: " + json.dumps(r), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
