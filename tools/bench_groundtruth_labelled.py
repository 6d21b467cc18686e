#!/usr/bin/env python3
"""Labelled canonical ground-truth counts (--use_node_feature): networkx VF2 (the reference's procedure) vs the native
host enumerator vs the device enumerator -- developer tool.  Prints seconds per backend; results are compared bit for
bit.  Labels are seeded one-hot rows, queries the reference's expansion of the given standard query ids."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(sys.path[0], "tests"))
import numpy as np
import torch

from desco_amd import groundtruth as GT
from desco_amd import synthetic
from desco_amd.data import add_node_feat_to_networkx, graph_atlas_plus
from desco_amd.graphs import GraphSet
from desco_amd.groundtruth import canonical_counts_labelled
from helpers import standard_queries


def labelled(gs, F):
    rng = np.random.default_rng(11)
    feat = np.concatenate([np.eye(F, dtype=np.float32)[rng.integers(F, size=int(n))] for n in np.diff(gs.graph_ptr)])
    return GraphSet(gs.graph_ptr, gs.rowptr, gs.col, feat)


def timed(gs, qs, backend):
    t0 = time.perf_counter()
    out = canonical_counts_labelled(gs, qs, backend=backend)
    if backend == "device":
        torch.cuda.synchronize()
    assert GT.last_labelled_backend == backend
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-vf2", action="store_true", help="leave out the VF2 timing of the 6-graph case")
    args = ap.parse_args()
    ALL = standard_queries()[0]
    cox2, syn = synthetic.WORKLOADS["cox2"](), synthetic.WORKLOADS["syn_1827"]().subset(300, 420)
    cases = [("cox2 first 6 graphs", cox2.subset(0, 6), 2, ALL, not args.skip_vf2),
             ("cox2 all graphs", cox2, 2, ALL, False),
             ("cox2 first 100 graphs", cox2.subset(0, 100), 7, [6, 7, 13, 14], False),
             ("syn_1827 graphs 300..419", syn, 2, ALL, False)]
    have_gpu = torch.cuda.is_available()
    if have_gpu:                                    # load the library, warm the context
        g0 = labelled(cox2.subset(0, 2), 2)
        canonical_counts_labelled(g0, add_node_feat_to_networkx(graph_atlas_plus(6), np.eye(2).tolist()), backend="device")
    for name, gs, F, ids, vf2 in cases:
        gs = labelled(gs, F)
        qs = [g for q in ids for g in add_node_feat_to_networkx(graph_atlas_plus(q), np.eye(F).tolist(), "feat")]
        t_host, host = timed(gs, qs, "host")
        lab = GT._Labelled(gs, qs, "feat")
        lab.classes()
        line = (f"{name}, F = {F}: {gs.num_graphs} graphs, {gs.num_nodes} nodes, {len(qs)} labelled queries in "
                f"{lab.num_classes} classes, total count {int(host.sum())}\n  host ({os.cpu_count()} logical cores, "
                f"OpenMP): {t_host:.3f} s")
        if have_gpu:
            t_dev, dev = timed(gs, qs, "device")
            line += f"   device incl. upload, table and copy back: {t_dev:.3f} s   identical: {torch.equal(dev, host)}"
        if vf2:
            t_vf2, ref = timed(gs, qs, "vf2")
            line += f"   VF2: {t_vf2:.3f} s   identical: {torch.equal(ref, host)}"
        print(line, flush=True)


if __name__ == "__main__":
    main()
