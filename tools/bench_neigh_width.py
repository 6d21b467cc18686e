#!/usr/bin/env python3
"""Neighborhood stage at width H = 32, 64, 128, 256 (--neigh_hidden_dim) on the COX2-shaped x64 workload: ms per inference
pass of NeighborhoodCountingModel._logits (HIP events, warm-up first).  H = 64 runs the fused kernels of the reference
configuration; the others the wide path (gnn_model.shmp_forward_wide).  At H = 128 (Wp = 128) the wide path is timed
with the fused layer kernel (desco_shmp_layer_wide_f16x3_f32) and un-fused (gather + f16x3 GEMM,
DESCO_SHMP_WIDE_FUSED=0), and one count-row launch of the layer kernel alone: ms and its algorithmic bytes per second --
rows x (Wp fp32 self row + Wp per neighbour row + Wp written) + CSR.
usage: bench_neigh_width.py [--widths 32,64,128,256] [--iters 20]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from desco_amd import gnn_model as GM, ops, synthetic  # noqa: E402
from desco_amd.batch import NeighborhoodBatch  # noqa: E402
from desco_amd.lightning_model import NeighborhoodCountingModel  # noqa: E402
from desco_amd.partition import build_partition  # noqa: E402


def timeit(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2]


def model(h):
    torch.manual_seed(0)
    a = argparse.Namespace(layer_num=8, conv_type="SAGE", use_hetero=True, dropout=0.0, depth=4, lr=1e-4,
                           weight_decay=0.0, use_tconv=True, hidden_dim=h, input_dim=1, batch_size=512)
    return NeighborhoodCountingModel(1, h, a).to_hetero_old(True, True).cuda().eval()


def main():
    from desco_amd import data
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", default="32,64,128,256")
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    gs = synthetic.WORKLOADS["cox2"]().replicate(64)
    batch = NeighborhoodBatch(build_partition(gs, 4), "cuda")
    print(f"COX2 x64: {batch.num_graphs} neighborhoods, {batch.num_rows} rows, {batch.vcol.numel()} edges")
    for h in [int(w) for w in args.widths.split(",")]:
        nm = model(h)
        nm.set_queries(data.STANDARD_QUERY_IDS)
        with torch.no_grad():
            forms = [("fused", True), ("un-fused", False)] if GM.padded_width(h) == 128 else [("", True)]
            for name, fused in forms:
                GM.SHMP_WIDE_FUSED = fused
                ms = timeit(lambda: nm._logits(batch, exp2=True), args.iters)
                print(f"H={h:4d} {name:9s} {ms:8.3f} ms per pass")
            GM.SHMP_WIDE_FUSED = True
            if h != 64:
                wp = GM.padded_width(h)
                e = nm.emb_model.packed()["layers"][1]["count"]
                x = torch.rand(batch.num_rows, wp, device="cuda")
                out = torch.empty_like(x)
                Nc = batch.num_count
                ms = timeit(lambda: ops.shmp_layer_wide(x, batch.vrowptr, batch.vcol, 4, 0, Nc, 4, e["w16"], e["b"],
                                                        out=out), args.iters * 4)
                nbytes = 4.0 * wp * (2 * Nc + int(batch.vrowptr[4 * Nc])) + 4.0 * (4 * Nc + int(batch.vrowptr[4 * Nc]))
                print(f"    layer kernel Wp={wp}: {ms:.3f} ms per count-row launch, {nbytes / ms / 1e9:.2f} TB/s")


if __name__ == "__main__":
    main()
