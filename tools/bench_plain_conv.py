#!/usr/bin/env python3
"""Neighborhood stage of the plain GIN / GCN models (--neigh_conv_type GIN / GCN, gnn_model.plain_forward) on the
COX2-shaped x64 workload's RESTRICTED neighborhoods, 8 layers, the 29 standard queries: ms per inference pass of
NeighborhoodCountingModel._logits (HIP events around one pass, device synchronise, warm-up first).  Each type at H = 64
and 128, with the fused plain-layer kernel (desco_plain_layer_f16x3_f32) and un-fused (gather + eps x + f16x3 GEMMs,
PLAIN_FUSED off); the homogeneous SAGE model at H = 64 beside them, for scale.  The variants are timed in ALTERNATING
rounds (every round runs each variant a few times) and the median over all of a variant's passes is printed with its
quartiles, so that other work on the host hits all of them alike.  Prints one JSON line at the end.
usage: bench_plain_conv.py [--widths 64,128] [--rounds 10] [--per_round 3] [--copies 64]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from desco_amd import data, gnn_model as GM, synthetic  # noqa: E402
from desco_amd.batch import NeighborhoodBatch  # noqa: E402
from desco_amd.lightning_model import NeighborhoodCountingModel  # noqa: E402
from desco_amd.partition import build_partition  # noqa: E402


def model(conv, h):
    torch.manual_seed(0)
    a = argparse.Namespace(layer_num=8, conv_type=conv, use_hetero=False, dropout=0.0, depth=4, lr=1e-4, weight_decay=0.0,
                           use_tconv=False, use_canonical=True, hidden_dim=h, input_dim=1, batch_size=512)
    nm = NeighborhoodCountingModel(1, h, a).cuda().eval()
    nm.set_queries(data.STANDARD_QUERY_IDS, hetero=False)
    return nm


def one_pass(nm, batch, fused):
    GM.PLAIN_FUSED = fused
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record()
    nm._logits(batch, exp2=True)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", default="64,128")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--per_round", type=int, default=3)
    ap.add_argument("--copies", type=int, default=64)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_plain_conv.py needs an MI355X: a CPU run measures nothing")
    gs = synthetic.WORKLOADS["cox2"]().replicate(args.copies)
    batch = NeighborhoodBatch(build_partition(gs, 4, restricted=True), "cuda", anchor_flag=True)
    print(f"COX2 x{args.copies}, restricted: {batch.num_graphs} neighborhoods, {batch.num_rows} rows, "
          f"{batch.vcol.numel()} edges")
    variants = [("SAGE homogeneous", 64, "fused", model("SAGE", 64), True)]
    for h in [int(w) for w in args.widths.split(",")]:
        for conv in ("GIN", "GCN"):
            nm = model(conv, h)
            variants += [(conv, h, "fused", nm, True), (conv, h, "un-fused", nm, False)]
    times = {v[:3]: [] for v in variants}
    with torch.no_grad():
        for _, _, _, nm, fused in variants:                      # warm-up: code objects, packed operands, query embeddings
            for _ in range(3):
                one_pass(nm, batch, fused)
        for _ in range(args.rounds):
            for conv, h, form, nm, fused in variants:
                for _ in range(args.per_round):
                    times[(conv, h, form)].append(one_pass(nm, batch, fused))
    GM.PLAIN_FUSED = True
    result = []
    for key, ts in times.items():
        t = torch.tensor(ts)
        q = torch.quantile(t, torch.tensor([0.25, 0.5, 0.75])).tolist()
        print(f"{key[0]:17s} H={key[1]:4d} {key[2]:9s} median {q[1]:8.3f} ms per pass (quartiles {q[0]:.3f} .. {q[2]:.3f}, "
              f"{len(ts)} passes)")
        result.append({"conv": key[0], "hidden": key[1], "form": key[2], "median_ms": round(q[1], 4),
                       "q25_ms": round(q[0], 4), "q75_ms": round(q[2], 4), "passes": len(ts)})
    print(json.dumps({"workload": f"cox2 x{args.copies} restricted", "rows": batch.num_rows, "layers": 8, "queries": 29,
                      "results": result}))


if __name__ == "__main__":
    main()
