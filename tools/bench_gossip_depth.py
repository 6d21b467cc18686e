#!/usr/bin/env python3
"""Gossip stage at depth L = 1, 2, 3, 4 (--gossip_layer_num) on the COX2-shaped x64 and Syn_1827-shaped x2 workloads:
ms per inference pass (HIP events, warm-up first) and (node, query) rows per second, plus the layer kernel of the depth-L
path (desco_gossip_layer_f16x3_f32) timed alone: its ms per launch and its algorithmic bytes over that time -- rows x
(256 B read + 256 B written + 256 B per neighbour row) + CSR -- against the measured 6.3 TB/s copy
peak, and with the [R, 64] accumulator the kernel also reads and writes (512 B per row) counted too.  L = 2 runs the
fused kernel of the reference configuration; the others the depth-L path.
usage: bench_gossip_depth.py [--depths 1,2,3,4] [--iters 5]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from desco_amd import ops, synthetic  # noqa: E402
from desco_amd.batch import GossipBatch  # noqa: E402
from desco_amd.lightning_model import GossipCountingModel  # noqa: E402

COPY_PEAK = 6.3e12
Q = 29


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


def model(L):
    torch.manual_seed(0)
    a = argparse.Namespace(layer_num=L, conv_type="GOSSIP", use_hetero=False, dropout=0.0, lr=1e-3, weight_decay=0.0,
                           hidden_dim=64, batch_size=256)
    return GossipCountingModel(1, 64, a, emb_channels=64, input_pattern_emb=True).cuda().eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depths", default="1,2,3,4")
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    depths = [int(d) for d in args.depths.split(",")]
    g = torch.Generator().manual_seed(0)
    qemb = torch.randn(Q, 64, generator=g).cuda()
    for wl, rep in (("cox2", 64), ("syn_1827", 2)):
        gs = synthetic.WORKLOADS[wl]().replicate(rep)
        x = (torch.rand(gs.num_nodes, Q, generator=g) * 20).cuda()
        batch = GossipBatch(gs, "cuda", x=x)
        N, E = gs.num_nodes, batch.col.numel()
        R = N * Q
        for L in depths:
            gm = model(L)
            gm.set_query_emb(qemb)
            with torch.no_grad():
                ms = timeit(lambda: gm.graph_to_count(batch), args.iters)
            line = f"{wl} x{rep}: N={N} E={E} rows={R} | L={L}: {ms:.3f} ms per pass, {R / ms * 1e3:.3e} rows/s"
            if L >= 3:
                pk = gm.emb_model.packed()
                from desco_amd.gnn_model import _gossip_deep_consts, _gossip_query_terms_deep
                with torch.no_grad():
                    q = _gossip_query_terms_deep(gm.emb_model, pk, qemb)
                    C3, _ = _gossip_deep_consts(batch, batch.x)
                    h = torch.rand(R, 64, device="cuda")
                    acc = torch.zeros(R, 64, device="cuda")
                    out = torch.empty_like(h)
                    kms = timeit(lambda: ops.gossip_layer_f16(h, batch.rowptr, batch.col, N, Q, q["g"][1], C3, q["V"][0],
                                                              pk["deep"][0]["w"], pk["deep_p"][0], acc, out=out),
                                 args.iters)
                    klast = timeit(lambda: ops.gossip_layer_f16(h, batch.rowptr, batch.col, N, Q, q["g"][1], C3,
                                                                q["V"][0], pk["deep"][0]["w"], pk["deep_p"][0], acc,
                                                                pn=pk["deep_p"][1], out=out), args.iters)
                # algorithmic bytes: rows x (256 B read + 256 B written + 256 B per neighbour row) + CSR; the kernel
                # also reads and writes the [R, 64] accumulator and reads C3 (rows x 524 B more)
                core = R * 512.0 + 256.0 * E * Q + 4.0 * (E + N + 1)
                full = core + R * (512.0 + 12.0)
                share = 100.0 * (kms * (L - 2) + klast) / ms
                line += (f" | layer kernel {kms:.3f} ms (last layer {klast:.3f} ms), {share:.0f} % of the pass; "
                         f"{core / (kms * 1e-3) / 1e12:.2f} TB/s = {core / (kms * 1e-3) / COPY_PEAK:.2f} of the copy "
                         f"peak without the accumulator, {full / (kms * 1e-3) / 1e12:.2f} TB/s = "
                         f"{full / (kms * 1e-3) / COPY_PEAK:.2f} with it")
            print(line, flush=True)
            del gm
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
