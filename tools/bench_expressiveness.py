"""Times the colour refinement (desco_amd.expressiveness) on one MI355X against its host twin.

Workloads: the canonical neighborhoods, depth 4, of Syn_1827-shaped (1827 graphs) and COX2-shaped x64 (29 888
molecules), 8 rounds, the three views -- "plain" on the restricted neighborhoods the homogeneous models train on,
"hetero" and "shmp" on the ball neighborhoods.  Per workload and view, only after signatures, final colours and status
of the device have been compared with the twin's bit for bit: the launches alone (HIP events around the entry point,
every array resident), the whole device call with the partition resident (``refine_device``: the bucket plan, the
launches, HIP events), and the twin on --threads threads (host clock, arrays in place), min / median / max of --repeat
runs after a warm-up.  Then, on the Syn shape under "shmp", the launch alone by segment size with one wave and with four
waves per segment: what decides DESCO_WL_WAVE_ROWS (--wave_rows: the threshold of the library under test, when another
build is loaded through DESCO_LIB).  One JSON line per measurement.

    python tools/bench_expressiveness.py [--repeat 5] [--threads 16]
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

ROUNDS = 8


def summary(xs):
    xs = sorted(xs)
    return {"min_s": xs[0], "median_s": xs[len(xs) // 2], "max_s": xs[-1], "runs": len(xs)}


def launches_alone(X, b, group, plan, repeat):
    """Seconds of the entry point alone over the launches ``plan`` = [(seg_ids tensor or None, bound)], arrays resident"""
    import torch
    from desco_amd import _lib
    S = b.seg_ptr.numel() - 1
    sig = torch.empty(S, dtype=torch.int64, device="cuda")
    status = torch.full((S,), -5, dtype=torch.int32, device="cuda")
    g = np.asarray(group, dtype=np.int32)
    stream = torch.cuda.current_stream().cuda_stream
    times = []
    for r in range(repeat + 1):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for ids, bound in plan:
            _lib.check(_lib.lib().desco_wl_refine_dev(
                b.vrowptr.data_ptr(), b.vcol.data_ptr(), b.num_rows, b.slots, g.ctypes.data, b.seg_ptr.data_ptr(), S,
                b.anchor_base, None, ROUNDS, None if ids is None else ids.data_ptr(), 0 if ids is None else ids.numel(),
                bound, sig.data_ptr(), None, status.data_ptr(), stream), "desco_wl_refine_dev")
        t1.record()
        torch.cuda.synchronize()
        if r:                                                     # (the first run warms up)
            times.append(t0.elapsed_time(t1) * 1e-3)
    for ids, _ in plan:
        assert bool((status == 0).all() if ids is None else (status[ids] == 0).all())
    return times, sig


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--repeat", type=int, default=5)
    p.add_argument("--threads", type=int, default=16)
    p.add_argument("--wave_rows", type=int, default=None, help="DESCO_WL_WAVE_ROWS of the library under test")
    p.add_argument("--threshold_only", action="store_true", help="only the one-wave / four-wave comparison")
    args = p.parse_args(argv)
    import torch
    from desco_amd import expressiveness as X, synthetic
    from desco_amd.batch import NeighborhoodBatch
    from desco_amd.partition import build_partition_device
    assert torch.cuda.is_available(), "bench_expressiveness needs an MI355X"
    W = args.wave_rows or X.WAVE_ROWS
    workloads = (("syn_1827_shaped", synthetic.syn_1827_shaped(1827)),
                 ("cox2_shaped_x64", synthetic.cox2_shaped(467).replicate(64)))
    for name, g in workloads:
        for restricted, views in ((False, ("shmp", "hetero")), (True, ("plain",))):
            if args.threshold_only and (restricted or not name.startswith("syn")):
                continue
            part = build_partition_device(g, 4, "cuda", restricted=restricted)
            batch = NeighborhoodBatch(part, "cuda")
            b = X._block(batch)
            rows = X.segment_rows(b)
            base = {"workload": name, "restricted": restricted, "neighborhoods": part.num_neigh, "rows": part.num_rows,
                    "entries": part.num_edges, "largest_segment_rows": int(rows.max().item()), "rounds": ROUNDS}
            host_block = X.Block(*X._host_arrays(b, None)[:2], b.num_rows, 4, X._host_arrays(b, None)[2], b.anchor_base)
            for view in views if not args.threshold_only else ():
                group = X.view_groups(view, 4)
                host_t = []
                for _ in range(args.repeat):
                    t0 = time.perf_counter()
                    ref = X._host(host_block, group, ROUNDS, None, True, args.threads)
                    host_t.append(time.perf_counter() - t0)
                got = X.refine_device(batch, view, ROUNDS, keep_colours=True).cpu()      # (warm-up, and the comparison)
                assert not got.status.any() and not ref.status.any(), f"{name}: a segment was refused"
                assert np.array_equal(got.signature, ref.signature) and np.array_equal(got.colours, ref.colours), \
                    f"{name} {view}: kernel and twin differ"
                dev_t = []
                for _ in range(args.repeat):
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    out = X.refine_device(batch, view, ROUNDS)
                    t1.record()
                    torch.cuda.synchronize()
                    dev_t.append(t0.elapsed_time(t1) * 1e-3)
                    del out
                plan = X._launches(rows, None)
                alone, sig = launches_alone(X, b, group, plan, args.repeat)
                assert np.array_equal(sig.cpu().numpy(), ref.signature)
                classes = int(torch.unique(sig).numel())
                print(json.dumps({**base, "view": view, "side": f"host twin, {args.threads} threads", **summary(host_t),
                                  "classes": classes}), flush=True)
                print(json.dumps({**base, "view": view, "side": "device, whole call (partition resident)",
                                  **summary(dev_t), "bit_identical": True,
                                  "speedup_median": summary(host_t)["median_s"] / summary(dev_t)["median_s"]}), flush=True)
                print(json.dumps({**base, "view": view, "side": "device, launches alone", "launches": len(plan),
                                  **summary(alone)}), flush=True)
            if name.startswith("syn") and not restricted:         # where the entry point changes the workgroup shape
                group = X.view_groups("shmp", 4)
                lo = 0
                while lo < W:
                    hi = max(32, 2 * lo)
                    ids = torch.nonzero((rows > lo) & (rows <= hi)).flatten().contiguous()
                    if ids.numel():
                        for label, bound in (("one wave per segment", hi), ("four waves per segment", W + 1)):
                            t, _ = launches_alone(X, b, group, [(ids, bound)], args.repeat)
                            print(json.dumps({**base, "view": "shmp", "segments_in_launch": int(ids.numel()),
                                              "side": f"device, launch alone, segments of {lo + 1}..{hi} rows, {label}",
                                              **summary(t)}), flush=True)
                    lo = hi
            del batch, part, b


if __name__ == "__main__":
    main()
