"""Accuracy metrics of the reference (subgraph_counting/analysis.py:22-83): the parity metric the
README's accuracy table is quoted in.  Pinned by tests/golden/metrics.json.

Below them: the data-set statistics of the reference's coverage study (analysis/dataset_statistics.py) -- graph features
of node sets, canonical neighborhoods and whole graphs, on the host or the MI355X."""
from __future__ import annotations

import numpy as np


def _groups(pred, groupby):
    return [list(range(pred.shape[1]))] if groupby is None else groupby


def norm_mse(pred, truth, groupby=None):
    """MSE / Var(truth) per query group, float64 (analysis.py:22-43)."""
    pred, truth = np.asarray(pred, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    return [float(np.mean((pred[:, g] - truth[:, g]) ** 2) / np.var(truth[:, g]))
            for g in _groups(pred, groupby)]


def mse(pred, truth, groupby=None):
    pred, truth = np.asarray(pred, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    return [float(np.mean((pred[:, g] - truth[:, g]) ** 2)) for g in _groups(pred, groupby)]


def mae(pred, truth, groupby):
    pred, truth = np.asarray(pred), np.asarray(truth)
    return [float(np.mean(np.abs(pred[:, g] - truth[:, g]))) for g in groupby]


# ---- data-set statistics: graph features of node sets (include/desco_hip.h, "Data-set statistics") -------------------
# The reference's coverage study computes seven features per canonical neighborhood with networkx, one neighborhood at a
# time: nx.density, nx.average_clustering, nx.average_shortest_path_length and nx.diameter on the largest connected
# component.  Here they are derived from seven exact per-set quantities computed natively (csrc/subgraph_stats.cpp on
# the host, csrc/subgraph_stats_dev.hip on the MI355X).
STAT_FIELDS = ("members", "n", "m", "diameter", "dist_sum", "triangles")
TABLE_COLUMNS = ("clustering", "shortest_path_length", "diameter", "density", "num_nodes", "num_edges", "avg_degree")
# word buckets of the device kernel: a set of up to 64 * words members runs in the launch of `words`
DEVICE_WORDS = (1, 2, 4, 8, 16)
DEVICE_SET_LIMIT = 64 * DEVICE_WORDS[-1]
# which side served the last subgraph_statistics call: "host", "device", or "device+host" when the device handed sets
# it does not take (more than DEVICE_SET_LIMIT members) to the host twin
last_stats_backend = None


class SubgraphStatistics:
    """The seven raw quantities of S node sets as arrays (``members``, ``n``, ``m``, ``diameter``, ``dist_sum``,
    ``triangles`` int64 and ``clustering_sum`` float64) and ``table()``, the reference's seven columns.  ``neigh_index``
    ([S, 2] int64: graph id, node id in the graph) is set when the sets are canonical neighborhoods."""

    def __init__(self, ints: np.ndarray, clustering_sum: np.ndarray, neigh_index=None):
        ints = np.ascontiguousarray(ints, dtype=np.int64).reshape(-1, len(STAT_FIELDS))
        for k, name in enumerate(STAT_FIELDS):
            setattr(self, name, ints[:, k].copy())
        self.clustering_sum = np.ascontiguousarray(clustering_sum, dtype=np.float64)
        self.neigh_index = neigh_index

    def __len__(self):
        return len(self.n)

    def table(self) -> dict:
        """column name -> float64 [S], in the column order of the reference's CSV; zeros for an empty set."""
        n, m = self.n.astype(np.float64), self.m.astype(np.float64)
        pairs = n * (n - 1.0)
        safe_pairs, safe_n = np.where(pairs > 0, pairs, 1.0), np.where(n > 0, n, 1.0)
        cols = {
            "clustering": self.clustering_sum / safe_n,
            "shortest_path_length": np.where(pairs > 0, self.dist_sum / safe_pairs, 0.0),
            "diameter": self.diameter.astype(np.float64),
            "density": np.where(pairs > 0, 2.0 * m / safe_pairs, 0.0),
            "num_nodes": n,
            "num_edges": m,
            "avg_degree": 2.0 * m / safe_n,
        }
        return {c: cols[c] for c in TABLE_COLUMNS}


def _check_sets(graphs, set_ptr, set_nodes):
    set_ptr = np.ascontiguousarray(set_ptr, dtype=np.int64).reshape(-1)
    set_nodes = np.ascontiguousarray(set_nodes, dtype=np.int32).reshape(-1)
    if len(set_ptr) == 0:
        raise ValueError("subgraph_statistics: set_ptr needs at least one entry")
    return set_ptr, set_nodes


def _stats_host(graphs, set_ptr, set_nodes, num_threads=0):
    from . import _lib
    S = len(set_ptr) - 1
    ints, cs = np.zeros((S, len(STAT_FIELDS)), dtype=np.int64), np.zeros(S, dtype=np.float64)
    _lib.check(_lib.lib().desco_subgraph_stats(
        graphs.rowptr.ctypes.data, graphs.col.ctypes.data if len(graphs.col) else None, graphs.num_nodes,
        set_ptr.ctypes.data, set_nodes.ctypes.data if len(set_nodes) else None, S, num_threads, ints.ctypes.data,
        cs.ctypes.data), "desco_subgraph_stats")
    return ints, cs


def subgraph_stats_launch(rowptr, col, num_nodes, set_ptr, set_nodes, set_ids, words, out_i64, out_f64):
    """One launch of desco_subgraph_stats_dev on device tensors (current stream of their device): the sets ``set_ids``
    (int64) in the bucket ``words``; writes those rows of ``out_i64`` [S, 6] / ``out_f64`` [S]."""
    import torch
    from . import _lib
    for name, t, dt in (("rowptr", rowptr, torch.int64), ("col", col, torch.int32), ("set_ptr", set_ptr, torch.int64),
                        ("set_nodes", set_nodes, torch.int32), ("set_ids", set_ids, torch.int64),
                        ("out_i64", out_i64, torch.int64), ("out_f64", out_f64, torch.float64)):
        if not t.is_cuda or t.dtype != dt or not t.is_contiguous():
            raise RuntimeError(f"subgraph_stats_launch: {name} must be a contiguous {dt} tensor on the GPU "
                               "(there is no CPU fallback; the host twin is subgraph_statistics(backend='host'))")
    with torch.cuda.device(out_i64.device):
        st = torch.cuda.current_stream(out_i64.device).cuda_stream
        _lib.check(_lib.lib().desco_subgraph_stats_dev(
            rowptr.data_ptr(), col.data_ptr(), num_nodes, set_ptr.data_ptr(), set_nodes.data_ptr(),
            set_ids.data_ptr(), set_ids.numel(), int(words), out_i64.data_ptr(), out_f64.data_ptr(), st),
            "desco_subgraph_stats_dev")


def device_buckets(set_ptr):
    """The launches of a set list (device tensor ``set_ptr``): [(words, set ids int64)] for the non-empty buckets, and
    the ids of the sets above DEVICE_SET_LIMIT members (which no launch takes)."""
    import torch
    sizes = set_ptr[1:] - set_ptr[:-1]
    edges = torch.tensor([64 * w for w in DEVICE_WORDS], device=set_ptr.device, dtype=sizes.dtype)
    bucket = torch.bucketize(sizes, edges)                 # sizes <= 64 w -> the first such w; above the last: 5
    out = []
    for k, w in enumerate(DEVICE_WORDS):
        ids = torch.nonzero(bucket == k).reshape(-1)
        if ids.numel():
            out.append((w, ids))
    return out, torch.nonzero(bucket == len(DEVICE_WORDS)).reshape(-1)


def _stats_device(graphs, rowptr_d, col_d, set_ptr_d, set_nodes_d, words=None):
    """All launches of one set list on the device; rows the device refuses (n = -1: more than ``words`` holds) go to the
    host twin and are merged in place.  Returns (ints, clustering_sum, number of host-routed sets) as numpy."""
    import torch
    dev = set_ptr_d.device
    S = set_ptr_d.numel() - 1
    out_i = torch.zeros((S, len(STAT_FIELDS)), dtype=torch.int64, device=dev)
    out_f = torch.zeros(S, dtype=torch.float64, device=dev)
    if S:
        if words is None:
            launches, over = device_buckets(set_ptr_d)
            if over.numel():                               # no bucket: the widest launch refuses them, as the ABI says
                launches.append((DEVICE_WORDS[-1], over))
        else:
            launches = [(words, torch.arange(S, device=dev, dtype=torch.int64))]
        for w, ids in launches:
            subgraph_stats_launch(rowptr_d, col_d, graphs.num_nodes, set_ptr_d, set_nodes_d, ids, w, out_i, out_f)
    ints, cs = out_i.cpu().numpy(), out_f.cpu().numpy()
    routed = np.nonzero(ints[:, 1] == -1)[0]
    if len(routed):
        ridx = torch.from_numpy(routed).to(dev)
        lo, hi = set_ptr_d[ridx], set_ptr_d[ridx + 1]
        sub_ptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(hi - lo, 0)])
        pos = torch.repeat_interleave(lo - sub_ptr[:-1], hi - lo) + torch.arange(int(sub_ptr[-1]), device=dev)
        h_i, h_f = _stats_host(graphs, sub_ptr.cpu().numpy(), set_nodes_d[pos].cpu().numpy())
        ints[routed], cs[routed] = h_i, h_f
    return ints, cs, len(routed)


def _pick_backend(backend: str) -> str:
    import torch
    if backend not in ("host", "device", "auto"):
        raise ValueError(f"unknown backend {backend!r}")
    if backend == "auto":
        return "device" if torch.cuda.is_available() else "host"
    if backend == "device" and not torch.cuda.is_available():
        raise RuntimeError("backend='device' needs the MI355X; there is no silent fallback (use backend='host')")
    return backend


def _graph_on_device(graphs, dev):
    import torch
    return torch.from_numpy(graphs.rowptr).to(dev), torch.from_numpy(graphs.col).to(dev)


def subgraph_statistics(graphs, set_ptr, set_nodes, backend: str = "auto", num_threads: int = 0, words=None,
                        device="cuda") -> SubgraphStatistics:
    """Statistics of S node sets of ``graphs``: set s = ``set_nodes[set_ptr[s]:set_ptr[s+1]]``, global node ids of one
    graph, strictly ascending.  ``backend``: "host" (OpenMP, ``num_threads``), "device" (HIP kernel, one launch per
    word bucket; sets above ``DEVICE_SET_LIMIT`` members are computed by the host twin and merged in place) or "auto"
    (the device when there is one).  ``last_stats_backend`` names who served the call.  ``words`` forces every set into
    one bucket (tests)."""
    global last_stats_backend
    import torch
    backend = _pick_backend(backend)
    set_ptr, set_nodes = _check_sets(graphs, set_ptr, set_nodes)
    if backend == "host":
        ints, cs = _stats_host(graphs, set_ptr, set_nodes, num_threads)
        last_stats_backend = "host"
        return SubgraphStatistics(ints, cs)
    if np.any(np.diff(set_ptr) < 0) or set_ptr[0] < 0 or set_ptr[-1] > len(set_nodes):
        raise RuntimeError("subgraph_statistics: set_ptr is not monotone inside set_nodes")
    dev = torch.device(device)
    rowptr_d, col_d = _graph_on_device(graphs, dev)
    ints, cs, routed = _stats_device(graphs, rowptr_d, col_d, torch.from_numpy(set_ptr).to(dev),
                                     torch.from_numpy(set_nodes).to(dev), words)
    last_stats_backend = "device+host" if routed else "device"
    return SubgraphStatistics(ints, cs)


def neighborhood_sets_device(part, graphs):
    """``set_ptr`` (int64) / ``set_nodes`` (int32) of a device-resident partition, assembled on its device: set b = the
    count rows of neighborhood b (global ids) plus its canonical node, ascending.  Nothing is downloaded."""
    import torch
    da = part._device_arrays("neighborhood_sets_device")
    B, Nc = part.num_neigh, part.num_count
    dev = da["device"]
    cp = da["count_ptr"].to(torch.int64)
    set_ptr = cp + torch.arange(B + 1, device=dev, dtype=torch.int64)
    seg = torch.bucketize(torch.arange(Nc, device=dev, dtype=torch.int64), cp[1:], right=True)   # row -> neighborhood
    set_nodes = torch.empty(Nc + B, dtype=torch.int32, device=dev)
    set_nodes[torch.arange(Nc, device=dev, dtype=torch.int64) + seg] = da["count_orig"]
    ni = da["neigh_index"]
    gp = da["graph_ptr"] if "graph_ptr" in da else torch.from_numpy(graphs.graph_ptr).to(dev)
    canon = (gp[ni[:, 0]] + ni[:, 1]).to(torch.int32)
    set_nodes[set_ptr[1:] - 1] = canon
    if Nc + B > 1:
        # ascending inside every segment?  (the builders emit count rows in ascending id order and the canonical node
        # holds the largest id; a degree-sorted partition does not)
        rising = set_nodes[1:] > set_nodes[:-1]
        rising[set_ptr[1:-1] - 1] = True
        if not bool(rising.all()):
            seg_all = torch.bucketize(torch.arange(Nc + B, device=dev, dtype=torch.int64), set_ptr[1:], right=True)
            order = torch.argsort(seg_all * (graphs.num_nodes + 1) + set_nodes.to(torch.int64))
            set_nodes = set_nodes[order].contiguous()
    return set_ptr, set_nodes


def neighborhood_sets_host(part, graphs):
    """The same two arrays from a host partition (numpy)."""
    B, Nc = part.num_neigh, part.num_count
    cp = part.count_ptr.astype(np.int64)
    set_ptr = cp + np.arange(B + 1, dtype=np.int64)
    seg = np.repeat(np.arange(B, dtype=np.int64), np.diff(cp))
    set_nodes = np.empty(Nc + B, dtype=np.int32)
    set_nodes[np.arange(Nc, dtype=np.int64) + seg] = part.count_orig
    ni = np.asarray(part.neigh_index, dtype=np.int64).reshape(-1, 2)
    set_nodes[set_ptr[1:] - 1] = graphs.graph_ptr[ni[:, 0]] + ni[:, 1]
    seg_all = np.repeat(np.arange(B, dtype=np.int64), np.diff(set_ptr))
    order = np.lexsort((set_nodes, seg_all))               # a no-op on ascending segments
    return set_ptr, np.ascontiguousarray(set_nodes[order])


def neighborhood_statistics(graphs, depth: int = 4, restricted: bool = False, backend: str = "auto",
                            partition=None) -> SubgraphStatistics:
    """Statistics of every canonical neighborhood of ``graphs`` (the reference's "neighborhood-features" table): the
    sets are each neighborhood's count rows plus its canonical node, the rows in ``neigh_index`` order (carried by the
    result).  With a GPU the partition is built there (``build_partition_device``, or ``partition`` when it is device
    resident) and the sets are assembled on its device; it is not downloaded."""
    global last_stats_backend
    import torch
    from .partition import build_partition, build_partition_device
    backend = _pick_backend(backend)
    if backend == "host":
        part = partition if partition is not None else build_partition(graphs, depth, restricted=restricted)
        set_ptr, set_nodes = neighborhood_sets_host(part, graphs)
        ints, cs = _stats_host(graphs, set_ptr, set_nodes)
        last_stats_backend = "host"
        return SubgraphStatistics(ints, cs, np.asarray(part.neigh_index, dtype=np.int64).reshape(-1, 2).copy())
    part = partition if partition is not None else build_partition_device(graphs, depth, restricted=restricted)
    da = part._device_arrays("neighborhood_statistics(backend='device')")
    set_ptr, set_nodes = neighborhood_sets_device(part, graphs)
    rowptr_d, col_d = _graph_on_device(graphs, da["device"])
    ints, cs, routed = _stats_device(graphs, rowptr_d, col_d, set_ptr, set_nodes)
    last_stats_backend = "device+host" if routed else "device"
    return SubgraphStatistics(ints, cs, da["neigh_index"].cpu().numpy())


def graph_statistics(graphs, backend: str = "auto") -> SubgraphStatistics:
    """Statistics of the whole graphs of ``graphs`` (the reference's "graph-features" table): set g = all nodes of g."""
    return subgraph_statistics(graphs, graphs.graph_ptr, np.arange(graphs.num_nodes, dtype=np.int32), backend=backend)
