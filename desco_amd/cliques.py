"""Clique census of graph sets: how much is in the dense regions.

``clique_census`` gives every graph and every node its exact number of k-cliques for every k up to ``kmax``, and every
graph its clique number (definitions: include/desco_hip.h, "CLIQUE CENSUS"), by pivoting on the out-neighbourhoods of a
core-peel order: no clique is listed, a K_n is one branch.  The host twins (csrc/clique_census.cpp, OpenMP over graphs)
or the gfx950 kernels (csrc/clique_census_dev.hip: the peel with one workgroup per graph, the census with one wave per
root).  The counts are integers modulo 2^64 whose sums commute, so the two agree bit for bit.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from . import groundtruth as gt
from .graphs import GraphSet

# who served the last clique_census / peel_order call: "host", "device", or "device+host" when graphs above a device
# limit were counted by the host twin and merged
last_backend = None

MAX_K = 64                          # DESCO_CLIQUE_MAX_K (include/desco_hip.h)
DEVICE_MAX_OUT = 64                 # DESCO_CLIQUE_DEV_MAX_OUT: the largest out-degree the census kernel takes
DEVICE_MAX_WORDS = 40960            # DESCO_PEEL_DEV_MAX_WORDS
WAVE_WORDS = 512                    # DESCO_PEEL_WAVE_WORDS: a peel launch bound up to this runs one wave per graph
_PEEL_BUCKETS = (WAVE_WORDS, 4096, 16384, DEVICE_MAX_WORDS)     # LDS words per graph: one peel launch per bucket
_OUT_BUCKETS = (8, 16, 32, DEVICE_MAX_OUT)                      # out-degree bound: one census launch per bucket
_BACKENDS = ("auto", "host", "device")
NOT_LAUNCHED = 1                    # ``status`` of a graph that no launch of the call held


def _graph_sizes(graphs: GraphSet):
    """(nodes, undirected edges) of every graph, int64"""
    return np.diff(graphs.graph_ptr), np.diff(graphs.rowptr[graphs.graph_ptr]) // 2


def peel_words(n, m):
    """LDS words the peel kernel needs for a graph of n nodes and m edges (csrc/clique_census.hpp)."""
    n, m = np.asarray(n, dtype=np.int64), np.asarray(m, dtype=np.int64)
    return 2 * n + 2 * m + 8


def wave_bytes(max_out: int, kmax: int) -> int:
    """LDS bytes per wave of a census launch (csrc/clique_census.hpp)."""
    return 8 * max_out + ((4 * max_out + 7) & ~7) + 16 * 64 * max_out + 8 * (max_out + 1) * kmax


def _peel_fit(graphs: GraphSet) -> np.ndarray:
    return peel_words(*_graph_sizes(graphs)) <= DEVICE_MAX_WORDS


def out_degrees(graphs: GraphSet, key):
    """int64 [N]: the out-degree of every node under ``key`` -- its neighbours u with (key[u], u) > (key[v], v).  A
    numpy array for a numpy key, a tensor on the key's device for a tensor."""
    N, E = graphs.num_nodes, graphs.num_directed_edges
    if isinstance(key, torch.Tensor):
        dev = key.device
        if E == 0:
            return torch.zeros(N, dtype=torch.int64, device=dev)
        rowptr, col = gt._put(graphs.rowptr, np.int64, dev), gt._put(graphs.col, np.int64, dev)
        rows = torch.repeat_interleave(torch.arange(N, device=dev), rowptr[1:] - rowptr[:-1], output_size=E)
        ku, kv = key[col], key[rows]
        return torch.bincount(rows[(ku > kv) | ((ku == kv) & (col > rows))], minlength=N)
    key = np.asarray(key)
    rows = np.repeat(np.arange(N, dtype=np.int64), np.diff(graphs.rowptr))
    col = graphs.col.astype(np.int64)
    ku, kv = key[col], key[rows]
    return np.bincount(rows[(ku > kv) | ((ku == kv) & (col > rows))], minlength=N).astype(np.int64)


def _graph_max(graphs: GraphSet, per_node: np.ndarray) -> np.ndarray:
    out = np.zeros(graphs.num_graphs, dtype=np.int64)
    np.maximum.at(out, graphs.node_graph_ids(), per_node)
    return out


class CliqueCensus:
    """Clique counts of a graph set.  ``graph_cliques`` int64 [G, kmax]: column k - 1 = the k-cliques of the graph;
    ``node_cliques`` int64 [N, kmax]: the k-cliques through the node (None unless asked for); ``omega`` int32 [G], the
    clique number; ``key`` int32 [N], the peel order the census ran under.  The counts are uint64 bit patterns: exact
    below 2^64.  numpy arrays from ``clique_census``, tensors on the GPU from ``clique_census_device`` (``cpu()`` brings
    them over), which also sets ``status`` int32 [G]: 0 for a counted graph, -1 for one a kernel refused,
    ``NOT_LAUNCHED`` for one outside ``graph_ids``."""

    def __init__(self, graphs: GraphSet, graph_cliques, node_cliques, omega, key, status=None, backend=None):
        self.graphs, self.graph_cliques, self.node_cliques, self.omega = graphs, graph_cliques, node_cliques, omega
        self.key, self.status, self.last_backend = key, status, backend

    @property
    def kmax(self) -> int:
        return int(self.graph_cliques.shape[1])

    def cpu(self) -> "CliqueCensus":
        host = lambda x: x.cpu().numpy() if isinstance(x, torch.Tensor) else x          # noqa: E731
        return CliqueCensus(self.graphs, host(self.graph_cliques), host(self.node_cliques), host(self.omega),
                            host(self.key), host(self.status), self.last_backend)

    def graph_table(self) -> dict:
        """One row per graph: ``graph``, ``omega``, ``k1`` .. ``k<kmax>``.  int64 columns."""
        d = self.cpu()
        out = {"graph": np.arange(self.graphs.num_graphs, dtype=np.int64), "omega": d.omega.astype(np.int64)}
        for k in range(self.kmax):
            out[f"k{k + 1}"] = np.ascontiguousarray(d.graph_cliques[:, k])
        return out


def _check_backend(backend):
    if backend not in _BACKENDS:
        raise ValueError(f"unknown backend {backend!r}: one of {_BACKENDS}")


def _check_kmax(kmax):
    if not 1 <= int(kmax) <= MAX_K:
        raise ValueError(f"kmax = {kmax} is outside 1..{MAX_K} (DESCO_CLIQUE_MAX_K)")


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def _peel_host(graphs: GraphSet, num_threads: int):
    key, core = np.zeros(graphs.num_nodes, dtype=np.int32), np.zeros(graphs.num_nodes, dtype=np.int32)
    _lib.check(_lib.lib().desco_peel_order(graphs.graph_ptr.ctypes.data, graphs.rowptr.ctypes.data, _ptr(graphs.col),
                                           graphs.num_graphs, num_threads, _ptr(key), _ptr(core)), "desco_peel_order")
    return key, core


def _host(graphs: GraphSet, kmax: int, nodes: bool, num_threads: int, key=None) -> CliqueCensus:
    G, N = graphs.num_graphs, graphs.num_nodes
    key = _peel_host(graphs, num_threads)[0] if key is None else np.ascontiguousarray(key, dtype=np.int32)
    if key.shape != (N,):
        raise ValueError("key must have one entry per node")
    gc = np.zeros((G, kmax), dtype=np.int64)
    nc = np.zeros((N, kmax), dtype=np.int64) if nodes else None
    omega = np.zeros(G, dtype=np.int32)
    # (an empty key array has no pointer: the twin then computes the key of the empty node set itself)
    _lib.check(_lib.lib().desco_clique_census(graphs.graph_ptr.ctypes.data, graphs.rowptr.ctypes.data, _ptr(graphs.col),
                                              G, _ptr(key), kmax, num_threads, _ptr(gc), _ptr(nc), _ptr(omega)),
               "desco_clique_census")
    return CliqueCensus(graphs, gc, nc, omega, key, None, "host")


class _Upload:
    def __init__(self, graphs: GraphSet, dev):
        self.graph_ptr, self.rowptr = gt._put(graphs.graph_ptr, np.int64, dev), gt._put(graphs.rowptr, np.int64, dev)
        # (one spare entry: the entry points want a col pointer even for a set without edges)
        self.col = gt._put(graphs.col if graphs.num_directed_edges else np.zeros(1, np.int32), np.int32, dev)


def _peel_launches(graphs: GraphSet, up: _Upload, ids: np.ndarray, dev, key, core, status, max_words=None):
    """One launch of the peel kernel per workspace bucket over ``ids``, the largest graphs of a bucket first."""
    L = _lib.lib()
    words = peel_words(*_graph_sizes(graphs))
    keep = []
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        lo = -1
        for hi in (max_words,) if max_words is not None else _PEEL_BUCKETS + (int(words[ids].max()),):
            mine = ids if max_words is not None else ids[(words[ids] > lo) & (words[ids] <= hi)]
            lo = max(lo, hi)
            if len(mine) == 0:
                continue
            mine = mine[np.argsort(-words[mine], kind="stable")]
            ids_d = gt._put(mine, np.int64, dev)
            keep.append(ids_d)
            bound = max_words if max_words is not None else int(words[mine].max())
            _lib.check(L.desco_peel_order_dev(up.graph_ptr.data_ptr(), up.rowptr.data_ptr(), up.col.data_ptr(),
                                              graphs.num_graphs, ids_d.data_ptr(), len(mine), bound, key.data_ptr(),
                                              core.data_ptr() if core is not None else None, status.data_ptr(), stream),
                       "desco_peel_order_dev")
        torch.cuda.current_stream(dev).synchronize()                # the id lists are released when this returns
    return keep


def peel_order_device(graphs: GraphSet, device="cuda", graph_ids=None, fill: int = 0):
    """(key, core, status) int32 tensors on the GPU by the peel kernel.  ``graph_ids``: only these graphs are peeled and
    only their rows written, the others hold ``fill`` (their ``status`` ``NOT_LAUNCHED``).  A graph above
    ``DEVICE_MAX_WORDS`` is refused by the C entry point, which names the limit."""
    dev = torch.device(device)
    ids = _ids(graphs, graph_ids)
    key = torch.full((graphs.num_nodes,), fill, dtype=torch.int32, device=dev)
    core = torch.full((graphs.num_nodes,), fill, dtype=torch.int32, device=dev)
    status = torch.full((graphs.num_graphs,), NOT_LAUNCHED, dtype=torch.int32, device=dev)
    if len(ids) and graphs.num_nodes:
        _peel_launches(graphs, _Upload(graphs, dev), ids, dev, key, core, status)
    elif len(ids):
        status[torch.from_numpy(ids).to(dev)] = 0
    return key, core, status


def peel_order(graphs: GraphSet, backend: str = "auto", num_threads: int = 0):
    """(key, core) int32 [N]: the pass of the level-synchronous core peel in which every node leaves, and its core
    number.  ``backend`` as in ``clique_census``."""
    global last_backend
    _check_backend(backend)
    if backend == "host" or (backend == "auto" and not torch.cuda.is_available()):
        last_backend = "host"
        return _peel_host(graphs, num_threads)
    fit = _peel_fit(graphs) if backend == "auto" else np.ones(graphs.num_graphs, dtype=bool)
    key, core, _ = peel_order_device(graphs, graph_ids=np.flatnonzero(fit))
    key, core = key.cpu().numpy(), core.cpu().numpy()
    last_backend = "device"
    for g in np.flatnonzero(~fit):
        n0, n1 = int(graphs.graph_ptr[g]), int(graphs.graph_ptr[g + 1])
        key[n0:n1], core[n0:n1] = _peel_host(graphs.subset(int(g), int(g) + 1), num_threads)
        last_backend = "device+host"
    return key, core


def _ids(graphs: GraphSet, graph_ids) -> np.ndarray:
    ids = np.arange(graphs.num_graphs, dtype=np.int64) if graph_ids is None else np.asarray(graph_ids, dtype=np.int64)
    if len(ids) and (ids.min() < 0 or ids.max() >= graphs.num_graphs):
        raise ValueError("graph_ids outside the graph set")
    return ids


def _device(graphs: GraphSet, ids: np.ndarray, dev, kmax: int, nodes: bool, fill: int = 0, key=None,
            route_over: bool = False, max_out: int = None):
    """The kernels on the graphs ``ids``, everything on ``dev``; the rows of other graphs hold ``fill``.  The peel (one
    launch per workspace bucket) unless ``key`` is given, the out-degrees by index plumbing on the device, then one
    census launch per out-degree bucket -- or, with ``max_out``, one launch with that bound.  ``route_over``: graphs
    whose largest out-degree exceeds ``DEVICE_MAX_OUT`` are left out instead of being handed to the entry point, which
    refuses them.  Returns the census and the ids that were launched."""
    L = _lib.lib()
    G, N = graphs.num_graphs, graphs.num_nodes
    full = lambda shape, dt: torch.full(shape, fill, dtype=dt, device=dev)                # noqa: E731
    gc, omega = full((G, kmax), torch.int64), full((G,), torch.int32)
    nc = full((N, kmax), torch.int64) if nodes else None
    status = torch.full((G,), NOT_LAUNCHED, dtype=torch.int32, device=dev)
    if key is None:
        key_d = full((N,), torch.int32)
    else:
        key_d = key.to(dev).to(torch.int32) if isinstance(key, torch.Tensor) else gt._put(key, np.int32, dev)
    if len(ids) == 0:
        return CliqueCensus(graphs, gc, nc, omega, key_d, status, "device"), ids
    up = _Upload(graphs, dev)
    if key is None and N:
        _peel_launches(graphs, up, ids, dev, key_d, None, status)
    mine = np.zeros(G, dtype=bool)
    mine[ids] = True
    deg = out_degrees(graphs, key_d).cpu().numpy()
    deg[~mine[graphs.node_graph_ids()]] = 0                      # (rows of graphs outside the launch hold the fill)
    top = _graph_max(graphs, deg)
    if route_over:
        ids = ids[top[ids] <= DEVICE_MAX_OUT]
    ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None                # noqa: E731
    keep = []
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        lo = -1
        for hi in (max_out,) if max_out is not None else _OUT_BUCKETS + (int(top[ids].max()) if len(ids) else 0,):
            sel = ids if max_out is not None else ids[(top[ids] > lo) & (top[ids] <= hi)]
            lo = max(lo, hi)
            if len(sel) == 0:
                continue
            sel = sel[np.argsort(-top[sel], kind="stable")]
            ids_d = gt._put(sel, np.int64, dev)
            keep.append(ids_d)
            _lib.check(L.desco_clique_census_dev(up.graph_ptr.data_ptr(), up.rowptr.data_ptr(), up.col.data_ptr(), G,
                                                 key_d.data_ptr() if N else up.col.data_ptr(), kmax, ids_d.data_ptr(),
                                                 len(sel), hi, ptr(gc), ptr(nc), ptr(omega), status.data_ptr(), stream),
                       "desco_clique_census_dev")
        torch.cuda.current_stream(dev).synchronize()                # the id lists are released when this returns
    return CliqueCensus(graphs, gc, nc, omega, key_d, status, "device"), ids


def clique_census_device(graphs: GraphSet, kmax: int = 8, nodes: bool = True, graph_ids=None, fill: int = 0,
                         device="cuda", key=None) -> CliqueCensus:
    """``clique_census`` by the gfx950 kernels, the results kept on the GPU.  ``graph_ids``: only these graphs are
    counted (default: all) and only their rows are written, the others hold ``fill``.  Every graph has to fit the peel
    kernel's LDS workspace (``peel_words(n, m) <= DEVICE_MAX_WORDS``) and have no out-degree above ``DEVICE_MAX_OUT``;
    the C entry points refuse others and name the limit -- ``clique_census(backend="auto")`` sends those to the host
    twin instead.  ``key``: a peel order to count under instead of the peel kernel's."""
    _check_kmax(kmax)
    return _device(graphs, _ids(graphs, graph_ids), torch.device(device), int(kmax), nodes, fill, key)[0]


def _merged(graphs: GraphSet, kmax: int, nodes: bool, num_threads: int) -> CliqueCensus:
    """Device for the graphs within its limits, host twin for the others."""
    fit = _peel_fit(graphs)
    d, launched = _device(graphs, np.flatnonzero(fit).astype(np.int64), torch.device("cuda"), kmax, nodes,
                          route_over=True)
    d = d.cpu()
    done = np.zeros(graphs.num_graphs, dtype=bool)
    done[launched] = True
    if done.all():
        return d
    for g in np.flatnonzero(~done):
        h = _host(graphs.subset(int(g), int(g) + 1), kmax, nodes, num_threads)
        n0, n1 = int(graphs.graph_ptr[g]), int(graphs.graph_ptr[g + 1])
        d.graph_cliques[g], d.omega[g], d.key[n0:n1] = h.graph_cliques[0], h.omega[0], h.key
        if nodes:
            d.node_cliques[n0:n1] = h.node_cliques
        d.status[g] = 0
    d.last_backend = "device+host"
    return d


def clique_census(graphs: GraphSet, kmax: int = 8, nodes: bool = True, backend: str = "auto", num_threads: int = 0,
                  key=None) -> CliqueCensus:
    """The k-cliques, k = 1 .. ``kmax``, of every graph and (``nodes``) through every node of ``graphs``, and every
    graph's clique number (numpy arrays in a ``CliqueCensus``).

    ``backend``: "host" (OpenMP twin, ``num_threads`` threads; no limit on the out-degree), "device" (HIP kernels; every
    graph must fit the peel's LDS workspace and have out-degrees of at most ``DEVICE_MAX_OUT``), or "auto": the device
    when there is one, graphs above either limit going to the host twin and being merged (``last_backend`` then reads
    "device+host").  ``key`` int32 [N]: count under this order instead of the peel's (the counts do not depend on it,
    the work does); with a key, "auto" is the host twin."""
    global last_backend
    _check_backend(backend)
    _check_kmax(kmax)
    kmax = int(kmax)
    if backend == "host" or (backend == "auto" and (key is not None or not torch.cuda.is_available())):
        res = _host(graphs, kmax, nodes, num_threads, key)
    elif backend == "device":
        res = clique_census_device(graphs, kmax, nodes, key=key).cpu()
    else:
        res = _merged(graphs, kmax, nodes, num_threads)
    last_backend = res.last_backend
    return res
