"""k-core and k-truss decomposition of graph sets: where the dense regions are.

``decompose`` gives every node its core number and every undirected edge its triangle support and its truss number
(definitions: include/desco_hip.h, "CORE / TRUSS"), with the host twin (csrc/core_truss.cpp, OpenMP over graphs) or the
gfx950 kernel (csrc/core_truss_dev.hip, one workgroup per graph, the whole peel in LDS).  Both decompositions are unique
-- they do not depend on the order in which a level is peeled -- so the two agree bit for bit.  The edge rows are those
of ``groundtruth.edge_orbit_rows``, and ``support`` is the non-induced triangle column of ``edge_orbit_counts``.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from . import groundtruth as gt
from .graphs import GraphSet

# who served the last decompose call: "host", "device", or "device+host" when graphs above the device's size limit were
# decomposed by the host twin and merged
last_backend = None

DEVICE_MAX_WORDS = 40960            # DESCO_CORE_TRUSS_DEV_MAX_WORDS (include/desco_hip.h)
WAVE_WORDS = 512                    # DESCO_CORE_TRUSS_WAVE_WORDS: a launch bound up to this runs one wave per graph
_BUCKETS = (WAVE_WORDS, 4096, 16384, DEVICE_MAX_WORDS)      # LDS words per graph: one launch per bucket
_BACKENDS = ("auto", "host", "device")
NOT_LAUNCHED = 1                    # ``status`` of a graph that no launch of the call held


def _graph_sizes(graphs: GraphSet):
    """(nodes, undirected edges) of every graph, int64"""
    return np.diff(graphs.graph_ptr), np.diff(graphs.rowptr[graphs.graph_ptr]) // 2


def workspace_words(n, m):
    """LDS words the device kernel needs for a graph of n nodes and m edges (csrc/core_truss.hpp)."""
    n, m = np.asarray(n, dtype=np.int64), np.asarray(m, dtype=np.int64)
    return n + 4 + 3 * m + np.maximum(3 * m, n)


def _device_fit(graphs: GraphSet) -> np.ndarray:
    return workspace_words(*_graph_sizes(graphs)) <= DEVICE_MAX_WORDS


def _entry_rows_host(graphs: GraphSet) -> np.ndarray:
    """int64 [E]: the edge row of every CSR entry (``groundtruth._entry_rows_device`` on the host)."""
    N = max(graphs.num_nodes, 1)
    rows = np.repeat(np.arange(graphs.num_nodes, dtype=np.int64), np.diff(graphs.rowptr))
    col = np.asarray(graphs.col, dtype=np.int64)
    lower = col < rows
    entry = np.cumsum(lower) - 1
    entry[~lower] = np.searchsorted((rows * N + col)[lower], (col * N + rows)[~lower])
    return entry


def _node_truss_host(num_nodes: int, rows: np.ndarray, truss: np.ndarray) -> np.ndarray:
    out = np.zeros(num_nodes, dtype=np.int32)
    np.maximum.at(out, rows[:, 0], truss)
    np.maximum.at(out, rows[:, 1], truss)
    return out


class Decomposition:
    """Core and truss numbers of a graph set.  ``core`` int32 [N] (None unless asked for); ``truss`` and ``support``
    int32 [M], ``node_truss`` int32 [N] = the largest truss number among a node's edges, 0 without edges (None unless
    asked for); ``rows`` int64 [M, 2], the ends (u, v), u < v, of every edge row as ``groundtruth.edge_orbit_rows``.
    numpy arrays from ``decompose``, tensors on the GPU from ``decompose_device`` (``cpu()`` brings them over), which
    also sets ``status`` int32 [G]: 0 for a decomposed graph, -1 for one the kernel refused, ``NOT_LAUNCHED`` for one
    outside ``graph_ids``."""

    def __init__(self, graphs: GraphSet, core, truss, support, rows, node_truss, status=None, backend=None):
        self.graphs, self.core, self.truss, self.support = graphs, core, truss, support
        self.rows, self.node_truss, self.status, self.last_backend = rows, node_truss, status, backend

    def cpu(self) -> "Decomposition":
        host = lambda x: x.cpu().numpy() if isinstance(x, torch.Tensor) else x          # noqa: E731
        return Decomposition(self.graphs, host(self.core), host(self.truss), host(self.support), host(self.rows),
                             host(self.node_truss), host(self.status), self.last_backend)

    def graph_table(self) -> dict:
        """One row per graph: ``graph``; with core numbers ``degeneracy`` (the largest core number) and
        ``nodes_in_top_core``; with truss numbers ``max_truss`` (0 without edges), ``edges_in_top_truss`` and
        ``triangles`` = the sum of ``support`` / 3.  int64 columns."""
        d, g = self.cpu(), self.graphs
        G = g.num_graphs
        out = {"graph": np.arange(G, dtype=np.int64)}

        def top(values, owner):
            best = np.zeros(G, dtype=np.int64)
            np.maximum.at(best, owner, values)
            count = np.zeros(G, dtype=np.int64)
            np.add.at(count, owner, values == best[owner])
            return best, count

        if d.core is not None:
            out["degeneracy"], out["nodes_in_top_core"] = top(d.core.astype(np.int64), g.node_graph_ids())
        if d.truss is not None:
            owner = np.repeat(np.arange(G, dtype=np.int64), _graph_sizes(g)[1])
            out["max_truss"], out["edges_in_top_truss"] = top(d.truss.astype(np.int64), owner)
            tri = np.zeros(G, dtype=np.int64)
            np.add.at(tri, owner, d.support.astype(np.int64))
            out["triangles"] = tri // 3
        return out

    def _keep_entries(self, keep: np.ndarray) -> GraphSet:
        g = self.graphs
        rows = np.repeat(np.arange(g.num_nodes, dtype=np.int64), np.diff(g.rowptr))
        rowptr = np.zeros(g.num_nodes + 1, dtype=np.int64)
        np.add.at(rowptr, rows[keep] + 1, 1)
        return GraphSet(g.graph_ptr, np.cumsum(rowptr), g.col[keep], g.node_feat)

    def k_core(self, k: int) -> GraphSet:
        """The k-cores: the same ``graph_ptr`` and node ids, only the edges between nodes of core number >= k."""
        if self.core is None:
            raise ValueError("k_core needs the core numbers (decompose(..., core=True))")
        g, core = self.graphs, self.cpu().core
        rows = np.repeat(np.arange(g.num_nodes, dtype=np.int64), np.diff(g.rowptr))
        return self._keep_entries((core[rows] >= k) & (core[g.col] >= k))

    def k_truss(self, k: int) -> GraphSet:
        """The k-trusses: the same ``graph_ptr`` and node ids, only the edges of truss number >= k."""
        if self.truss is None:
            raise ValueError("k_truss needs the truss numbers (decompose(..., truss=True))")
        return self._keep_entries(self.cpu().truss[_entry_rows_host(self.graphs)] >= k)


def _check_backend(backend):
    if backend not in _BACKENDS:
        raise ValueError(f"unknown backend {backend!r}: one of {_BACKENDS}")


def _host(graphs: GraphSet, num_threads: int, core: bool, truss: bool) -> Decomposition:
    N, E = graphs.num_nodes, graphs.num_directed_edges
    rows = gt.edge_orbit_rows(graphs).numpy()
    M = rows.shape[0]
    c = np.zeros(N, dtype=np.int32) if core else None
    t = np.zeros(M, dtype=np.int32) if truss else None
    s = np.zeros(M, dtype=np.int32) if truss else None
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None                 # noqa: E731
    _lib.check(_lib.lib().desco_core_truss(graphs.graph_ptr.ctypes.data, graphs.rowptr.ctypes.data,
                                           graphs.col.ctypes.data if E else None, graphs.num_graphs, num_threads,
                                           ptr(c), ptr(t), ptr(s)), "desco_core_truss")
    return Decomposition(graphs, c, t, s, rows, _node_truss_host(N, rows, t) if truss else None, None, "host")


def _device(graphs: GraphSet, ids: np.ndarray, dev, core: bool, truss: bool, fill: int = 0,
            max_words: int = None) -> Decomposition:
    """The kernel on the graphs ``ids``, everything on ``dev``; the rows of other graphs hold ``fill``.  One launch per
    workspace bucket, the largest graphs of a bucket first -- or, with ``max_words``, one launch with that bound."""
    L = _lib.lib()
    G, N, E = graphs.num_graphs, graphs.num_nodes, graphs.num_directed_edges
    graph_ptr, rowptr = gt._put(graphs.graph_ptr, np.int64, dev), gt._put(graphs.rowptr, np.int64, dev)
    col = gt._put(graphs.col, np.int32, dev)
    entry_row, M = gt._entry_rows_device(SimpleNamespace(_keep=(graph_ptr, rowptr, col), E=E, N=N, dev=dev))
    if E:
        node = torch.repeat_interleave(torch.arange(N, device=dev), rowptr[1:] - rowptr[:-1], output_size=E)
        lower = col < node
        rows = torch.stack([col[lower].long(), node[lower]], dim=1)
    else:
        rows = torch.zeros((0, 2), dtype=torch.int64, device=dev)
    new = lambda size, value: torch.full((size,), value, dtype=torch.int32, device=dev)  # noqa: E731
    c = new(N, fill) if core else None
    t, s = (new(M, fill), new(M, fill)) if truss else (None, None)
    status = new(G, NOT_LAUNCHED)
    ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None               # noqa: E731
    if len(ids):
        n, m = _graph_sizes(graphs)
        words = workspace_words(n, m)
        keep = []
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            lo = -1
            for hi in (max_words,) if max_words is not None else _BUCKETS + (int(words[ids].max()),):
                mine = ids if max_words is not None else ids[(words[ids] > lo) & (words[ids] <= hi)]
                lo = max(lo, hi)
                if len(mine) == 0:
                    continue
                mine = mine[np.argsort(-words[mine], kind="stable")]
                ids_d = gt._put(mine, np.int64, dev)
                keep.append(ids_d)
                bound = max_words if max_words is not None else int(words[mine].max())
                _lib.check(L.desco_core_truss_dev(graph_ptr.data_ptr(), rowptr.data_ptr(), ptr(col), G, M,
                                                  ptr(entry_row), ids_d.data_ptr(), len(mine), bound, ptr(c), ptr(t),
                                                  ptr(s), status.data_ptr(), stream), "desco_core_truss_dev")
            torch.cuda.current_stream(dev).synchronize()            # the id lists are released when this returns
    node_truss = None
    if truss:
        node_truss = torch.zeros(N, dtype=torch.int32, device=dev)
        if M:
            node_truss.scatter_reduce_(0, rows.reshape(-1), t.repeat_interleave(2), reduce="amax")
    return Decomposition(graphs, c, t, s, rows, node_truss, status, "device")


def decompose_device(graphs: GraphSet, device="cuda", core: bool = True, truss: bool = True, graph_ids=None,
                     fill: int = 0) -> Decomposition:
    """``decompose`` by the gfx950 kernel, the results kept on the GPU.  ``graph_ids``: only these graphs are
    decomposed (default: all) and only their rows are written, the others hold ``fill``.  Every graph has to fit the
    kernel's LDS workspace (``workspace_words(n, m) <= DEVICE_MAX_WORDS``); a larger one is refused by the C entry
    point, which names the limit -- ``decompose(backend="auto")`` sends those to the host twin instead."""
    ids = np.arange(graphs.num_graphs, dtype=np.int64) if graph_ids is None else np.asarray(graph_ids, dtype=np.int64)
    if len(ids) and (ids.min() < 0 or ids.max() >= graphs.num_graphs):
        raise ValueError("graph_ids outside the graph set")
    return _device(graphs, ids, torch.device(device), core, truss, fill)


def _merged(graphs: GraphSet, num_threads: int, core: bool, truss: bool) -> Decomposition:
    """Device for the graphs that fit its workspace, host twin for the others."""
    fit = _device_fit(graphs)
    d = _device(graphs, np.flatnonzero(fit).astype(np.int64), torch.device("cuda"), core, truss).cpu()
    if fit.all():
        return d
    for g in np.flatnonzero(~fit):
        h = _host(graphs.subset(int(g), int(g) + 1), num_threads, core, truss)
        n0, n1 = int(graphs.graph_ptr[g]), int(graphs.graph_ptr[g + 1])
        r0, r1 = int(graphs.rowptr[n0]) // 2, int(graphs.rowptr[n1]) // 2
        if core:
            d.core[n0:n1] = h.core
        if truss:
            d.truss[r0:r1], d.support[r0:r1], d.node_truss[n0:n1] = h.truss, h.support, h.node_truss
        d.status[g] = 0
    d.last_backend = "device+host"
    return d


def decompose(graphs: GraphSet, backend: str = "auto", num_threads: int = 0, core: bool = True,
              truss: bool = True) -> Decomposition:
    """Core number of every node and support and truss number of every undirected edge of ``graphs`` (numpy arrays in a
    ``Decomposition``; ``core=False`` / ``truss=False`` leave that half out).

    ``backend``: "host" (OpenMP twin, ``num_threads`` threads), "device" (HIP kernel; every graph must fit its LDS
    workspace), or "auto": the device when there is one, graphs above its limit going to the host twin and being merged
    (``last_backend`` then reads "device+host")."""
    global last_backend
    _check_backend(backend)
    if backend == "host" or (backend == "auto" and not torch.cuda.is_available()):
        res = _host(graphs, num_threads, core, truss)
    elif backend == "device":
        res = decompose_device(graphs, "cuda", core, truss).cpu()
    else:
        res = _merged(graphs, num_threads, core, truss)
    last_backend = res.last_backend
    return res


def core_numbers(graphs: GraphSet, backend: str = "auto", num_threads: int = 0) -> np.ndarray:
    """int32 [N]: the core number of every node."""
    return decompose(graphs, backend, num_threads, core=True, truss=False).core


def truss_numbers(graphs: GraphSet, backend: str = "auto", num_threads: int = 0) -> np.ndarray:
    """int32 [M]: the truss number of every undirected edge, rows as ``groundtruth.edge_orbit_rows``."""
    return decompose(graphs, backend, num_threads, core=False, truss=True).truss
