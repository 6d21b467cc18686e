"""Degree-preserving null models and motif significance (Milo et al., "Network motifs", Science 2002).

``rewire`` draws replicas of a graph set by double edge switches -- every replica keeps every node's degree -- with the
host twin (csrc/null_model.cpp) or the gfx950 kernel (csrc/null_model_dev.hip); the two agree bit for bit, because the
chain of every (graph, replica) pair is defined sequentially over a counter-based generator (include/desco_hip.h,
"NULL MODEL").  ``motif_significance`` counts the queries in the graphs and in their replicas with the exact census and
turns the integers into z-scores, significance profiles and empirical p-values.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from . import _lib
from . import groundtruth as gt
from .graphs import GraphSet

# who served the last rewire / motif_significance call: "host", "device", or "device+host" when graphs above the
# device's size limit were rewired by the host twin and merged
last_backend = None

DEVICE_MAX_WORDS = 40960            # DESCO_NULL_MODEL_DEV_MAX_WORDS (include/desco_hip.h)
_BUCKETS = (1024, 4096, 16384, DEVICE_MAX_WORDS)      # LDS words per chain: one launch per bucket
_BACKENDS = ("auto", "host", "device")


def _graph_sizes(graphs: GraphSet):
    """(nodes, undirected edges) of every graph, int64"""
    n = np.diff(graphs.graph_ptr)
    return n, np.diff(graphs.rowptr[graphs.graph_ptr]) // 2


def workspace_words(n, m):
    """LDS words the device kernel needs for a graph of n nodes and m edges (csrc/null_model.hpp)."""
    n, m = np.asarray(n, dtype=np.int64), np.asarray(m, dtype=np.int64)
    return n * (((n + 31) >> 5) | 1) + m


def _check_args(replicas, swaps_per_edge, backend, graph_base, replica_base):
    if backend not in _BACKENDS:
        raise ValueError(f"unknown backend {backend!r}: one of {_BACKENDS}")
    if replicas < 0 or swaps_per_edge < 0 or graph_base < 0 or replica_base < 0:
        raise ValueError("replicas, swaps_per_edge, graph_base and replica_base must not be negative")


def _rewire_host(graphs: GraphSet, replicas, swaps_per_edge, seed, graph_base, replica_base, num_threads):
    E = graphs.num_directed_edges
    col = np.zeros((replicas, E), dtype=np.int32)
    accepted = np.zeros((replicas, graphs.num_graphs), dtype=np.int32)
    _lib.check(_lib.lib().desco_null_model_rewire(
        graphs.graph_ptr.ctypes.data, graphs.rowptr.ctypes.data, graphs.col.ctypes.data if E else None,
        graphs.num_graphs, graph_base, replicas, replica_base, swaps_per_edge, seed & (2 ** 64 - 1), num_threads,
        col.ctypes.data if col.size else None, accepted.ctypes.data if accepted.size else None),
        "desco_null_model_rewire")
    return col, accepted


def _device_fit(graphs: GraphSet) -> np.ndarray:
    n, m = _graph_sizes(graphs)
    return workspace_words(n, m) <= DEVICE_MAX_WORDS


def _rewire_device_ids(graphs: GraphSet, ids: np.ndarray, replicas, swaps_per_edge, seed, graph_base, replica_base, dev):
    """The kernel on the graphs ``ids``: (col [replicas, E] int32, accepted [replicas, G] int32) on ``dev``; the rows of
    other graphs hold the input's col and 0.  One launch per workspace bucket, the largest graphs of a bucket first."""
    L = _lib.lib()
    G, E = graphs.num_graphs, graphs.num_directed_edges
    col_in = gt._put(graphs.col, np.int32, dev)
    col = col_in.unsqueeze(0).repeat(replicas, 1).contiguous()
    accepted = torch.zeros((replicas, G), dtype=torch.int32, device=dev)
    if replicas == 0 or len(ids) == 0:
        return col, accepted
    n, m = _graph_sizes(graphs)
    words = workspace_words(n, m)
    graph_ptr, rowptr = gt._put(graphs.graph_ptr, np.int64, dev), gt._put(graphs.rowptr, np.int64, dev)
    keep = []
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        lo = -1
        for hi in _BUCKETS + (int(words[ids].max()),):
            mine = ids[(words[ids] > lo) & (words[ids] <= hi)]
            lo = max(lo, hi)
            if len(mine) == 0:
                continue
            mine = mine[np.argsort(-m[mine], kind="stable")]
            ids_d = gt._put(mine, np.int64, dev)
            keep.append(ids_d)
            _lib.check(L.desco_null_model_rewire_dev(
                graph_ptr.data_ptr(), rowptr.data_ptr(), col_in.data_ptr() if E else None, G, E, ids_d.data_ptr(),
                len(mine), int(words[mine].max()), graph_base, replicas, replica_base, swaps_per_edge,
                seed & (2 ** 64 - 1), col.data_ptr() if E else None, accepted.data_ptr(), stream),
                "desco_null_model_rewire_dev")
        torch.cuda.current_stream(dev).synchronize()            # the id lists are released when this returns
    return col, accepted


def rewire_device(graphs: GraphSet, replicas: int = 1, swaps_per_edge: int = 10, seed: int = 0, device="cuda",
                  graph_base: int = 0, replica_base: int = 0):
    """``rewire`` by the gfx950 kernel, the results kept on the GPU: (col int32 [replicas, E], accepted int32
    [replicas, G]).  Every graph has to fit the kernel's LDS workspace (``workspace_words(n, m) <= DEVICE_MAX_WORDS``);
    a larger one is refused by the C entry point, which names the limit -- ``rewire(backend="auto")`` sends those to
    the host twin instead."""
    _check_args(replicas, swaps_per_edge, "device", graph_base, replica_base)
    return _rewire_device_ids(graphs, np.arange(graphs.num_graphs, dtype=np.int64), replicas, swaps_per_edge, seed,
                              graph_base, replica_base, torch.device(device))


def _rewire_merged(graphs: GraphSet, replicas, swaps_per_edge, seed, graph_base, replica_base, num_threads, dev):
    """Device for the graphs that fit its workspace, host twin for the others: (col, accepted) on ``dev`` and whether
    the host served any."""
    fit = _device_fit(graphs)
    col, accepted = _rewire_device_ids(graphs, np.flatnonzero(fit).astype(np.int64), replicas, swaps_per_edge, seed,
                                       graph_base, replica_base, dev)
    for g in np.flatnonzero(~fit):
        one = graphs.subset(int(g), int(g) + 1)
        c, a = _rewire_host(one, replicas, swaps_per_edge, seed, graph_base + int(g), replica_base, num_threads)
        n0 = int(graphs.graph_ptr[g])
        e0, e1 = int(graphs.rowptr[n0]), int(graphs.rowptr[graphs.graph_ptr[g + 1]])
        col[:, e0:e1] = torch.from_numpy(c + np.int32(n0)).to(dev)
        accepted[:, g] = torch.from_numpy(a[:, 0]).to(dev)
    return col, accepted, not bool(fit.all())


def _route(backend: str) -> str:
    if backend == "auto":
        return "device" if torch.cuda.is_available() else "host"
    return backend


def rewire(graphs: GraphSet, replicas: int = 1, swaps_per_edge: int = 10, seed: int = 0, backend: str = "auto",
           graph_base: int = 0, replica_base: int = 0, num_threads: int = 0):
    """Degree-preserving replicas of ``graphs``: ``(sets, accepted)``, a list of ``replicas`` GraphSets with the same
    ``graph_ptr`` / ``rowptr`` (every node keeps its degree) and a new ``col``, and the int32 [replicas, G] array of
    accepted switches.

    Every (graph, replica) pair is one Markov chain of ``swaps_per_edge * m`` double edge switch attempts over the
    graph's m edges: two edge slots and an orientation are drawn from Philox4x32-10 keyed by ``seed`` and counted by
    (attempt, ``graph_base`` + graph, ``replica_base`` + replica); the switch {a,b},{c,d} -> {a,d},{c,b} is taken unless
    it would make a loop or a double edge (include/desco_hip.h, "NULL MODEL").  The result is a function of those
    numbers alone: not of the backend, the thread count, or which other graphs and replicas the call holds -- a slice
    ``graphs.subset(g0, g1)`` with ``graph_base=g0``, or replicas r0.. with ``replica_base=r0``, reproduce the bits of
    the whole call.  Graphs with fewer than 2 edges come back unchanged.  A replica MAY BE DISCONNECTED where the
    input was connected; the exact enumerators take that as it is.

    ``backend``: "host" (OpenMP twin), "device" (HIP kernel; every graph must fit its LDS workspace), or "auto": the
    device when there is one, graphs above its limit going to the host twin and being merged (``last_backend`` then
    reads "device+host")."""
    global last_backend
    _check_args(replicas, swaps_per_edge, backend, graph_base, replica_base)
    if _route(backend) == "host":
        col, accepted = _rewire_host(graphs, replicas, swaps_per_edge, seed, graph_base, replica_base, num_threads)
        last_backend = "host"
    elif backend == "device":
        c, a = rewire_device(graphs, replicas, swaps_per_edge, seed, "cuda", graph_base, replica_base)
        col, accepted, last_backend = c.cpu().numpy(), a.cpu().numpy(), "device"
    else:
        c, a, mixed = _rewire_merged(graphs, replicas, swaps_per_edge, seed, graph_base, replica_base, num_threads,
                                     torch.device("cuda"))
        col, accepted, last_backend = c.cpu().numpy(), a.cpu().numpy(), "device+host" if mixed else "device"
    return [GraphSet(graphs.graph_ptr, graphs.rowptr, col[r], graphs.node_feat) for r in range(replicas)], accepted


# ---- motif significance ------------------------------------------------------------------------------------------------
def _queries(queries):
    """[(k, edge tuple)], checked: connected, loop-free, 2..5 nodes.  None: the 29 connected graphs of 3..5 nodes."""
    if queries is None:
        return [(k, tuple(e)) for k in (3, 4, 5) for _, e in gt.census_classes(k)]
    flat = gt._flatten_queries(queries)[0]
    outside = [n for n, _ in flat if n < 2 or n > 5]
    if outside:
        raise ValueError("motif_significance takes queries of 2..5 nodes (the sizes of the census kernel); "
                         f"got one of {outside[0]}")
    if flat:
        gt.match_plan(flat)                 # refuses disconnected queries and loops, naming the reason
    return [(n, tuple((int(a), int(b)) for a, b in e)) for n, e in flat]


def _plan(flat, induced: bool):
    """(classes, M): the census classes of every size in use (census order, size by size) and the int64 [C, Q] matrix
    that takes a census row to the queries' counts -- induced: the 0/1 selection of every query's class (duplicates and
    isomorphic queries are free); non-induced: the occurrences of the query in every class (``noninduced_matrix``)."""
    classes, start = [], {}
    for k in sorted({n for n, _ in flat}):
        start[k] = len(classes)
        classes += [(n, list(e)) for n, e in gt.census_classes(k)]
    M = np.zeros((len(classes), len(flat)), dtype=np.int64)
    for q, (k, e) in enumerate(flat):
        if induced:
            M[start[k] + gt._census_class_of_mask(k)[gt._orbit_structure(k, tuple(e))[2]], q] = 1
        else:
            M[start[k]:start[k] + len(gt.census_classes(k)), q] = gt._noninduced_rows([(k, list(e))])[0]
    return classes, M


def _graph_sums_host(graphs: GraphSet, col: np.ndarray, classes, M, num_threads) -> np.ndarray:
    """int64 [G, Q]: per graph, the sum over its nodes of the canonical counts, for the graph set with ``col``."""
    census = gt._induced_host_int64(GraphSet(graphs.graph_ptr, graphs.rowptr, col), classes, num_threads)
    cs = np.concatenate([np.zeros((1, census.shape[1]), dtype=np.int64), np.cumsum(census, axis=0)])
    return (cs[graphs.graph_ptr[1:]] - cs[graphs.graph_ptr[:-1]]) @ M


class _DeviceCensus:
    """The device route's census of ``copies`` replicas at a time as ONE graph set: graph_ptr / rowptr tiled with
    offsets (uploaded once per copy count), col from the rewiring kernel, the existing census and transform kernels."""

    def __init__(self, graphs: GraphSet, classes, M, dev):
        self.g, self.classes, self.M, self.dev = graphs, classes, M, dev
        self.N, self.G, self.E = graphs.num_nodes, graphs.num_graphs, graphs.num_directed_edges
        self.words = gt._bitset_words(graphs)
        self.table = gt._class_table(classes) if classes else None
        self._tiled = {}

    def _tiles(self, copies: int):
        if copies not in self._tiled:
            g, k = self.g, np.arange(copies, dtype=np.int64)[:, None]
            tile = lambda a, step: np.concatenate([(a[None, :-1] + k * step).ravel(), [copies * step]])
            node_graph = gt._put((g.node_graph_ids()[None, :] + k * self.G).ravel(), np.int64, self.dev)
            self._tiled = {copies: (gt._put(tile(g.graph_ptr, self.N), np.int64, self.dev),
                                    gt._put(tile(g.rowptr, self.E), np.int64, self.dev),
                                    node_graph.int(), node_graph,
                                    torch.arange(copies, device=self.dev, dtype=torch.int32)[:, None] * self.N)}
        return self._tiled[copies]

    def sums(self, col: torch.Tensor) -> np.ndarray:
        """col int32 [copies, E] on the device (ids of ONE copy) -> int64 [copies, G, Q] on the host."""
        copies, Q = int(col.shape[0]), self.M.shape[1]
        if copies * self.N >= 2 ** 31:
            raise RuntimeError("motif_significance: replica_chunk * num_nodes must stay below 2^31")
        if self.N == 0 or Q == 0:
            return np.zeros((copies, self.G, Q), dtype=np.int64)
        graph_ptr, rowptr, node_graph, node_graph_index, shift = self._tiles(copies)
        d = gt._DeviceGraphs.from_device(graph_ptr, rowptr, (col + shift).reshape(-1).contiguous(), node_graph,
                                         np.tile(self.words, copies))
        census = gt._census_on(d, *self.table)
        # per-graph sums: integer adds commute, so the scatter-add is exact and the same whatever its order (a running
        # sum over 2 * 10^7 rows took 7.6 s on the MI355X where this takes 10 ms)
        per_graph = torch.zeros((copies * self.G, census.shape[1]), dtype=torch.int64, device=self.dev)
        per_graph.index_add_(0, node_graph_index, census)
        out = torch.empty((copies * self.G, Q), dtype=torch.int64, device=self.dev)
        gt._transform_device(per_graph, self.M, out, False)
        return out.cpu().numpy().reshape(copies, self.G, Q)


def _default_chunk(graphs: GraphSet, classes, replicas: int, dev) -> int:
    """Replicas per census call on the device: what half of the free memory holds (per replica: the adjacency bitset
    rows, the census with room to spare, the CSR), within the census's bitset limit and 2^31 node ids."""
    words = int(gt._bitset_words(graphs).sum())
    per = 8 * words + 3 * 8 * graphs.num_nodes * max(len(classes), 1) + 16 * graphs.num_directed_edges + 64
    free = torch.cuda.mem_get_info(dev)[0]
    chunk = min(replicas, free // 2 // per, gt._DEVICE_BITSET_LIMIT_WORDS // max(words, 1),
                (2 ** 31 - 1) // max(graphs.num_nodes, 1))
    return int(max(chunk, 1))


class MotifSignificance:
    """Counts of Q queries in G graphs (``real`` int64 [G, Q]) and in R degree-preserving replicas (``null`` int64
    [R, G, Q]; None unless kept), and per graph and query, in float64: ``mean`` and ``std`` (sample, ddof = 1) of the
    null counts, ``z`` = (real - mean) / std (NaN where std == 0), ``profile`` = z / ||z||_2 per graph with NaN taken
    as 0 (an all-zero row stays zero), ``p_over`` = (1 + #{r : null >= real}) / (R + 1) and ``p_under`` with <=.  The
    same for the data-set totals (the sum over graphs, per replica) as ``dataset_real`` [Q], ``dataset_null`` [R, Q],
    ``dataset_mean`` .. ``dataset_p_under``.  ``accepted`` int32 [R, G]: the accepted switches of every chain;
    ``last_backend``: who computed it."""

    FIELDS = ("mean", "std", "z", "profile", "p_over", "p_under")

    def __init__(self, queries, real: np.ndarray, null: np.ndarray, accepted=None, last_backend=None,
                 keep_null: bool = True):
        real, null = np.asarray(real, dtype=np.int64), np.asarray(null, dtype=np.int64)
        if null.ndim != 3 or real.shape != null.shape[1:]:
            raise ValueError("MotifSignificance: real [G, Q] and null [R, G, Q]")
        if null.shape[0] < 2:
            raise ValueError("MotifSignificance: the sample standard deviation needs replicas >= 2")
        self.queries, self.real, self.accepted, self.last_backend = list(queries), real, accepted, last_backend
        self.replicas = int(null.shape[0])
        for name, value in zip(self.FIELDS, self._moments(real, null)):
            setattr(self, name, value)
        self.dataset_real, self.dataset_null = real.sum(axis=0), null.sum(axis=1)
        for name, value in zip(self.FIELDS, self._moments(self.dataset_real[None], self.dataset_null[:, None])):
            setattr(self, "dataset_" + name, value[0])
        self.null = null if keep_null else None

    @staticmethod
    def _moments(real, null):
        x = null.astype(np.float64)
        mean, std = x.mean(axis=0), x.std(axis=0, ddof=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            z = np.where(std == 0, np.nan, (real - mean) / std)
        zz = np.nan_to_num(z, nan=0.0)
        norm = np.sqrt((zz * zz).sum(axis=-1, keepdims=True))
        profile = np.divide(zz, norm, out=np.zeros_like(zz), where=norm > 0)
        R = null.shape[0]
        p_over = (1 + (null >= real[None]).sum(axis=0)) / (R + 1)
        p_under = (1 + (null <= real[None]).sum(axis=0)) / (R + 1)
        return mean, std, z, profile, p_over, p_under

    def table(self) -> dict:
        """One row per (graph, query), graph-major: columns graph, query, real and the six float fields."""
        G, Q = self.real.shape
        out = {"graph": np.repeat(np.arange(G), Q), "query": np.tile(np.arange(Q), G), "real": self.real.ravel()}
        out.update({f: getattr(self, f).ravel() for f in self.FIELDS})
        return out

    def dataset_table(self) -> dict:
        """One row per query: columns query, real (the data set's total) and the six float fields of the totals."""
        out = {"query": np.arange(self.real.shape[1]), "real": self.dataset_real}
        out.update({f: getattr(self, "dataset_" + f) for f in self.FIELDS})
        return out


def motif_significance(graphs: GraphSet, queries: Sequence = None, replicas: int = 100, swaps_per_edge: int = 10,
                       seed: int = 0, induced: bool = True, backend: str = "auto", replica_chunk: int = None,
                       keep_null: bool = False, num_threads: int = 0) -> MotifSignificance:
    """Are the queries over- or under-represented in ``graphs`` against random graphs with the same degree sequences?

    ``queries``: networkx graphs or (n, edges) pairs of 2..5 nodes, connected, duplicates allowed; None = the 29
    connected graphs of 3..5 nodes in ``census_classes`` order.  Per graph, the canonical counts (``induced=False``: the
    non-induced ones) are summed over the nodes -- the number of occurrences in the graph -- for the graphs and for
    ``replicas`` (>= 2) replicas drawn by ``rewire`` with the same ``swaps_per_edge`` and ``seed``.  Both routes count
    the census of all classes of the sizes in use and apply one exact int64 matrix, so they agree in every integer and
    therefore in every float.

    "device" (and "auto" with a GPU): the kernel's replicas stay on the card, ``replica_chunk`` of them at a time are
    counted as one graph set by the census kernel and summed per graph there (default: what half of the free memory
    holds); graphs above the rewiring kernel's size limit are rewired by the host twin and uploaded (``last_backend``
    reads "device+host").  "host": the OpenMP twin and the host enumerator, replica by replica."""
    global last_backend
    _check_args(replicas, swaps_per_edge, backend, 0, 0)
    if replicas < 2:
        raise ValueError("motif_significance needs replicas >= 2 (sample standard deviation)")
    if replica_chunk is not None and replica_chunk < 1:
        raise ValueError("replica_chunk must be at least 1")
    flat = _queries(queries)
    classes, M = _plan(flat, induced)
    G, Q = graphs.num_graphs, len(flat)
    null = np.zeros((replicas, G, Q), dtype=np.int64)
    accepted = np.zeros((replicas, G), dtype=np.int32)
    if _route(backend) == "host":
        real = _graph_sums_host(graphs, graphs.col, classes, M, num_threads)
        chunk = replica_chunk or 8
        for r0 in range(0, replicas, chunk):
            rc = min(chunk, replicas - r0)
            col, accepted[r0:r0 + rc] = _rewire_host(graphs, rc, swaps_per_edge, seed, 0, r0, num_threads)
            for r in range(rc):
                null[r0 + r] = _graph_sums_host(graphs, col[r], classes, M, num_threads)
        served = "host"
    else:
        dev = torch.device("cuda")
        census = _DeviceCensus(graphs, classes, M, dev)
        real = census.sums(gt._put(graphs.col, np.int32, dev)[None])[0]
        chunk = replica_chunk or _default_chunk(graphs, classes, replicas, dev)
        all_fit = bool(_device_fit(graphs).all())
        if backend == "device" and not all_fit:
            rewire_device(graphs, 1, swaps_per_edge, seed, dev)         # (the entry point refuses, naming the limit)
        for r0 in range(0, replicas, chunk):
            rc = min(chunk, replicas - r0)
            if all_fit:
                col, acc = rewire_device(graphs, rc, swaps_per_edge, seed, dev, 0, r0)
            else:
                col, acc, _ = _rewire_merged(graphs, rc, swaps_per_edge, seed, 0, r0, num_threads, dev)
            null[r0:r0 + rc] = census.sums(col)
            accepted[r0:r0 + rc] = acc.cpu().numpy()
        served = "device" if all_fit else "device+host"
    last_backend = served
    return MotifSignificance(flat, real, null, accepted, served, keep_null)
