"""Listing the occurrences of a query: the matcher's maps written out as rows (include/desco_hip.h, OCCURRENCE LISTING).

``canonical_counts_match`` says how many occurrences of a query have their largest node at ``v``; this module returns
the occurrences themselves, one int32 row of ``k`` global node ids each (column ``a`` = the image of query node ``a``),
grouped by that largest node through ``ptr`` (the exclusive scan of the count column) and sorted lexicographically inside
every group.  Host twin (``desco_list_occurrences``) and HIP kernel (``desco_list_occurrences_dev``, the listing
instantiation of the matcher's walk) return the same bits."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from . import groundtruth as gt
from .graphs import GraphSet

# name of the backend that served the last list_occurrences / iter_occurrences call ("host", "device" or "vf2")
last_backend = None
# what backend="auto" resolves to.  The project's rule: the device only where tools/bench_occurrences.py shows the whole
# device call (uploads, count pass, emit launches and ordering) ahead of the host twin on BOTH benchmark shapes.  It is
# ahead on the Syn_1827 shape for the 4-cycle and the house (2.3x; behind for the triangle) and behind on COX2 x64 (two
# walks of 1.2 M nodes against one: 63 ms against 42 ms for the 5-path), so "auto" is the host twin; backend="device" and list_occurrences_device stay
# available.
_AUTO_BACKEND = "host"
_DEFAULT_MAX_ROWS = 1 << 26


class Occurrences:
    """The occurrences of one query whose largest node is in ``[v0, v1)`` (the whole graph set: ``[0, N)``).

    ``rows``  int32 [M, k]: one occurrence per row, column ``a`` = the global id of the image of query node ``a``
    ``ptr``   int64 [v1 - v0 + 1]: the rows anchored at ``v0 + i`` are ``rows[ptr[i] - ptr[0] : ptr[i + 1] - ptr[0]]``;
              ``ptr`` holds row numbers of the ONE-SHOT listing, so the chunks of ``iter_occurrences`` concatenate
    ``k``, ``query`` (``(k, edges)``), ``induced``; numpy arrays from ``list_occurrences``, tensors on the GPU from
    ``list_occurrences_device`` (``cpu()`` brings them over)."""

    def __init__(self, rows, ptr, query, induced, graphs: GraphSet, v0: int, v1: int):
        self.rows, self.ptr, self.query, self.induced = rows, ptr, query, induced
        self.k = int(query[0])
        self.v0, self.v1 = v0, v1
        self._graphs = graphs

    def __len__(self):
        return int(self.rows.shape[0])

    def cpu(self) -> "Occurrences":
        if isinstance(self.rows, np.ndarray):
            return self
        return Occurrences(self.rows.cpu().numpy(), self.ptr.cpu().numpy(), self.query, self.induced, self._graphs,
                           self.v0, self.v1)

    @property
    def graph(self) -> np.ndarray:
        """The graph id of every row."""
        rows = self.cpu().rows
        return self._graphs.node_graph_ids()[rows[:, 0]] if len(rows) else np.zeros(0, dtype=np.int32)

    def subsets(self) -> np.ndarray:
        """The rows sorted inside the row: the node SETS of the occurrences (int32 [M, k])."""
        return np.sort(self.cpu().rows, axis=1)

    def table(self) -> dict:
        """{"graph": graph id, "v0" .. "v<k-1>": the images, LOCAL to their graph} -- the driver's CSV columns."""
        rows, graph = self.cpu().rows, self.graph
        first = self._graphs.graph_ptr[:-1][graph].astype(np.int64)
        t = {"graph": graph}
        t.update({f"v{a}": rows[:, a] - first for a in range(self.k)})
        return t


def _one_query(query):
    flat = gt._flatten_queries([query])[0][0]
    return (int(flat[0]), [tuple(int(x) for x in e) for e in flat[1]])


def _resolve(backend: str) -> str:
    if backend not in ("host", "device", "auto", "vf2"):
        raise ValueError(f"unknown backend {backend!r}")
    if backend == "auto":
        backend = _AUTO_BACKEND
    if backend == "device" and not torch.cuda.is_available():
        raise RuntimeError("list_occurrences: backend=\"device\" needs a GPU (there is no fallback)")
    return backend


def _too_many(total: int, max_rows: int):
    return ValueError(f"list_occurrences: {total} occurrences exceed max_rows = {max_rows}; "
                      "iter_occurrences yields them in chunks of at most max_rows rows")


def _chunks(ptr: np.ndarray, max_rows: int):
    """Consecutive anchor ranges [v0, v1) covering [0, N), each with at most max_rows rows and as long as that allows."""
    N, v0 = len(ptr) - 1, 0
    while v0 < N:
        v1 = int(np.searchsorted(ptr, ptr[v0] + max_rows, side="right")) - 1
        if v1 == v0:
            raise ValueError(f"iter_occurrences: node {v0} alone anchors {int(ptr[v0 + 1] - ptr[v0])} occurrences, "
                             f"above max_rows = {max_rows}")
        yield v0, v1
        v0 = v1


# ---- host twin ---------------------------------------------------------------------------------------------------------

class _Host:
    def __init__(self, graphs: GraphSet, query, induced: bool, num_threads: int):
        self.graphs, self.query, self.induced, self.num_threads = graphs, query, bool(induced), int(num_threads)
        self.plan = gt.match_plan([query])
        counts = gt._match_host_int64(graphs, [query], self.induced, self.num_threads)[:, 0]
        self.ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)

    def chunk(self, v0: int, v1: int) -> Occurrences:
        g, ptr = self.graphs, self.ptr
        rows = np.empty((int(ptr[v1] - ptr[v0]), self.query[0]), dtype=np.int32)
        _lib.check(_lib.lib().desco_list_occurrences(
            g.graph_ptr.ctypes.data, g.num_graphs, g.rowptr.ctypes.data, g.col.ctypes.data, self.plan.ctypes.data,
            len(self.plan), int(self.induced), self.num_threads, v0, v1, ptr.ctypes.data, len(rows),
            rows.ctypes.data if len(rows) else None), "desco_list_occurrences")
        return Occurrences(rows, ptr[v0:v1 + 1].copy(), self.query, self.induced, g, v0, v1)


# ---- device ------------------------------------------------------------------------------------------------------------

def sort_segments_device(rows: torch.Tensor) -> torch.Tensor:
    """Rows in segment order: by anchor (the row's maximum), then lexicographically.  k + 1 stable sorts, from the last
    column to the first and then the anchor -- exact, and plumbing: the rows of one anchor already sit together."""
    M, k = rows.shape
    if M < 2:
        return rows
    order = torch.arange(M, device=rows.device)
    for key in [rows[:, c] for c in range(k - 1, -1, -1)] + [rows.max(dim=1).values]:
        order = order[torch.sort(key[order], stable=True).indices]
    return rows[order]


class _Device:
    """One query on one graph set on the device: upload, count pass (the existing matcher entry point), ptr."""

    def __init__(self, graphs: GraphSet, query, induced: bool, dev, slice_entries):
        self.graphs, self.query, self.induced = graphs, query, bool(induced)
        self.dev = torch.device(dev)
        self.plan = gt.match_plan([query])
        A = int(self.plan[1])
        self.slice_entries = int(slice_entries) if slice_entries is not None else max(gt._MATCH_SLICE_WAVES // max(A, 1), 1)
        if self.slice_entries < 1:
            raise ValueError("slice_entries must be positive")
        self.d = gt._DeviceGraphs(graphs, self.dev)
        self.plan_d = self.d.put(self.plan, np.int32)
        self.head = (*self.d.head, self.plan.ctypes.data, self.plan_d.data_ptr(), len(self.plan), 1, int(self.induced))
        N = self.d.N
        self.counts = torch.zeros((N, 1), dtype=torch.int64, device=self.dev)
        self.cursor = torch.zeros(N, dtype=torch.int32, device=self.dev)
        self.overflow = torch.zeros(1, dtype=torch.int32, device=self.dev)
        L = _lib.lib()
        with torch.cuda.device(self.dev):
            stream = torch.cuda.current_stream(self.dev)
            gt._sliced(self.d.E, self.slice_entries, stream, lambda e0, e1: _lib.check(
                L.desco_canonical_counts_match_mode_dev(*self.head, e0, e1, self.counts.data_ptr(), stream.cuda_stream),
                "desco_canonical_counts_match_mode_dev"))
        self.ptr = torch.zeros(N + 1, dtype=torch.int64, device=self.dev)
        torch.cumsum(self.counts[:, 0], 0, out=self.ptr[1:])

    def emit(self, e_begin: int, e_end: int, ptr_base: int, rows: torch.Tensor):
        """The emit launches over the CSR entries [e_begin, e_end), slice by slice, into ``rows`` (first row = row
        ``ptr_base`` of the listing); the stream is synchronised and the status checked after every slice."""
        L = _lib.lib()
        with torch.cuda.device(self.dev):
            stream = torch.cuda.current_stream(self.dev)
            e0 = e_begin
            while True:
                e1 = min(e0 + self.slice_entries, e_end)
                _lib.check(L.desco_list_occurrences_dev(
                    *self.head, e0, e1, self.ptr.data_ptr(), ptr_base, self.cursor.data_ptr(), rows.shape[0],
                    rows.data_ptr() if rows.shape[0] else None, self.overflow.data_ptr(), stream.cuda_stream),
                    "desco_list_occurrences_dev")
                stream.synchronize()            # a fault of this slice surfaces here, before the next is enqueued
                e0 = e1
                if e0 >= e_end:
                    break

    def finish(self, v0: int, v1: int):
        """After the last slice of the anchors [v0, v1): the flag and the cursors must agree with ptr."""
        if int(self.overflow.item()) != 0:
            raise RuntimeError("desco_list_occurrences_dev: a row was suppressed (overflow): ptr and the walk disagree "
                               "-- please report this graph set and query")
        if not torch.equal(self.cursor[v0:v1].to(torch.int64), self.counts[v0:v1, 0]):
            raise RuntimeError("desco_list_occurrences_dev: cursors differ from the counts: ptr and the walk disagree "
                               "-- please report this graph set and query")

    def chunk(self, v0: int, v1: int, lo: int, hi: int) -> Occurrences:
        """The anchors [v0, v1), whose rows are [lo, hi) = [ptr[v0], ptr[v1]) of the listing."""
        rows = torch.empty((hi - lo, self.query[0]), dtype=torch.int32, device=self.dev)
        rowptr = self.graphs.rowptr
        self.emit(int(rowptr[v0]), int(rowptr[v1]), lo, rows)
        self.finish(v0, v1)
        return Occurrences(sort_segments_device(rows), self.ptr[v0:v1 + 1].clone(), self.query, self.induced,
                           self.graphs, v0, v1)


def _device_fits(graphs: GraphSet):
    if int(gt._bitset_words(graphs).sum()) > gt._DEVICE_BITSET_LIMIT_WORDS:
        raise ValueError("list_occurrences: the adjacency bitsets of this graph set exceed the device limit "
                         "(_DEVICE_BITSET_LIMIT_WORDS); use backend=\"host\"")


def list_occurrences_device(graphs: GraphSet, query, induced: bool = True, device="cuda",
                            max_rows: int = _DEFAULT_MAX_ROWS, slice_entries=None) -> Occurrences:
    """``list_occurrences`` on the MI355X, the tensors left on ``device``: the count pass of
    ``canonical_counts_match_device``, its scan, the emit launches of ``desco_list_occurrences_dev`` slice by slice
    (``slice_entries`` CSR entries each; the slicing does not change the result) and the ordering sorts."""
    query = _one_query(query)
    _device_fits(graphs)
    if graphs.num_nodes == 0:
        dev = torch.device(device)
        return Occurrences(torch.zeros((0, query[0]), dtype=torch.int32, device=dev),
                           torch.zeros(1, dtype=torch.int64, device=dev), query, bool(induced), graphs, 0, 0)
    s = _Device(graphs, query, induced, device, slice_entries)
    total = int(s.ptr[-1].item())
    if total > max_rows:
        raise _too_many(total, max_rows)
    return s.chunk(0, s.d.N, 0, total)


# ---- the reference's procedure ------------------------------------------------------------------------------------------

def _vf2(graphs: GraphSet, query, induced: bool) -> Occurrences:
    """networkx VF2 over every graph: of the maps of every occurrence, the one the plan's constraints select.  Hours
    where the native paths take milliseconds; the same bits."""
    import networkx as nx
    GTM_HEAD, GTM_REC, GTM_ANCHOR, GTM_NODE, GTM_LT, GTM_GT = 2, 84, 2, 4, 52, 68       # csrc/groundtruth_match.hpp
    k, edges = query
    plan = gt.match_plan([query])
    recs = [plan[GTM_HEAD + a * GTM_REC: GTM_HEAD + (a + 1) * GTM_REC] for a in range(int(plan[1]))]
    q = nx.Graph()
    q.add_nodes_from(range(k))
    q.add_edges_from(edges)
    GM = nx.algorithms.isomorphism.GraphMatcher
    per_anchor = [[] for _ in range(graphs.num_nodes)]
    for g, (n, es) in enumerate(graphs.edge_lists()):
        base = int(graphs.graph_ptr[g])
        t = nx.Graph()
        t.add_nodes_from(range(n))
        t.add_edges_from(es)
        gm = GM(t, q)
        for vmap in (gm.subgraph_isomorphisms_iter() if induced else gm.subgraph_monomorphisms_iter()):
            f = {a: u for u, a in vmap.items()}
            v = max(f.values())
            for rec in recs:
                if f[int(rec[GTM_ANCHOR])] != v:
                    continue
                img = [f[int(rec[GTM_NODE + i])] for i in range(k)]
                if all((not (int(rec[GTM_LT + i]) >> j & 1) or img[i] < img[j]) and
                       (not (int(rec[GTM_GT + i]) >> j & 1) or img[i] > img[j]) for i in range(k) for j in range(i)):
                    per_anchor[base + v].append(tuple(base + f[a] for a in range(k)))
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in per_anchor])]).astype(np.int64)
    rows = np.array([r for seg in per_anchor for r in sorted(seg)], dtype=np.int32).reshape(-1, k)
    return Occurrences(rows, ptr, query, induced, graphs, 0, graphs.num_nodes)


# ---- public --------------------------------------------------------------------------------------------------------------

def list_occurrences(graphs: GraphSet, query, induced: bool = True, backend: str = "auto", num_threads: int = 0,
                     max_rows: int = _DEFAULT_MAX_ROWS, slice_entries=None) -> Occurrences:
    """Every occurrence of ``query`` (a networkx graph or ``(k, edges)``; connected, loop-free, 2..16 nodes) in
    ``graphs`` as an ``Occurrences`` object on the CPU.
    ``induced=True``: one row per node subset S with G[S] isomorphic to the query; ``induced=False``: one row per copy
    of the query (image edge set).  ``ptr[v + 1] - ptr[v]`` is ``canonical_counts_match`` of the query at ``v``.
    ``backend``: "host" (OpenMP over graphs), "device" (HIP kernel; ``slice_entries`` as in
    ``canonical_counts_match_device``), "vf2" (networkx, the yardstick) or "auto" (see ``_AUTO_BACKEND``);
    ``last_backend`` names the one that served the call.  More than ``max_rows`` occurrences raise ValueError naming the
    total: ``iter_occurrences`` yields them in chunks."""
    global last_backend
    backend = _resolve(backend)
    query = _one_query(query)
    last_backend = backend
    if backend == "vf2":
        gt.match_plan([query])
        return _vf2(graphs, query, bool(induced))
    if backend == "device":
        return list_occurrences_device(graphs, query, induced, max_rows=max_rows, slice_entries=slice_entries).cpu()
    s = _Host(graphs, query, induced, num_threads)
    total = int(s.ptr[-1])
    if total > max_rows:
        raise _too_many(total, max_rows)
    return s.chunk(0, graphs.num_nodes)


def iter_occurrences(graphs: GraphSet, query, induced: bool = True, backend: str = "auto", num_threads: int = 0,
                     max_rows: int = _DEFAULT_MAX_ROWS, slice_entries=None, device="cuda"):
    """``list_occurrences`` in chunks: yields ``Occurrences`` objects over consecutive anchor ranges ``[v0, v1)``, each
    with at most ``max_rows`` rows (CPU arrays); their ``rows`` concatenate to the one-shot listing bit for bit.  An
    anchor range is the window ``rowptr[v0] .. rowptr[v1]`` of CSR entries, emitted into a buffer of its own.  A single
    node that anchors more than ``max_rows`` occurrences raises ValueError naming the node and its count."""
    global last_backend
    backend = _resolve(backend)
    if backend == "vf2":
        raise ValueError("iter_occurrences: backend=\"vf2\" lists in one piece; use list_occurrences")
    if int(max_rows) < 1:
        raise ValueError("max_rows must be positive")
    query = _one_query(query)
    last_backend = backend
    if graphs.num_nodes == 0:
        return
    if backend == "device":
        _device_fits(graphs)
        s = _Device(graphs, query, induced, device, slice_entries)
        ptr = s.ptr.cpu().numpy()
        for v0, v1 in _chunks(ptr, int(max_rows)):
            yield s.chunk(v0, v1, int(ptr[v0]), int(ptr[v1])).cpu()
    else:
        s = _Host(graphs, query, induced, num_threads)
        for v0, v1 in _chunks(s.ptr, int(max_rows)):
            yield s.chunk(v0, v1)
