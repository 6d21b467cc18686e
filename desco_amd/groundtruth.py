"""Exact canonical-count ground truth via the native enumerator (replaces the reference's VF2
process pool, workload.py:551-726)."""
from __future__ import annotations

import ctypes
import functools
from typing import Sequence

import numpy as np
import torch

from . import _lib
from .graphs import GraphSet


def _flatten_queries(queries: Sequence):
    flat = []
    for q in queries:
        if hasattr(q, "nodes"):
            nodes = list(q.nodes)
            idx = {v: i for i, v in enumerate(nodes)}
            flat.append((len(nodes), [(idx[a], idx[b]) for a, b in q.edges()]))
        else:
            flat.append((int(q[0]), [tuple(e) for e in q[1]]))
    q_nodes = np.array([n for n, _ in flat], dtype=np.int32)
    q_edge_ptr = np.concatenate([[0], np.cumsum([len(e) for _, e in flat])]).astype(np.int32)
    q_edges = np.array([x for _, es in flat for e in es for x in e], dtype=np.int32)
    return flat, q_nodes, q_edge_ptr, q_edges


# the device path keeps one adjacency bitset row per node: bounded so that a huge single graph
# (n^2 / 8 bytes) goes to the host enumerator instead
_DEVICE_BITSET_LIMIT_WORDS = 1 << 28        # 2 GiB


def _bitset_words(graphs: GraphSet) -> np.ndarray:
    n = np.diff(graphs.graph_ptr).astype(np.int64)
    return n * ((n + 63) // 64)


def _device_eligible(graphs: GraphSet, q_nodes: np.ndarray) -> bool:
    if not torch.cuda.is_available() or len(q_nodes) == 0 or len(q_nodes) > 32:
        return False
    if q_nodes.min() < 2 or q_nodes.max() > 5:
        return False
    return int(_bitset_words(graphs).sum()) <= _DEVICE_BITSET_LIMIT_WORDS


def _put(a, dt, dev) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)


class _DeviceGraphs:
    """A GraphSet on the device as the enumerators' entry points take it: the CSR, the graph of every node, room for
    the adjacency bitset rows (filled by the entry point), and ``head``, the ten leading ABI arguments."""

    def __init__(self, graphs: GraphSet, dev):
        self.dev = dev
        self._bind(self.put(graphs.graph_ptr, np.int64), self.put(graphs.rowptr, np.int64),
                   self.put(graphs.col, np.int32), self.put(graphs.node_graph_ids(), np.int32), _bitset_words(graphs))

    @classmethod
    def from_device(cls, graph_ptr: torch.Tensor, rowptr: torch.Tensor, col: torch.Tensor, node_graph: torch.Tensor,
                    bitset_words: np.ndarray) -> "_DeviceGraphs":
        """A graph set that is on the device already: contiguous int64 ``graph_ptr`` [G + 1] and ``rowptr`` [N + 1],
        int32 ``col`` [E] (global ids) and ``node_graph`` [N]; ``bitset_words`` (host, per graph) as ``_bitset_words``
        gives it."""
        self = cls.__new__(cls)
        self.dev = col.device
        self._bind(graph_ptr, rowptr, col, node_graph, bitset_words)
        return self

    def _bind(self, graph_ptr, rowptr, col, node_graph, bitset_words):
        bit_off = np.concatenate([[0], np.cumsum(bitset_words)]).astype(np.int64)
        self.N, self.G, self.E = int(rowptr.numel()) - 1, int(graph_ptr.numel()) - 1, int(col.numel())
        self._keep = (graph_ptr, rowptr, col, node_graph, self.put(bit_off[:-1] if self.G else bit_off, np.int64),
                      torch.empty(max(int(bit_off[-1]), 1), dtype=torch.int64, device=self.dev))
        bit_off_d, bits = self._keep[4:]
        self.head = (graph_ptr.data_ptr(), self.G, self.N, rowptr.data_ptr(), self.E,
                     col.data_ptr() if col.numel() else None, node_graph.data_ptr(), bit_off_d.data_ptr(),
                     bits.data_ptr(), int(bit_off[-1]))

    def put(self, a, dt) -> torch.Tensor:
        return _put(a, dt, self.dev)


# name of the backend that served the ESU columns (queries of at most 6 nodes) of the last canonical_counts call:
# "host", "device" (the 2..5-node kernels) or "device6" (the 6-node kernel, canonical_counts6_device)
last_esu_backend = None
# Whether "auto" sends calls with a 6-node column to canonical_counts6_device.  True only if
# tools/bench_groundtruth_six.py shows the device ahead of the host twin (16 threads) on both of its shapes: it does
# (2026-10-21, one MI355X: 46x on COX2-shaped x64, 14x on the Syn_1827-shaped prefix; README).
AUTO_USES_DEVICE6 = True
_DEVICE6_MAX_QUERIES = 142          # every connected class of 2..6 nodes: 1 + 2 + 6 + 21 + 112


def _device6_eligible(graphs: GraphSet, q_nodes: np.ndarray) -> bool:
    """``_device_eligible`` for the 6-node kernel: a GPU, queries of 2..6 nodes, at most 142, bitsets within the limit."""
    if not torch.cuda.is_available() or len(q_nodes) == 0 or len(q_nodes) > _DEVICE6_MAX_QUERIES:
        return False
    if q_nodes.min() < 2 or q_nodes.max() > 6:
        return False
    return int(_bitset_words(graphs).sum()) <= _DEVICE_BITSET_LIMIT_WORDS


def _class_table6(queries: Sequence):
    """``_class_table`` for the 6-node kernel: (int16 [33866], largest query size, number of queries)."""
    _, q_nodes, q_edge_ptr, q_edges = _flatten_queries(queries)
    table = np.empty(33866, dtype=np.int16)
    kmax = ctypes.c_int(0)
    _lib.check(_lib.lib().desco_canonical_class_table6(q_nodes.ctypes.data, q_edge_ptr.ctypes.data,
                                                       q_edges.ctypes.data if len(q_edges) else None,
                                                       len(q_nodes), table.ctypes.data, ctypes.byref(kmax)),
               "desco_canonical_class_table6")
    return table, int(kmax.value), len(q_nodes)


def _census6_on(d: "_DeviceGraphs", table: np.ndarray, kmax: int, Q: int, slice_entries) -> torch.Tensor:
    """The 6-node census kernel on a graph set that is on the device (d.N > 0, Q > 0): int64 [d.N, Q]; one launch per
    slice of the CSR entries, the stream synchronised and the status checked after every slice."""
    slice_entries = _MATCH_SLICE_WAVES if slice_entries is None else int(slice_entries)     # one wave per entry
    if slice_entries < 1:
        raise ValueError("slice_entries must be positive")
    out = torch.empty((d.N, Q), dtype=torch.int64, device=d.dev)
    cls = d.put(table, np.int16)
    L = _lib.lib()
    with torch.cuda.device(d.dev):
        stream = torch.cuda.current_stream(d.dev)
        _sliced(d.E, slice_entries, stream, lambda e0, e1: _lib.check(
            L.desco_canonical_counts6_dev(*d.head, cls.data_ptr(), kmax, Q, e0, e1, out.data_ptr(),
                                          stream.cuda_stream), "desco_canonical_counts6_dev"))
    return out


def canonical_counts6_device(graphs: GraphSet, queries: Sequence, device="cuda", induced: bool = True,
                             slice_entries=None) -> torch.Tensor:
    """The counts of ``canonical_counts`` for queries of 2..6 nodes computed on the MI355X by the ESU walk at depth six
    (csrc/groundtruth6_dev.hip): every column in ONE walk.  Returns a [num_nodes, num_queries] int64 tensor on
    ``device``, bit-identical to the host enumerator.
    ``induced=True``: the queries are pairwise non-isomorphic and at most 142 (every connected class of 2..6 nodes).
    ``induced=False``: the non-induced counts of any number of queries, duplicates included: the census of all classes
    of the queries' sizes in one walk, then ``desco_canonical_noninduced_transform_dev`` in chunks of 32 classes.
    The CSR entries are cut into slices of ``slice_entries`` (default ``_MATCH_SLICE_WAVES``: one wave per entry), one
    launch each; the slicing does not change the result.  Empty graph sets and no queries give zeros without a launch.
    Raises RuntimeError naming "2..6 nodes" or "isomorphic" for queries it does not take."""
    dev = torch.device(device)
    flat = _flatten_queries(queries)[0]
    if any(n < 2 or n > 6 for n, _ in flat):
        raise RuntimeError("canonical_counts6_device: queries must have 2..6 nodes")
    if not induced:
        out = torch.zeros((graphs.num_nodes, len(flat)), dtype=torch.int64, device=dev)
        if not flat:
            return out
        groups = _census_plan(flat)                 # (refuses disconnected queries and loops)
        if graphs.num_nodes == 0:
            return out
        classes = [c for cl, _, _ in groups for c in cl]
        census = canonical_counts6_device(graphs, classes, dev, slice_entries=slice_entries)
        c_first = 0
        for cl, idx, m in groups:                   # (a size's classes only feed that size's columns)
            part = torch.empty((graphs.num_nodes, len(idx)), dtype=torch.int64, device=dev)
            for c0 in range(0, len(cl), 32):
                c1 = min(c0 + 32, len(cl))
                _transform_device(census[:, c_first + c0:c_first + c1], m[c0:c1], part, c0 > 0)
            out[:, torch.tensor(idx, device=dev)] = part
            c_first += len(cl)
        return out
    table, kmax, Q = _class_table6(flat)
    if graphs.num_nodes == 0 or Q == 0:
        return torch.zeros((graphs.num_nodes, Q), dtype=torch.int64, device=dev)
    return _census6_on(_DeviceGraphs(graphs, dev), table, kmax, Q, slice_entries)


def canonical_counts_device(graphs: GraphSet, queries: Sequence, device="cuda", induced: bool = True) -> torch.Tensor:
    """The counts of ``canonical_counts`` computed on the MI355X (csrc/groundtruth_dev.hip):
    queries of 2..5 nodes, at most 32, pairwise non-isomorphic.  Returns a [num_nodes, num_queries]
    int64 tensor on ``device``.  (6-node queries are refused here, naming "2..5 nodes": they are
    ``canonical_counts6_device``'s.)
    ``induced=False``: the non-induced counts (see ``canonical_counts``) of queries of 2..5 nodes, any number of them,
    duplicates included: the census of all connected classes of the queries' sizes by the same kernel, then the exact
    int64 transform on the device (``desco_canonical_noninduced_transform_dev``), without a round trip."""
    if not induced:
        return _noninduced_device(graphs, _flatten_queries(queries)[0], torch.device(device))
    dev = torch.device(device)
    table, kmax, Q = _class_table(queries)
    if graphs.num_nodes == 0 or Q == 0:
        return torch.zeros((graphs.num_nodes, Q), dtype=torch.int64, device=dev)
    return _census_on(_DeviceGraphs(graphs, dev), table, kmax, Q)


def _class_table(queries: Sequence):
    """(int16 [1098] class table of the census kernel, its largest query size, the number of queries); refuses what
    the kernel does not take, naming the reason."""
    _, q_nodes, q_edge_ptr, q_edges = _flatten_queries(queries)
    table = np.empty(1098, dtype=np.int16)
    kmax = ctypes.c_int(0)
    _lib.check(_lib.lib().desco_canonical_class_table(q_nodes.ctypes.data, q_edge_ptr.ctypes.data,
                                                      q_edges.ctypes.data if len(q_edges) else None,
                                                      len(q_nodes), table.ctypes.data, ctypes.byref(kmax)),
               "desco_canonical_class_table")
    return table, int(kmax.value), len(q_nodes)


def _census_on(d: _DeviceGraphs, table: np.ndarray, kmax: int, Q: int) -> torch.Tensor:
    """The induced census kernel on a graph set that is on the device (d.N > 0, Q > 0): int64 [d.N, Q]."""
    out = torch.empty((d.N, Q), dtype=torch.int64, device=d.dev)
    cls = d.put(table, np.int16)
    with torch.cuda.device(d.dev):
        _lib.check(_lib.lib().desco_canonical_counts_dev(*d.head, cls.data_ptr(), kmax, Q, out.data_ptr(),
                                                         torch.cuda.current_stream(d.dev).cuda_stream),
                   "desco_canonical_counts_dev")
    return out


def canonical_counts(graphs: GraphSet, queries: Sequence, num_threads: int = 0,
                     backend: str = "auto", induced: bool = True, method: str = "auto") -> torch.Tensor:
    """[num_nodes, num_queries] float tensor of canonical counts (the reference stores doubles).
    ``queries``: networkx graphs or (n, edges) pairs, connected, 2..16 nodes.
    ``backend``: "host" (OpenMP), "device" (HIP kernels), "auto", or "vf2" (the reference's procedure in Python:
    the yardstick of the tests and the way out for queries above 16 nodes).
    Columns of queries with at most 6 nodes go to the ESU enumerators -- "auto": the device when a GPU is present
    and the queries fit its path (2..5 nodes, <= 32, distinct classes), else the host; a call with a 6-node column
    sends ALL its columns of at most 6 nodes to ``canonical_counts6_device`` in one walk when ``AUTO_USES_DEVICE6``
    and the set is eligible (a GPU, bitsets within the limit, at most 142 distinct classes), else to the host.
    ``last_esu_backend`` names the one that served them ("host", "device", "device6").  ``backend="device"`` keeps
    meaning the 2..5-node kernels and refuses a 6-node query naming "2..5 nodes": ask ``canonical_counts6_device``.
    Columns of larger queries
    go to the matcher (``canonical_counts_match``) with the same ``backend``; the results are joined in query order.
    ``induced=False``: NON-INDUCED counts, count[v][q] = #{injective f : f maps every edge of q onto an edge of G,
    max(im f) = v} / |Aut(q)| -- occurrences that need only CONTAIN the query's edges (P3 in a triangle: 3, all at the
    largest node).  Columns of at most 6 nodes come from the census of all connected classes of that size, run where
    induced columns of that size run, and the exact int64 transform ``noninduced_matrix``; larger ones from the
    matcher's non-induced mode; "vf2" is ``subgraph_monomorphisms_iter`` keyed and divided the same way.
    ``method``: "auto" (the routing above) or "matcher" (every size to the matcher, to compare the two native routes)."""
    if method not in ("auto", "matcher"):
        raise ValueError(f"unknown method {method!r}")
    if backend == "vf2":
        return _canonical_counts_vf2(graphs, queries, induced)
    if not induced and backend not in ("auto", "host", "device"):
        raise ValueError(f"unknown backend {backend!r}")
    flat, q_nodes, _, _ = _flatten_queries(queries)
    if method == "matcher":
        return canonical_counts_match(graphs, flat, backend, num_threads, induced=induced)
    large = [i for i, k in enumerate(q_nodes) if k > 6]
    if large:
        small = [i for i, k in enumerate(q_nodes) if k <= 6]
        out = torch.zeros((graphs.num_nodes, len(flat)), dtype=torch.double)
        out[:, large] = canonical_counts_match(graphs, [flat[i] for i in large], backend, num_threads, induced=induced)
        if small:
            out[:, small] = canonical_counts(graphs, [flat[i] for i in small], num_threads, backend, induced)
        return out
    global last_esu_backend
    if not induced:
        return _noninduced_small(graphs, flat, backend, num_threads)
    if backend == "auto" and _auto_device6(graphs, q_nodes):        # a 6-node column: every column in one walk
        try:
            out = canonical_counts6_device(graphs, flat).cpu().double()
            last_esu_backend = "device6"
            return out
        except RuntimeError as e:
            if "isomorphic" not in str(e):
                raise                           # (duplicate query classes: host path below)
    if backend == "device" or (backend == "auto" and _device_eligible(graphs, q_nodes)):
        try:
            out = canonical_counts_device(graphs, queries).cpu().double()
            last_esu_backend = "device"
            return out
        except RuntimeError as e:
            if backend == "device" or "isomorphic" not in str(e):
                raise                           # (duplicate query classes: host path below)
    out = torch.from_numpy(_induced_host_int64(graphs, flat, num_threads)).double()
    last_esu_backend = "host"
    return out


def _auto_device6(graphs: GraphSet, q_nodes: np.ndarray) -> bool:
    """Whether "auto" sends these ESU columns (at most 6 nodes) to the 6-node kernel: the measured switch, a 6-node
    column among them, and the set eligible.  Calls without a 6-node column go where they went."""
    return bool(AUTO_USES_DEVICE6 and len(q_nodes) and q_nodes.max() == 6 and _device6_eligible(graphs, q_nodes))


# ---- non-induced counts of small queries: census of all classes + an exact transform ---------------------------------
@functools.lru_cache(maxsize=None)
def census_classes(k: int):
    """All connected k-node graphs, k = 2..6, as a tuple of (k, edges) in graph-atlas order: 1, 2, 6, 21 and 112."""
    if k == 2:
        return ((2, ((0, 1),)),)
    if not 3 <= k <= 6:
        raise ValueError("census classes exist for 2..6 nodes")
    from .data import gen_query_ids, graph_atlas_plus
    return tuple((k, tuple(tuple(e) for e in graph_atlas_plus(i).edges())) for i in gen_query_ids([k]))


_occurrence_rows = {}               # (k, sorted edges) -> int64 [number of classes]: computed once per process


def _noninduced_rows(flat) -> np.ndarray:
    """int64 [len(flat), number of k-node classes], rows M_k[q][:] of queries ``flat`` that all have k nodes (2..6):
    the occurrences of q in every class representative, by the host matcher's non-induced mode."""
    k = int(flat[0][0])
    classes = census_classes(k)
    keys = [(k, tuple(sorted((min(a, b), max(a, b)) for a, b in edges))) for _, edges in flat]
    todo = sorted({key for key in keys if key not in _occurrence_rows})
    if todo:
        reps = GraphSet.from_edge_lists([(n, list(e)) for n, e in classes])
        counts = _match_host_int64(reps, [(n, list(e)) for n, e in todo], False, 1)
        per_class = counts.reshape(len(classes), k, len(todo)).sum(axis=1)
        for j, key in enumerate(todo):
            _occurrence_rows[key] = np.ascontiguousarray(per_class[:, j])
    return np.stack([_occurrence_rows[key] for key in keys])


def noninduced_matrix(k: int) -> np.ndarray:
    """M_k, int64 [C, C] over ``census_classes(k)``: M_k[q][c] = the occurrences of class q in class c as a not
    necessarily induced subgraph.  noninduced[v][q] = sum_c M_k[q][c] * induced[v][c]: a k-subset whose induced
    subgraph is c holds M_k[q][c] occurrences of q, and ESU visits every connected k-subset once."""
    return _noninduced_rows([(n, list(e)) for n, e in census_classes(k)])


def _census_plan(flat):
    """Checks the queries (the matcher's plan refuses what is not connected, loop-free, of 2..16 nodes) and returns
    [(classes, query indices, M rows)] per census call: the sizes 2..5 together (30 classes at most), size 6 apart."""
    match_plan(flat)
    groups = []
    for sizes in ((2, 3, 4, 5), (6,)):
        classes, idx, blocks = [], [], []
        for k in sizes:
            mine = [i for i, (n, _) in enumerate(flat) if n == k]
            if mine:
                blocks.append((len(classes), mine, _noninduced_rows([flat[i] for i in mine])))
                classes += [(n, list(e)) for n, e in census_classes(k)]
                idx += mine
        if idx:
            m = np.zeros((len(classes), len(idx)), dtype=np.int64)          # [C, Q]: zero across sizes
            col = 0
            for c0, mine, rows in blocks:
                m[c0:c0 + rows.shape[1], col:col + len(mine)] = rows.T
                col += len(mine)
            groups.append((classes, idx, m))
    return groups


def _transform_device(census: torch.Tensor, m: np.ndarray, out: torch.Tensor, accumulate: bool):
    """out[:, :] (+)= census @ m on the device, int64: census [N, C <= 32], m [C, Q], out [N, Q]; Q in chunks of 64."""
    L = _lib.lib()
    dev = census.device
    N, C = census.shape
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        for q0 in range(0, m.shape[1], 64):
            q1 = min(q0 + 64, m.shape[1])
            m_d = torch.from_numpy(np.ascontiguousarray(m[:, q0:q1])).to(dev)
            _lib.check(L.desco_canonical_noninduced_transform_dev(
                census.data_ptr(), census.stride(0), m_d.data_ptr(), N, C, q1 - q0, int(accumulate),
                out.data_ptr() + 8 * q0, out.stride(0), stream), "desco_canonical_noninduced_transform_dev")
            torch.cuda.current_stream(dev).synchronize()        # m_d is released when this iteration ends


def noninduced_transform_device(census: torch.Tensor, m, accumulate_into=None) -> torch.Tensor:
    """``census`` [N, C] int64 on the GPU times ``m`` [C, Q] int64 (numpy or tensor), modulo 2^64, by the HIP kernel of
    ``canonical_counts_device(induced=False)``: C of 1..32, any Q.  Returns the [N, Q] int64 tensor on the census's
    device; with ``accumulate_into`` (such a tensor) the product is added to it."""
    if not census.is_cuda:
        raise RuntimeError("noninduced_transform_device: no CPU fallback (the host route uses numpy int64)")
    m = np.ascontiguousarray(m.cpu().numpy() if isinstance(m, torch.Tensor) else m, dtype=np.int64)
    census = census.contiguous()
    if census.dtype != torch.int64 or census.dim() != 2 or m.ndim != 2 or m.shape[0] != census.shape[1]:
        raise ValueError("noninduced_transform_device: census [N, C] int64 and m [C, Q] int64")
    out = accumulate_into if accumulate_into is not None else \
        torch.empty((census.shape[0], m.shape[1]), dtype=torch.int64, device=census.device)
    if out.shape != (census.shape[0], m.shape[1]) or out.dtype != torch.int64 or out.stride(1) != 1:
        raise ValueError("noninduced_transform_device: accumulate_into must be [N, Q] int64 with unit column stride")
    if census.shape[0] and m.shape[1]:
        _transform_device(census, m, out, accumulate_into is not None)
    return out


def _noninduced_device(graphs: GraphSet, flat, dev) -> torch.Tensor:
    """[num_nodes, len(flat)] int64 on ``dev``: device census of the classes, 32 per call, and the transform kernel."""
    out = torch.zeros((graphs.num_nodes, len(flat)), dtype=torch.int64, device=dev)
    if not flat:
        return out
    groups = _census_plan(flat)
    if max(n for n, _ in flat) > 5:
        raise RuntimeError("canonical_counts_device: the device path takes queries of 2..5 nodes")
    if graphs.num_nodes == 0:
        return out
    for classes, idx, m in groups:
        part = torch.zeros((graphs.num_nodes, len(idx)), dtype=torch.int64, device=dev)
        for c0 in range(0, len(classes), 32):
            census = canonical_counts_device(graphs, classes[c0:c0 + 32], dev)
            _transform_device(census, m[c0:c0 + 32], part, c0 > 0)
        out[:, torch.tensor(idx, device=dev)] = part
    return out


def _noninduced_small(graphs: GraphSet, flat, backend: str, num_threads: int) -> torch.Tensor:
    """Non-induced counts of queries of at most 6 nodes as a [num_nodes, len(flat)] double tensor on the CPU.  The census
    of a size goes where induced columns of that size go: the device when ``backend`` says so or "auto" finds the
    classes eligible (2..5 nodes, a GPU, bitsets within the limit), else the host enumerator and numpy int64.  "auto" with
    a 6-node query: every size in one walk of the 6-node kernel (``canonical_counts6_device(induced=False)``) when
    ``AUTO_USES_DEVICE6`` and the set is eligible.  Sets ``last_esu_backend``."""
    global last_esu_backend
    # (any number of queries: what the kernel counts are the classes of their sizes, 142 at most)
    if backend == "auto" and _auto_device6(graphs, np.array(sorted({n for n, _ in flat}), dtype=np.int32)):
        last_esu_backend = "device6"                # a 6-node column: the census of every size in one walk
        return canonical_counts6_device(graphs, flat, induced=False).cpu().double()
    out = np.zeros((graphs.num_nodes, len(flat)), dtype=np.int64)
    served = set()
    for classes, idx, m in _census_plan(flat):
        sizes = np.array([n for n, _ in classes], dtype=np.int32)
        if backend == "device" or (backend == "auto" and _device_eligible(graphs, sizes[:32])):
            out[:, idx] = _noninduced_device(graphs, [flat[i] for i in idx], torch.device("cuda")).cpu().numpy()
            served.add("device")
        else:
            out[:, idx] = _induced_host_int64(graphs, classes, num_threads) @ m
            served.add("host")
    if served:                                      # (a call served by both names the host: its census is the larger)
        last_esu_backend = "host" if "host" in served else "device"
    return torch.from_numpy(out).double()


def _induced_host_int64(graphs: GraphSet, flat, num_threads: int) -> np.ndarray:
    """The host ESU enumerator (desco_canonical_counts) on queries of 2..6 nodes: int64 [num_nodes, len(flat)]."""
    _, q_nodes, q_edge_ptr, q_edges = _flatten_queries(flat)
    out = np.zeros((graphs.num_nodes, len(flat)), dtype=np.int64)
    _lib.check(_lib.lib().desco_canonical_counts(graphs.graph_ptr.ctypes.data, graphs.num_graphs,
                                                 graphs.rowptr.ctypes.data, graphs.col.ctypes.data,
                                                 q_nodes.ctypes.data, q_edge_ptr.ctypes.data,
                                                 q_edges.ctypes.data if len(q_edges) else None, len(flat),
                                                 num_threads, out.ctypes.data), "desco_canonical_counts")
    return out


# ---- orbit counts (graphlet degree vectors) ---------------------------------------------------------------------------
# Definitions (include/desco_hip.h, "ORBIT COUNTS"):
#   query: connected, loop-free, 2..5 nodes; an nx.Graph whose positions are list(q.nodes), or (n, edges)
#   orbits of a query: the orbits of Aut(q) on its node positions, numbered in ascending order of their smallest member
#   induced:      orbit[v][(q,o)] = #{S containing v : G[S] isomorphic to q by a map that takes v into orbit o}
#   non-induced:  #{injective edge-preserving f : q -> G with v in f(orbit o)} / |Aut(q)|: copies of q (a copy being its
#                 edge set) in which v plays role o
#   columns: the queries in the given order and, inside a query, its orbits in order; queries=None means
#            census_classes(2) + .. + census_classes(5): 30 classes, 1 + 3 + 11 + 58 = 73 columns.  The numbering is
#            this project's own (it is not ORCA's).
#   per graph, sum_v orbit[v][(q,o)] = |o| * sum_v canonical_counts[v][q] (both forms); the 2-node column is the degree;
#   relabelling the nodes of G permutes the rows and changes nothing else.
def _pair_bit(a, b):
    return b * (b - 1) // 2 + a if a < b else a * (a - 1) // 2 + b


@functools.lru_cache(maxsize=None)
def _perms(k: int):
    import itertools
    return tuple(itertools.permutations(range(k)))


def _relabelled_mask(edges, p) -> int:
    m = 0
    for a, b in edges:
        m |= 1 << _pair_bit(p[a], p[b])
    return m


@functools.lru_cache(maxsize=None)
def _orbit_structure(k: int, edges: tuple):
    """(orbit index of every position, member positions of every orbit, canonical mask, a relabelling that gives it)
    of the graph (k, edges); refuses nothing (the callers have checked the query)."""
    mask = _relabelled_mask(edges, range(k))
    low = list(range(k))
    best, best_p = None, None
    for p in _perms(k):
        r = _relabelled_mask(edges, p)
        if r == mask:
            low = [min(x, y) for x, y in zip(low, p)]
        if best is None or r < best:
            best, best_p = r, p
    firsts = sorted(set(low))
    orbit_of = tuple(firsts.index(x) for x in low)
    members = tuple(tuple(i for i in range(k) if orbit_of[i] == o) for o in range(len(firsts)))
    return orbit_of, members, best, best_p


def _orbit_queries(queries, what="orbit counts"):
    """The flattened, checked queries of an orbit call: [(k, edge tuple)]."""
    if queries is None:
        return [(k, tuple(e)) for k in (2, 3, 4, 5) for _, e in census_classes(k)]
    flat = _flatten_queries(queries)[0]
    if any(n < 2 or n > 5 for n, _ in flat):
        raise RuntimeError(what + " take queries of 2..5 nodes")
    if flat:
        match_plan(flat)                # refuses disconnected queries and loops, naming the reason
    return [(n, tuple((int(a), int(b)) for a, b in e)) for n, e in flat]


def orbit_columns(queries=None):
    """The columns of ``orbit_counts``: a list of (query index, orbit index, member positions).  ``queries=None``: the
    30 connected graphs of 2..5 nodes in ``census_classes`` order, 73 columns."""
    return [(qi, o, mem) for qi, (k, e) in enumerate(_orbit_queries(queries))
            for o, mem in enumerate(_orbit_structure(k, e)[1])]


@functools.lru_cache(maxsize=None)
def _census_class_of_mask(k: int):
    """canonical mask -> class index in census_classes(k)"""
    return {_orbit_structure(k, tuple(e))[2]: ci for ci, (_, e) in enumerate(census_classes(k))}


def _orbit_select(flat, induced):
    """Every query is computed as its census class (so that duplicates and isomorphic queries cost nothing and the C
    routines get pairwise non-isomorphic ones) and its columns are mapped back through the position relabelling.
    Returns (reps, index, sizes, first, width): the class representatives handed to the enumerators (size by size, in
    census order: the classes in use, or for the non-induced form the whole census of every size in use), the index of
    every output column among the enumerators' columns, the sizes in use and, per size, the first of its columns and
    their number."""
    wanted = []                                      # per output column: (k, class, orbit of the class)
    for k, e in flat:
        _, members, canon, p = _orbit_structure(k, e)
        ci = _census_class_of_mask(k)[canon]
        rep_orbit_of, _, _, r = _orbit_structure(k, tuple(census_classes(k)[ci][1]))
        r_inv = {x: i for i, x in enumerate(r)}      # query position a -> canonical p[a] -> class position r^-1(p[a])
        wanted += [(k, ci, rep_orbit_of[r_inv[p[mem[0]]]]) for mem in members]
    return _class_columns(wanted, induced, lambda k, e: len(_orbit_structure(k, e)[1]))


def _class_columns(wanted, induced, orbits_of):
    """The second half of ``_orbit_select``, for node and edge orbits alike: ``wanted`` = per output column (k, class,
    orbit of the class), ``orbits_of(k, edges)`` = the number of orbits of a class representative."""
    sizes = sorted({k for k, _, _ in wanted})
    used = {(k, ci) for k, ci, _ in wanted}
    reps, start, first, width, col = [], {}, {}, {}, 0
    for k in sizes:
        first[k] = col
        for ci, (_, e) in enumerate(census_classes(k)):
            if induced and (k, ci) not in used:
                continue
            reps.append((k, list(e)))
            start[(k, ci)] = col
            col += orbits_of(k, tuple(e))
        width[k] = col - first[k]
    index = np.array([start[(k, ci)] + o for k, ci, o in wanted], dtype=np.int64)
    return reps, index, sizes, first, width


_orbit_transform = {}               # k -> int64 [columns of size k, columns of size k]: computed once per process


def orbit_noninduced_matrix(k: int) -> np.ndarray:
    """T_k, int64 [C_k, C_k] over the orbit columns of ``census_classes(k)``: T_k[(c,o')][(q,o)] = the copies of q in
    the class representative c in which one fixed node of orbit o' has role o.  noninduced = induced @ T_k (a k-subset
    whose induced subgraph is c, seen from a node of orbit o', holds that many copies of q with the node in role o).
    By exhaustive enumeration of the k! maps of every pair of classes."""
    if k not in _orbit_transform:
        classes = [(tuple(e), _orbit_structure(k, tuple(e))) for _, e in census_classes(k)]
        starts = np.concatenate([[0], np.cumsum([len(st[1]) for _, st in classes])])
        T = np.zeros((starts[-1], starts[-1]), dtype=np.int64)
        for qi, (qe, (q_orbit_of, _, _, _)) in enumerate(classes):
            aut = sum(1 for p in _perms(k) if _relabelled_mask(qe, p) == _relabelled_mask(qe, range(k)))
            for ci, (ce, (_, c_members, _, _)) in enumerate(classes):
                cmask = _relabelled_mask(ce, range(k))
                hits = np.zeros((k, len(set(q_orbit_of))), dtype=np.int64)        # [node of c][role]
                for f in _perms(k):
                    if _relabelled_mask(qe, f) & ~cmask == 0:
                        for a in range(k):
                            hits[f[a], q_orbit_of[a]] += 1
                for o2, mem in enumerate(c_members):
                    assert (hits[list(mem)] == hits[mem[0]]).all() and (hits[mem[0]] % aut == 0).all()
                    T[starts[ci] + o2, starts[qi]:starts[qi + 1]] = hits[mem[0]] // aut
        _orbit_transform[k] = T
    return _orbit_transform[k]


def _orbit_table(reps):
    _, q_nodes, q_edge_ptr, q_edges = _flatten_queries(reps)
    table = np.empty((1098, 5), dtype=np.int16)
    ncol, kmax = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(_lib.lib().desco_orbit_table(q_nodes.ctypes.data, q_edge_ptr.ctypes.data,
                                            q_edges.ctypes.data if len(q_edges) else None, len(q_nodes),
                                            table.ctypes.data, ctypes.byref(ncol), ctypes.byref(kmax)),
               "desco_orbit_table")
    return table, int(ncol.value), int(kmax.value)


def _orbit_device_raw(graphs: GraphSet, reps, dev) -> torch.Tensor:
    """desco_orbit_counts_dev on pairwise non-isomorphic ``reps``: int64 [N, columns of reps] on ``dev``."""
    table, C, kmax = _orbit_table(reps)
    out = torch.empty((graphs.num_nodes, C), dtype=torch.int64, device=dev)
    if graphs.num_nodes == 0 or C == 0:
        return out.zero_()
    d = _DeviceGraphs(graphs, dev)
    table_d = d.put(table, np.int16)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().desco_orbit_counts_dev(*d.head, table_d.data_ptr(), kmax, C, out.data_ptr(),
                                                     torch.cuda.current_stream(dev).cuda_stream),
                   "desco_orbit_counts_dev")
    return out


def _orbit_host_raw(graphs: GraphSet, reps, num_threads: int) -> np.ndarray:
    """desco_orbit_counts on pairwise non-isomorphic ``reps``: int64 [N, columns of reps]."""
    _, q_nodes, q_edge_ptr, q_edges = _flatten_queries(reps)
    out = np.zeros((graphs.num_nodes, _orbit_table(reps)[1]), dtype=np.int64)
    _lib.check(_lib.lib().desco_orbit_counts(graphs.graph_ptr.ctypes.data, graphs.num_graphs,
                                             graphs.rowptr.ctypes.data, graphs.col.ctypes.data,
                                             q_nodes.ctypes.data, q_edge_ptr.ctypes.data,
                                             q_edges.ctypes.data if len(q_edges) else None, len(reps),
                                             num_threads, out.ctypes.data), "desco_orbit_counts")
    return out


def orbit_counts_device(graphs: GraphSet, queries=None, device="cuda", induced: bool = True) -> torch.Tensor:
    """Exact per-node orbit counts (definitions above) on the MI355X (csrc/groundtruth_dev.hip, go_count_kernel):
    int64 [num_nodes, len(orbit_columns(queries))] on ``device``.  Duplicate and isomorphic queries are accepted: every
    class is enumerated once.  ``induced=False``: the orbit census of the queries' sizes by the same kernel, then the
    exact int64 transform ``orbit_noninduced_matrix`` with ``desco_canonical_noninduced_transform_dev`` (source columns
    in chunks of 32), without a round trip."""
    flat = _orbit_queries(queries)
    dev = torch.device(device)
    if not flat:
        return torch.zeros((graphs.num_nodes, 0), dtype=torch.int64, device=dev)
    reps, index, sizes, first, width = _orbit_select(flat, induced)
    raw = _orbit_device_raw(graphs, reps, dev)
    if not induced and graphs.num_nodes:
        full = torch.zeros_like(raw)
        for k in sizes:
            T = orbit_noninduced_matrix(k)
            src, dst = raw[:, first[k]:first[k] + width[k]], full[:, first[k]:first[k] + width[k]]
            for c0 in range(0, width[k], 32):
                _transform_device(src[:, c0:c0 + 32], T[c0:c0 + 32], dst, c0 > 0)
        raw = full
    return raw.index_select(1, torch.from_numpy(index).to(dev))


def orbit_counts(graphs: GraphSet, queries=None, num_threads: int = 0, backend: str = "auto",
                 induced: bool = True, per_query: bool = False) -> torch.Tensor:
    """Exact per-node orbit counts -- the graphlet degree vector when ``queries`` is None (73 columns) -- as a double
    [num_nodes, len(orbit_columns(queries))] tensor on the CPU (definitions above; ``canonical_counts`` returns doubles
    too).  ``backend``: "host" (OpenMP over graphs, ``num_threads`` threads), "device" (``orbit_counts_device``) or
    "auto": the device when a GPU is present and the adjacency bitsets fit ``_DEVICE_BITSET_LIMIT_WORDS``.
    ``induced=False``: the non-induced form.  ``per_query=True``: the orbits of every query summed, [num_nodes,
    num_queries]: the occurrences of the query that contain v.  Raises RuntimeError for queries outside 2..5 nodes and
    for disconnected or looped ones."""
    if backend not in ("auto", "host", "device"):
        raise ValueError(f"unknown backend {backend!r}")
    flat = _orbit_queries(queries)
    if backend == "auto":       # _device_eligible's conditions: a GPU and bitsets within the limit (the sizes are checked)
        backend = "device" if flat and _device_eligible(graphs, np.array([2], dtype=np.int32)) else "host"
    if backend == "device":
        out = orbit_counts_device(graphs, flat, induced=induced).cpu()
    elif not flat:
        out = torch.zeros((graphs.num_nodes, 0), dtype=torch.int64)
    else:
        reps, index, sizes, first, width = _orbit_select(flat, induced)
        raw = _orbit_host_raw(graphs, reps, num_threads)
        if not induced:
            raw = np.concatenate([raw[:, first[k]:first[k] + width[k]] @ orbit_noninduced_matrix(k) for k in sizes],
                                 axis=1)
        out = torch.from_numpy(np.ascontiguousarray(raw[:, index]))
    if per_query:
        owner = torch.tensor([qi for qi, _, _ in orbit_columns(flat)], dtype=torch.long)
        summed = torch.zeros((out.shape[0], len(flat)), dtype=torch.int64)
        out = summed.index_add_(1, owner, out)
    return out.double()


# ---- edge orbit counts (edge graphlet degree vectors) ------------------------------------------------------------------
# Definitions (include/desco_hip.h, "EDGE ORBIT COUNTS"):
#   query: connected, loop-free, 2..5 nodes; an nx.Graph whose positions are list(q.nodes), or (n, edges)
#   edge orbits of a query: the orbits of Aut(q) on its edge set; the edges are ordered by pair_bit(a, b) = b(b-1)/2 + a
#                 (a < b) and the orbits numbered in ascending order of their smallest member
#   rows: one per undirected edge of the GraphSet, in the order of the CSR entries (v, u) with u < v (ascending v, then
#                 ascending u: the work items of the ESU walk); ``edge_orbit_rows`` gives their endpoints
#   induced:      eorb[e][(q,o)] = #{connected S containing both ends of e : G[S] isomorphic to q by a map that takes e
#                 into orbit o}
#   non-induced:  #{injective edge-preserving f : q -> G with e in f(orbit o)} / |Aut(q)|: copies of q (a copy being its
#                 edge set) in which e is an edge of the copy and plays role o
#   columns: the queries in the given order and, inside a query, its edge orbits in order; queries=None means
#            census_classes(2) + .. + census_classes(5): 30 classes, 1 + 2 + 10 + 56 = 69 columns.  The numbering is this
#            project's own (ORCA's 68 edge orbits leave out the single edge).
#   both forms: per graph, sum_e eorb[e][(q,o)] = |o| * sum_v canonical_counts[v][q]; the 2-node column is 1; the
#   triangle column is the number of common neighbours of the ends; the P3 column is deg(a) + deg(b) - 2 (induced: less
#   twice the triangles); for every node v, sum_{e at v} eorb[e][(q,o)] = sum_p orbit_counts[v][(q,p)] * inc_q[p][o] with
#   inc_q[p][o] = the edges of orbit o at a node of node orbit p; relabelling the nodes of G permutes the rows.
@functools.lru_cache(maxsize=None)
def _edge_orbit_structure(k: int, edges: tuple):
    """({edge (a, b), a < b: its orbit}, member edges of every orbit in pair-bit order) of the graph (k, edges)."""
    mine = sorted({(min(a, b), max(a, b)) for a, b in edges}, key=lambda e: _pair_bit(*e))
    mask = _relabelled_mask(edges, range(k))
    low = {e: _pair_bit(*e) for e in mine}
    for p in _perms(k):
        if _relabelled_mask(edges, p) == mask:
            for a, b in mine:
                low[(a, b)] = min(low[(a, b)], _pair_bit(p[a], p[b]))
    firsts = sorted(set(low.values()))
    orbit_of = {e: firsts.index(low[e]) for e in mine}
    return orbit_of, tuple(tuple(e for e in mine if orbit_of[e] == o) for o in range(len(firsts)))


def edge_orbit_columns(queries=None):
    """The columns of ``edge_orbit_counts``: a list of (query index, orbit index, member edges (a, b) with a < b).
    ``queries=None``: the 30 connected graphs of 2..5 nodes in ``census_classes`` order, 69 columns."""
    return [(qi, o, mem) for qi, (k, e) in enumerate(_orbit_queries(queries, "edge orbit counts"))
            for o, mem in enumerate(_edge_orbit_structure(k, e)[1])]


def edge_orbit_rows(graphs: GraphSet) -> torch.Tensor:
    """The rows of ``edge_orbit_counts``: int64 [M, 2], the endpoints (u, v), u < v, global ids, of every undirected
    edge in the order of the CSR entries (v, u) with u < v."""
    rows = np.repeat(np.arange(graphs.num_nodes, dtype=np.int64), np.diff(graphs.rowptr))
    col = np.asarray(graphs.col, dtype=np.int64)
    lower = col < rows
    return torch.from_numpy(np.stack([col[lower], rows[lower]], axis=1))


def _num_edges(graphs: GraphSet) -> int:
    """M, the number of rows: the CSR entries (v, u) with u < v."""
    rows = np.repeat(np.arange(graphs.num_nodes, dtype=np.int64), np.diff(graphs.rowptr))
    return int((np.asarray(graphs.col) < rows).sum())


def _entry_rows_device(d: "_DeviceGraphs"):
    """(int32 [E] on the device: the row of the edge of every CSR entry, both directions of an edge naming one row; M).
    Index plumbing on the device (the CSR is there already): a lower entry's row is its rank among the lower entries;
    an upper entry (v, u) takes the row of its twin (u, v), found among the ascending keys of the lower entries."""
    _, rowptr, col = d._keep[:3]
    if d.E == 0:
        return torch.zeros(0, dtype=torch.int32, device=d.dev), 0
    rows = torch.repeat_interleave(torch.arange(d.N, device=d.dev), rowptr[1:] - rowptr[:-1], output_size=d.E)
    c = col.long()
    lower = c < rows
    entry = torch.cumsum(lower, 0) - 1
    keys, twin = (rows * d.N + c)[lower], (c * d.N + rows)[~lower]
    M = int(keys.numel())
    found = torch.searchsorted(keys, twin)
    if 2 * M != d.E or M >= 2 ** 30 or not bool((keys[found.clamp(max=M - 1)] == twin).all()):
        raise RuntimeError("edge orbit counts take a symmetric, loop-free CSR of fewer than 2^30 edges")
    entry[~lower] = found
    return entry.int(), M


def _edge_orbit_select(flat, induced):
    """``_orbit_select`` for edge orbits: every query is computed as its census class and its columns are mapped back
    through the position relabelling (query edge (a, b) -> the class representative's edge at the same place)."""
    wanted = []
    for k, e in flat:
        _, _, canon, p = _orbit_structure(k, e)
        ci = _census_class_of_mask(k)[canon]
        rep_edges = tuple(census_classes(k)[ci][1])
        rep_orbit_of = _edge_orbit_structure(k, rep_edges)[0]
        r = _orbit_structure(k, rep_edges)[3]
        r_inv = {x: i for i, x in enumerate(r)}
        for mem in _edge_orbit_structure(k, e)[1]:
            a, b = (r_inv[p[x]] for x in mem[0])
            wanted.append((k, ci, rep_orbit_of[(min(a, b), max(a, b))]))
    return _class_columns(wanted, induced, lambda k, e: len(_edge_orbit_structure(k, e)[1]))


_edge_orbit_transform = {}          # k -> int64 [columns of size k, columns of size k]: computed once per process


def edge_orbit_noninduced_matrix(k: int) -> np.ndarray:
    """T_k, int64 [C_k, C_k] over the edge-orbit columns of ``census_classes(k)``: T_k[(c,o')][(q,o)] = the copies of q
    in the class representative c in which one fixed edge of orbit o' has role o.  noninduced = induced @ T_k (a
    k-subset whose induced subgraph is c, seen from an edge of orbit o', holds that many copies of q with the edge in
    role o).  By exhaustive enumeration of the k! maps of every pair of classes."""
    if k not in _edge_orbit_transform:
        classes = [(tuple(e), _edge_orbit_structure(k, tuple(e))) for _, e in census_classes(k)]
        starts = np.concatenate([[0], np.cumsum([len(st[1]) for _, st in classes])])
        T = np.zeros((starts[-1], starts[-1]), dtype=np.int64)
        for qi, (qe, (q_orbit_of, q_members)) in enumerate(classes):
            aut = sum(1 for p in _perms(k) if _relabelled_mask(qe, p) == _relabelled_mask(qe, range(k)))
            for ci, (ce, (_, c_members)) in enumerate(classes):
                cmask = _relabelled_mask(ce, range(k))
                hits = np.zeros((k * (k - 1) // 2, len(q_members)), dtype=np.int64)     # [pair bit of c][role]
                for f in _perms(k):
                    if _relabelled_mask(qe, f) & ~cmask == 0:
                        for (a, b), o in q_orbit_of.items():
                            hits[_pair_bit(f[a], f[b]), o] += 1
                for o2, mem in enumerate(c_members):
                    bits = [_pair_bit(a, b) for a, b in mem]
                    assert (hits[bits] == hits[bits[0]]).all() and (hits[bits[0]] % aut == 0).all()
                    T[starts[ci] + o2, starts[qi]:starts[qi + 1]] = hits[bits[0]] // aut
        _edge_orbit_transform[k] = T
    return _edge_orbit_transform[k]


def _edge_orbit_table(reps):
    _, q_nodes, q_edge_ptr, q_edges = _flatten_queries(reps)
    table = np.empty((1098, 10), dtype=np.int16)
    ncol, kmax = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(_lib.lib().desco_edge_orbit_table(q_nodes.ctypes.data, q_edge_ptr.ctypes.data,
                                                 q_edges.ctypes.data if len(q_edges) else None, len(q_nodes),
                                                 table.ctypes.data, ctypes.byref(ncol), ctypes.byref(kmax)),
               "desco_edge_orbit_table")
    return table, int(ncol.value), int(kmax.value)


def _edge_orbit_device_raw(graphs: GraphSet, reps, dev) -> torch.Tensor:
    """desco_edge_orbit_counts_dev on pairwise non-isomorphic ``reps``: int64 [M, columns of reps] on ``dev``."""
    table, C, kmax = _edge_orbit_table(reps)
    if graphs.col.shape[0] == 0 or C == 0:           # no edges: no rows
        return torch.zeros((_num_edges(graphs), C), dtype=torch.int64, device=dev)
    d = _DeviceGraphs(graphs, dev)
    entry_row_d, M = _entry_rows_device(d)
    out = torch.empty((M, C), dtype=torch.int64, device=dev)
    table_d = d.put(table, np.int16)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().desco_edge_orbit_counts_dev(*d.head, entry_row_d.data_ptr(), M, table_d.data_ptr(), kmax,
                                                          C, out.data_ptr(),
                                                          torch.cuda.current_stream(dev).cuda_stream),
                   "desco_edge_orbit_counts_dev")
    return out


def _edge_orbit_host_raw(graphs: GraphSet, reps, num_threads: int) -> np.ndarray:
    """desco_edge_orbit_counts on pairwise non-isomorphic ``reps``: int64 [M, columns of reps]."""
    _, q_nodes, q_edge_ptr, q_edges = _flatten_queries(reps)
    out = np.zeros((_num_edges(graphs), _edge_orbit_table(reps)[1]), dtype=np.int64)
    _lib.check(_lib.lib().desco_edge_orbit_counts(graphs.graph_ptr.ctypes.data, graphs.num_graphs,
                                                  graphs.rowptr.ctypes.data, graphs.col.ctypes.data,
                                                  q_nodes.ctypes.data, q_edge_ptr.ctypes.data,
                                                  q_edges.ctypes.data if len(q_edges) else None, len(reps),
                                                  num_threads, out.ctypes.data), "desco_edge_orbit_counts")
    return out


def edge_orbit_counts_device(graphs: GraphSet, queries=None, device="cuda", induced: bool = True) -> torch.Tensor:
    """Exact per-edge orbit counts (definitions above) on the MI355X (csrc/groundtruth_dev.hip, ge_count_kernel): int64
    [M, len(edge_orbit_columns(queries))] on ``device``, rows as ``edge_orbit_rows``.  Duplicate and isomorphic queries
    are accepted: every class is enumerated once.  ``induced=False``: the edge-orbit census of the queries' sizes by the
    same kernel, then the exact int64 transform ``edge_orbit_noninduced_matrix`` with
    ``desco_canonical_noninduced_transform_dev`` (source columns in chunks of 32), without a round trip."""
    flat = _orbit_queries(queries, "edge orbit counts")
    dev = torch.device(device)
    if not flat:
        return torch.zeros((_num_edges(graphs), 0), dtype=torch.int64, device=dev)
    reps, index, sizes, first, width = _edge_orbit_select(flat, induced)
    raw = _edge_orbit_device_raw(graphs, reps, dev)
    if not induced and raw.shape[0]:
        full = torch.zeros_like(raw)
        for k in sizes:
            T = edge_orbit_noninduced_matrix(k)
            src, dst = raw[:, first[k]:first[k] + width[k]], full[:, first[k]:first[k] + width[k]]
            for c0 in range(0, width[k], 32):
                _transform_device(src[:, c0:c0 + 32], T[c0:c0 + 32], dst, c0 > 0)
        raw = full
    return raw.index_select(1, torch.from_numpy(index).to(dev))


def edge_orbit_counts(graphs: GraphSet, queries=None, num_threads: int = 0, backend: str = "auto",
                      induced: bool = True, per_query: bool = False) -> torch.Tensor:
    """Exact per-edge orbit counts -- the edge graphlet degree vector when ``queries`` is None (69 columns) -- as a
    double [M, len(edge_orbit_columns(queries))] tensor on the CPU, one row per undirected edge (``edge_orbit_rows``;
    definitions above).  ``backend``: "host" (OpenMP over graphs, ``num_threads`` threads), "device"
    (``edge_orbit_counts_device``) or "auto": the device when a GPU is present and the adjacency bitsets fit
    ``_DEVICE_BITSET_LIMIT_WORDS``.  ``induced=False``: the non-induced form.  ``per_query=True``: the orbits of every
    query summed, [M, num_queries]: the copies of the query through the edge, the motif weight of that adjacent pair.
    Raises RuntimeError for queries outside 2..5 nodes and for disconnected or looped ones."""
    if backend not in ("auto", "host", "device"):
        raise ValueError(f"unknown backend {backend!r}")
    flat = _orbit_queries(queries, "edge orbit counts")
    if backend == "auto":       # _device_eligible's conditions: a GPU and bitsets within the limit (the sizes are checked)
        backend = "device" if flat and _device_eligible(graphs, np.array([2], dtype=np.int32)) else "host"
    if backend == "device":
        out = edge_orbit_counts_device(graphs, flat, induced=induced).cpu()
    elif not flat:
        out = torch.zeros((_num_edges(graphs), 0), dtype=torch.int64)
    else:
        reps, index, sizes, first, width = _edge_orbit_select(flat, induced)
        raw = _edge_orbit_host_raw(graphs, reps, num_threads)
        if not induced:
            raw = np.concatenate([raw[:, first[k]:first[k] + width[k]] @ edge_orbit_noninduced_matrix(k)
                                  for k in sizes], axis=1)
        out = torch.from_numpy(np.ascontiguousarray(raw[:, index]))
    if per_query:
        owner = torch.tensor([qi for qi, _, _ in edge_orbit_columns(flat)], dtype=torch.long)
        summed = torch.zeros((out.shape[0], len(flat)), dtype=torch.int64)
        out = summed.index_add_(1, owner, out)
    return out.double()


# ---- large queries: the pattern-guided matcher ------------------------------------------------------------------------
# One device launch covers the CSR entries of a slice; a slice holds so many entries that entries x anchors (= waves)
# stays at this bound, so that no single kernel carries the whole of an unbounded search
_MATCH_SLICE_WAVES = 1 << 18
# name of the backend that served the last canonical_counts_match call ("host" or "device")
last_match_backend = None


def match_plan(queries: Sequence) -> np.ndarray:
    """The matcher's plan of ``queries`` (desco_canonical_match_plan, include/desco_hip.h): int32, plan[0] = number of
    queries, plan[1] = number of anchors, then one record of 84 entries per anchor.  Raises RuntimeError naming the
    limit for queries outside 2..16 nodes, disconnected queries and loops."""
    _, q_nodes, q_edge_ptr, q_edges = _flatten_queries(queries)
    L = _lib.lib()
    qargs = (q_nodes.ctypes.data, q_edge_ptr.ctypes.data, q_edges.ctypes.data if len(q_edges) else None, len(q_nodes))
    entries = int(L.desco_canonical_match_plan_size(*qargs))
    if entries < 0:
        _lib.check(-1, "desco_canonical_match_plan_size")
    plan = np.zeros(entries, dtype=np.int32)
    _lib.check(L.desco_canonical_match_plan(*qargs, plan.ctypes.data, entries), "desco_canonical_match_plan")
    return plan


def _sliced(E: int, slice_entries: int, stream, launch):
    """``launch(e0, e1)`` for consecutive slices of the CSR entries [0, E) (once, empty, when E is 0)."""
    e0 = 0
    while True:
        e1 = min(e0 + slice_entries, E)
        launch(e0, e1)
        stream.synchronize()                # a fault of this slice surfaces here, before the next is enqueued
        e0 = e1
        if e0 >= E:
            break


def canonical_counts_match_device(graphs: GraphSet, queries: Sequence, device="cuda",
                                  slice_entries=None, induced: bool = True) -> torch.Tensor:
    """The counts of ``canonical_counts_match`` computed on the MI355X (csrc/groundtruth_match_dev.hip).  Returns a
    [num_nodes, num_queries] int64 tensor on ``device``.  The CSR entries are cut into slices of ``slice_entries``
    (default: ``_MATCH_SLICE_WAVES`` waves per launch), one launch each, and the stream is synchronised and the
    status checked after every slice; the slicing does not change the result.  ``induced=False``: the non-induced counts
    of ``canonical_counts`` by the kernel's non-induced instantiation (same plan, same slices)."""
    plan = match_plan(queries)
    Q, A = int(plan[0]), int(plan[1])
    dev = torch.device(device)
    out = torch.zeros((graphs.num_nodes, Q), dtype=torch.int64, device=dev)
    if graphs.num_nodes == 0 or Q == 0:
        return out
    if slice_entries is None:
        slice_entries = max(_MATCH_SLICE_WAVES // max(A, 1), 1)
    slice_entries = int(slice_entries)
    if slice_entries < 1:
        raise ValueError("slice_entries must be positive")
    d = _DeviceGraphs(graphs, dev)
    plan_d = d.put(plan, np.int32)
    L = _lib.lib()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        head = (*d.head, plan.ctypes.data, plan_d.data_ptr(), len(plan), Q)

        def launch(e0, e1):
            if induced:
                _lib.check(L.desco_canonical_counts_match_dev(*head, e0, e1, out.data_ptr(), stream.cuda_stream),
                           "desco_canonical_counts_match_dev")
            else:
                _lib.check(L.desco_canonical_counts_match_mode_dev(*head, 0, e0, e1, out.data_ptr(),
                                                                   stream.cuda_stream),
                           "desco_canonical_counts_match_mode_dev")
        _sliced(d.E, slice_entries, stream, launch)
    return out


def _match_host_int64(graphs: GraphSet, queries: Sequence, induced: bool, num_threads: int) -> np.ndarray:
    """The host matcher: int64 [num_nodes, num_queries]."""
    plan = match_plan(queries)
    out = np.zeros((graphs.num_nodes, int(plan[0])), dtype=np.int64)
    head = (graphs.graph_ptr.ctypes.data, graphs.num_graphs, graphs.rowptr.ctypes.data, graphs.col.ctypes.data,
            plan.ctypes.data, len(plan), int(plan[0]))
    L = _lib.lib()
    if induced:
        _lib.check(L.desco_canonical_counts_match(*head, num_threads, out.ctypes.data), "desco_canonical_counts_match")
    else:
        _lib.check(L.desco_canonical_counts_match_mode(*head, 0, num_threads, out.ctypes.data),
                   "desco_canonical_counts_match_mode")
    return out


def canonical_counts_match(graphs: GraphSet, queries: Sequence, backend: str = "auto",
                           num_threads: int = 0, slice_entries=None, induced: bool = True) -> torch.Tensor:
    """Canonical counts by the pattern-guided induced-subgraph matcher: [num_nodes, num_queries] double tensor on the
    CPU, count[v][q] = #{S : max(S) = v, G[S] isomorphic to q} as ``canonical_counts``.  Its work follows the query
    instead of the number of connected k-subsets, so it takes queries of 2..16 nodes (small ones too, to be checked
    against ESU), any number of them, isomorphic duplicates included.
    ``backend``: "host" (OpenMP over graphs, ``num_threads`` threads), "device" (HIP kernel, ``slice_entries`` as in
    ``canonical_counts_match_device``) or "auto": the device when a GPU is present and the adjacency bitsets fit
    ``_DEVICE_BITSET_LIMIT_WORDS``, else the host.  ``last_match_backend`` names the one that served the call.
    ``induced=False``: the non-induced counts of ``canonical_counts`` -- the same plan, a candidate only has to be
    adjacent to the images the record's mask names."""
    global last_match_backend
    if backend not in ("host", "device", "auto"):
        raise ValueError(f"unknown backend {backend!r}")
    if backend == "auto":
        fits = int(_bitset_words(graphs).sum()) <= _DEVICE_BITSET_LIMIT_WORDS
        backend = "device" if torch.cuda.is_available() and fits else "host"
    last_match_backend = backend
    if backend == "device":
        return canonical_counts_match_device(graphs, queries, slice_entries=slice_entries,
                                             induced=induced).cpu().double()
    return torch.from_numpy(_match_host_int64(graphs, queries, induced, num_threads)).double()


def _canonical_counts_vf2(graphs: GraphSet, queries: Sequence, induced: bool = True) -> torch.Tensor:
    """The reference's own procedure for unlabelled queries: networkx VF2, one match per isomorphism keyed by
    ``max(vmap.keys())`` (workload.py:327-348), divided by the query's automorphism count (data.py:61-67).  Any query
    size; minutes where the native paths take milliseconds.  ``induced=False``: one match per MONOMORPHISM
    (``subgraph_monomorphisms_iter``), keyed and divided the same way."""
    import networkx as nx
    flat, _, _, _ = _flatten_queries(queries)
    GM = nx.algorithms.isomorphism.GraphMatcher
    targets = []
    for n, edges in graphs.edge_lists():
        t = nx.Graph()
        t.add_nodes_from(range(n))
        t.add_edges_from(edges)
        targets.append(t)
    out = torch.zeros((graphs.num_nodes, len(flat)), dtype=torch.double)
    for qi, (k, edges) in enumerate(flat):
        q = nx.Graph()
        q.add_nodes_from(range(k))
        q.add_edges_from(edges)
        sym = sum(1 for _ in GM(q, q).subgraph_isomorphisms_iter())
        for g, t in enumerate(targets):
            base = int(graphs.graph_ptr[g])
            gm = GM(t, q)
            for vmap in (gm.subgraph_isomorphisms_iter() if induced else gm.subgraph_monomorphisms_iter()):
                out[base + max(vmap.keys()), qi] += 1
        out[:, qi] /= sym
    return out


# ---- labelled queries (--use_node_feature) ---------------------------------------------------------------------------
# Limits of the native paths (include/desco_hip.h).  Host: label ids of 8 bits, queries of 2..6 nodes.  Device:
# label ids of 4 bits, queries of 2..5 nodes, and a direct lookup table of sum_k 2^(k(k-1)/2) A^k int32 entries that
# must fit the budget below: 256 MiB, the size of the MI355X's Infinity Cache, so that the few entries a graph set
# touches are served on chip (A = 8 with 5-node queries is 134 MB, A = 9 242 MB; A = 10 goes to the host path, as
# does anything wider than 16 labels).
_HOST_LABEL_LIMIT = 256
_DEVICE_LABEL_LIMIT = 16
_DEVICE_LABEL_TABLE_LIMIT_BYTES = 256 << 20
# the device path counts per labelled CLASS into [nodes, C] int64 and expands to [nodes, Q] (int64, and its double
# copy on the way to the host): they live on the device for one chunk of whole graphs at a time, chosen so that
# 8 (C + 2 Q) bytes per node stay below this budget (a single graph above it is a chunk of its own)
_DEVICE_LABEL_CHUNK_BYTES = 1 << 30
# name of the backend that served the last canonical_counts_labelled call ("vf2", "host" or "device")
last_labelled_backend = None


class _Labelled:
    """Label ids, flattened queries and labelled isomorphism classes of one call."""

    def __init__(self, graphs, queries: Sequence, key: str):
        """``graphs``: a GraphSet with node_feat, or None (query labels only: ``match_plan_labelled``)."""
        if graphs is not None and graphs.node_feat is None:
            raise ValueError("labelled ground truth needs GraphSet.node_feat")
        self.nan = False
        ids = {}                      # feature row as a tuple of floats -> id: float equality, as the VF2 node_match
        # (-0.0 == 0.0 and hash alike; NaN never equals anything -> VF2 path)
        nf = (graphs.node_feat.astype(np.float64) if graphs is not None else np.zeros((0, 1))) + 0.0
        self.nan |= bool(np.isnan(nf).any())
        if nf.shape[0]:
            uniq, inv = np.unique(nf, axis=0, return_inverse=True)
            remap = np.array([ids.setdefault(tuple(r.tolist()), len(ids)) for r in uniq], dtype=np.int32)
            self.node_labels = np.ascontiguousarray(remap[np.asarray(inv).reshape(-1)], dtype=np.int32)
        else:
            self.node_labels = np.zeros(0, dtype=np.int32)
        flat, q_labels = [], []
        for q in queries:
            nodes = list(q.nodes)
            idx = {v: i for i, v in enumerate(nodes)}
            flat.append((len(nodes), [(idx[a], idx[b]) for a, b in q.edges()]))
            for v in nodes:
                f = tuple(float(x) for x in np.asarray(q.nodes[v][key]).reshape(-1))
                self.nan |= any(x != x for x in f)
                q_labels.append(ids.setdefault(f, len(ids)))
        self.num_labels = max(len(ids), 1)
        self.flat, self.q_nodes, self.q_edge_ptr, self.q_edges = _flatten_queries(flat)
        self.q_labels = np.array(q_labels, dtype=np.int32)
        self.num_queries = len(flat)
        self.kmin = int(self.q_nodes.min()) if len(flat) else 2
        self.kmax = int(self.q_nodes.max()) if len(flat) else 2
        self.class_of_query, self.num_classes = None, 0

    def host_limit(self):
        """None when the native host path takes this input, else the limit it is outside of."""
        if self.nan:
            return "features contain NaN (never equal to anything): only the VF2 path reproduces that"
        if self.num_labels > _HOST_LABEL_LIMIT:
            return f"{self.num_labels} distinct labels: the native paths take at most {_HOST_LABEL_LIMIT}"
        if self.kmin < 2 or self.kmax > 6:
            return "the native host path takes queries of 2..6 nodes"
        return None

    def table_bytes(self):
        return 4 * sum((1 << (k * (k - 1) // 2)) * self.num_labels ** k for k in range(2, self.kmax + 1))

    def device_limit(self, graphs: GraphSet):
        """None when the device path takes this input, else the limit it is outside of."""
        if self.host_limit():
            return self.host_limit()
        if self.kmax > 5:
            return "the device path takes labelled queries of 2..5 nodes"
        if self.num_labels > _DEVICE_LABEL_LIMIT:
            return f"{self.num_labels} distinct labels: the device path takes at most {_DEVICE_LABEL_LIMIT}"
        if self.table_bytes() > _DEVICE_LABEL_TABLE_LIMIT_BYTES:
            return (f"the lookup table for {self.num_labels} labels and {self.kmax}-node queries takes "
                    f"{self.table_bytes()} bytes, above the budget of {_DEVICE_LABEL_TABLE_LIMIT_BYTES}")
        if int(_bitset_words(graphs).sum()) > _DEVICE_BITSET_LIMIT_WORDS:
            return "the adjacency bitsets are above the device path's limit"
        return None

    def _qargs(self):
        return (self.q_nodes.ctypes.data, self.q_edge_ptr.ctypes.data,
                self.q_edges.ctypes.data if len(self.q_edges) else None, self.q_labels.ctypes.data,
                self.num_queries, self.num_labels)

    def classes(self):
        if self.class_of_query is None:
            coq = np.zeros(self.num_queries, dtype=np.int32)
            c, kmax = ctypes.c_int(0), ctypes.c_int(0)
            _lib.check(_lib.lib().desco_canonical_label_classes(*self._qargs(), coq.ctypes.data, ctypes.byref(c),
                                                                ctypes.byref(kmax)), "desco_canonical_label_classes")
            self.class_of_query, self.num_classes = coq, int(c.value)
        return self.class_of_query

    def table(self):
        coq = self.classes()
        L = _lib.lib()
        entries = int(L.desco_canonical_label_table_size(self.kmax, self.num_labels))
        if entries < 0:
            _lib.check(-1, "desco_canonical_label_table_size")
        table = np.empty(entries, dtype=np.int32)
        _lib.check(L.desco_canonical_label_table(*self._qargs(), coq.ctypes.data, self.num_classes, self.kmax,
                                                 table.ctypes.data, entries), "desco_canonical_label_table")
        return table


def _labelled_host(graphs: GraphSet, lab: _Labelled, num_threads: int) -> torch.Tensor:
    coq = lab.classes()
    out = np.zeros((graphs.num_nodes, lab.num_classes), dtype=np.int64)
    _lib.check(_lib.lib().desco_canonical_counts_labelled(
        graphs.graph_ptr.ctypes.data, graphs.num_graphs, graphs.rowptr.ctypes.data, graphs.col.ctypes.data,
        lab.node_labels.ctypes.data, lab.num_labels, *lab._qargs()[:5], coq.ctypes.data, lab.num_classes,
        num_threads, out.ctypes.data), "desco_canonical_counts_labelled")
    return torch.from_numpy(out)[:, torch.from_numpy(coq).long()].double()


def _labelled_device_chunks(graphs: GraphSet, lab: _Labelled, dev, chunk_bytes=None):
    """Yields (first node, end node, [nodes, Q] int64 counts on ``dev``) for consecutive chunks of whole graphs."""
    L = _lib.lib()
    table = _put(lab.table(), np.int32, dev)
    coq = _put(lab.classes(), np.int64, dev)
    C, Q, G = lab.num_classes, lab.num_queries, graphs.num_graphs
    budget = _DEVICE_LABEL_CHUNK_BYTES if chunk_bytes is None else int(chunk_bytes)
    max_nodes = max(budget // (8 * (C + 2 * Q)), 1)
    g0 = 0
    while g0 < G:
        g1 = g0 + 1
        while g1 < G and graphs.graph_ptr[g1 + 1] - graphs.graph_ptr[g0] <= max_nodes:
            g1 += 1
        sub = graphs if (g0, g1) == (0, G) else graphs.subset(g0, g1)
        n0, n1 = int(graphs.graph_ptr[g0]), int(graphs.graph_ptr[g1])
        g0 = g1
        if n1 == n0:
            continue
        d = _DeviceGraphs(sub, dev)
        labels = d.put(lab.node_labels[n0:n1], np.int32)
        out = torch.empty((n1 - n0, C), dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            _lib.check(L.desco_canonical_counts_labelled_dev(
                *d.head, labels.data_ptr(), lab.num_labels, table.data_ptr(), table.numel(), lab.kmax, C,
                out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "desco_canonical_counts_labelled_dev")
        yield n0, n1, out.index_select(1, coq)


def _require_device(lab: _Labelled, graphs: GraphSet):
    limit = lab.device_limit(graphs)
    if limit:
        raise RuntimeError("canonical_counts_labelled: device path: " + limit)


def canonical_counts_labelled_device(graphs: GraphSet, queries: Sequence, node_feat_key: str = "feat",
                                     device="cuda", chunk_bytes=None) -> torch.Tensor:
    """The counts of ``canonical_counts_labelled`` computed on the MI355X (csrc/groundtruth_label_dev.hip): labelled
    queries of 2..5 nodes, any number of them, duplicates (isomorphic labelled copies) included, at most 16 distinct
    labels and a lookup table within ``_DEVICE_LABEL_TABLE_LIMIT_BYTES``; raises RuntimeError naming the limit
    otherwise.  Returns a [num_nodes, num_queries] int64 tensor on ``device``.  The per-class intermediate is
    produced in node chunks of at most ``chunk_bytes`` (default ``_DEVICE_LABEL_CHUNK_BYTES``); the chunking does
    not change the result."""
    lab = _Labelled(graphs, queries, node_feat_key)
    _require_device(lab, graphs)
    dev = torch.device(device)
    out = torch.zeros((graphs.num_nodes, lab.num_queries), dtype=torch.int64, device=dev)
    if graphs.num_nodes and lab.num_queries:
        for n0, n1, counts in _labelled_device_chunks(graphs, lab, dev, chunk_bytes):
            out[n0:n1] = counts
    return out


def canonical_counts_labelled(graphs: GraphSet, queries: Sequence, node_feat_key: str = "feat",
                              backend: str = "auto", num_threads: int = 0, induced: bool = True) -> torch.Tensor:
    """Canonical counts of LABELLED queries (--use_node_feature): [num_nodes, num_queries] double tensor on the CPU,
    count[v][q] = #{S : max(S) = v, G[S] connected, G[S] with its node labels isomorphic to labelled query q} --
    the reference's VF2 with ``node_match`` on the feature (workload.py:327-348) divided by the labelled symmetry
    factor (data.py:61-68).  ``queries``: networkx graphs whose nodes carry ``node_feat_key``; two nodes match iff
    their feature vectors are equal as lists of floats.  Isomorphic labelled copies (the reference's expansion is
    full of them) get equal columns.

    ``backend``: "vf2" (the reference's procedure in Python, the yardstick of the tests), "host" (OpenMP enumerator,
    queries of 2..6 nodes, ``num_threads`` threads), "device" (HIP kernel; raises RuntimeError naming the limit the
    input is outside of, see ``canonical_counts_labelled_device``) or "auto": the device when a GPU is present and
    the input fits it, else the host enumerator, else (features with NaN, more than 256 distinct labels) VF2.
    ``last_labelled_backend`` names the one that served the call.
    Columns of queries with 7..16 nodes go to the labelled matcher (``canonical_counts_match_labelled``) with the same
    ``backend`` and the results are joined in query order; a call made only of such queries sets
    ``last_labelled_backend`` to the matcher's backend.  Above 16 nodes "auto" uses VF2 and "host" / "device" raise.
    ``induced=False``: NON-INDUCED labelled counts (label-preserving monomorphisms with the largest image v, divided by
    the label-preserving automorphisms).  There is no labelled census: every size 2..16 goes to the labelled matcher."""
    global last_labelled_backend
    if backend not in ("vf2", "host", "device", "auto"):
        raise ValueError(f"unknown backend {backend!r}")
    if backend == "vf2":
        last_labelled_backend = "vf2"
        return _canonical_counts_labelled_vf2(graphs, queries, node_feat_key, induced)
    lab = _Labelled(graphs, queries, node_feat_key)
    if not induced:
        if lab.nan or lab.kmax > 16:
            if backend == "auto":
                last_labelled_backend = "vf2"
                return _canonical_counts_labelled_vf2(graphs, queries, node_feat_key, False)
            if lab.nan:
                raise RuntimeError(f"canonical_counts_labelled: {backend} path: " + lab.host_limit())
            raise RuntimeError(f"canonical_counts_labelled: {backend} path: the native paths take labelled queries "
                               "of 2..16 nodes (backend=\"vf2\" takes larger ones)")
        out = canonical_counts_match_labelled(graphs, queries, node_feat_key, backend, num_threads, induced=False)
        last_labelled_backend = last_labelled_match_backend
        return out
    large = [i for i, k in enumerate(lab.q_nodes) if k > 6]
    if large and not (backend == "auto" and (lab.nan or lab.kmax > 16)):
        # columns above 6 nodes go to the labelled matcher with the same backend, the others where they always went
        if lab.nan:
            raise RuntimeError(f"canonical_counts_labelled: {backend} path: " + lab.host_limit())
        if lab.kmax > 16:
            raise RuntimeError(f"canonical_counts_labelled: {backend} path: the native paths take labelled queries "
                               "of 2..16 nodes (backend=\"vf2\" takes larger ones)")
        queries = list(queries)
        small = [i for i, k in enumerate(lab.q_nodes) if k <= 6]
        out = torch.zeros((graphs.num_nodes, lab.num_queries), dtype=torch.double)
        if small:
            out[:, small] = canonical_counts_labelled(graphs, [queries[i] for i in small], node_feat_key, backend,
                                                      num_threads)
        out[:, large] = canonical_counts_match_labelled(graphs, [queries[i] for i in large], node_feat_key, backend,
                                                        num_threads)
        if not small:
            last_labelled_backend = last_labelled_match_backend
        return out
    if large:
        backend = "vf2"                         # "auto" with NaN features or a query above 16 nodes
    if backend == "device":
        _require_device(lab, graphs)
    elif backend == "auto":
        if lab.host_limit():
            backend = "vf2"
        else:
            backend = "device" if torch.cuda.is_available() and not lab.device_limit(graphs) else "host"
    if backend == "vf2":
        last_labelled_backend = "vf2"
        return _canonical_counts_labelled_vf2(graphs, queries, node_feat_key)
    if backend == "host" and lab.host_limit():
        raise RuntimeError("canonical_counts_labelled: host path: " + lab.host_limit())
    out = torch.zeros((graphs.num_nodes, lab.num_queries), dtype=torch.double)
    if graphs.num_nodes and lab.num_queries:
        if backend == "host":
            out = _labelled_host(graphs, lab, num_threads)
        else:
            for n0, n1, counts in _labelled_device_chunks(graphs, lab, torch.device("cuda")):
                out[n0:n1] = counts.double().cpu()
    last_labelled_backend = backend
    return out


# ---- labelled queries of 7..16 nodes: the matcher with labels ---------------------------------------------------------
# name of the backend that served the last canonical_counts_match_labelled call ("host" or "device")
last_labelled_match_backend = None
# offsets into the labelled plan (csrc/groundtruth_match.hpp)
_GTML_HEAD, _GTML_REC, _GTML_LABEL, _GTML_BUCKET = 4, 100, 84, 4


def _match_plan_labelled(lab: _Labelled):
    L = _lib.lib()
    qargs = lab._qargs()[:5]
    entries = int(L.desco_canonical_match_plan_labelled_size(*qargs))
    if entries < 0:
        _lib.check(-1, "desco_canonical_match_plan_labelled_size")
    plan = np.zeros(entries, dtype=np.int32)
    coq = np.zeros(lab.num_queries, dtype=np.int32)
    c = ctypes.c_int(0)
    _lib.check(L.desco_canonical_match_plan_labelled(*qargs, plan.ctypes.data, entries, coq.ctypes.data,
                                                     ctypes.byref(c)), "desco_canonical_match_plan_labelled")
    return plan, coq


def match_plan_labelled(queries: Sequence, node_feat_key: str = "feat"):
    """The labelled matcher's plan of ``queries`` (networkx graphs whose nodes carry ``node_feat_key``) and
    class_of_query (desco_canonical_match_plan_labelled, include/desco_hip.h): ``(plan, class_of_query)``, int32.
    plan[0] = number of labelled isomorphism classes, plan[1] = number of records, plan[2] = number of buckets,
    plan[3] = the largest bucket, then records of 100 entries (the 84 of ``match_plan`` with the class as query, then
    the label id of every position) sorted by the labels of positions 0 and 1, then buckets of 4 entries.  Label ids
    number the distinct feature vectors of the queries in order of appearance.  Raises RuntimeError naming the limit
    for queries outside 2..16 nodes, disconnected queries and loops."""
    lab = _Labelled(None, queries, node_feat_key)
    if lab.nan:
        raise RuntimeError("match_plan_labelled: features contain NaN (never equal to anything)")
    return _match_plan_labelled(lab)


def _plan_buckets(plan: np.ndarray) -> np.ndarray:
    """[B, 4] view of the plan's buckets: label 0, label 1, first record, end record."""
    return plan[_GTML_HEAD + int(plan[1]) * _GTML_REC:].reshape(-1, _GTML_BUCKET)


def labelled_match_waves(graphs: GraphSet, lab_or_labels, plan: np.ndarray):
    """(launched, live) waves of the device labelled matcher for this input: it launches the largest bucket per CSR
    entry; live are the (entry (v, u0) with u0 < v, record of the bucket of their labels) pairs."""
    labels = lab_or_labels.node_labels if isinstance(lab_or_labels, _Labelled) else np.asarray(lab_or_labels)
    E = int(graphs.col.shape[0])
    launched = E * int(plan[3])
    rows = np.repeat(np.arange(graphs.num_nodes, dtype=np.int64), np.diff(graphs.rowptr))
    below = graphs.col < rows
    size = {(int(b[0]), int(b[1])): int(b[3] - b[2]) for b in _plan_buckets(plan)}
    pairs, counts = np.unique(np.stack([labels[rows[below]], labels[graphs.col[below]]], axis=1), axis=0,
                              return_counts=True) if below.any() else (np.zeros((0, 2), np.int64), np.zeros(0, np.int64))
    live = sum(int(n) * size.get((int(a), int(b)), 0) for (a, b), n in zip(pairs, counts))
    return launched, live


def _labelled_match_device(graphs: GraphSet, lab: _Labelled, dev, slice_entries=None, induced: bool = True):
    """([num_nodes, num_classes] int64 counts on ``dev``, class_of_query)"""
    plan, coq = _match_plan_labelled(lab)
    C, largest = int(plan[0]), int(plan[3])
    N = graphs.num_nodes
    if N == 0 or lab.num_queries == 0:
        return torch.zeros((N, C), dtype=torch.int64, device=dev), coq
    if slice_entries is None:           # waves per launch = entries x largest bucket, whatever the number of records
        slice_entries = max(_MATCH_SLICE_WAVES // max(largest, 1), 1)
    slice_entries = int(slice_entries)
    if slice_entries < 1:
        raise ValueError("slice_entries must be positive")
    d = _DeviceGraphs(graphs, dev)
    plan_d, labels = d.put(plan, np.int32), d.put(lab.node_labels, np.int32)
    out = torch.zeros((N, C), dtype=torch.int64, device=dev)
    L = _lib.lib()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        head = (*d.head, labels.data_ptr(), plan.ctypes.data, plan_d.data_ptr(), len(plan), C)

        def launch(e0, e1):
            if induced:
                _lib.check(L.desco_canonical_counts_match_labelled_dev(*head, e0, e1, out.data_ptr(),
                                                                       stream.cuda_stream),
                           "desco_canonical_counts_match_labelled_dev")
            else:
                _lib.check(L.desco_canonical_counts_match_labelled_mode_dev(*head, 0, e0, e1, out.data_ptr(),
                                                                            stream.cuda_stream),
                           "desco_canonical_counts_match_labelled_mode_dev")
        _sliced(d.E, slice_entries, stream, launch)
    return out, coq


def _require_no_nan(lab: _Labelled, who: str):
    if lab.nan:
        raise RuntimeError(f"{who}: features contain NaN (never equal to anything): only the VF2 path reproduces that")


def canonical_counts_match_labelled_device(graphs: GraphSet, queries: Sequence, node_feat_key: str = "feat",
                                           device="cuda", slice_entries=None, induced: bool = True) -> torch.Tensor:
    """The counts of ``canonical_counts_match_labelled`` computed on the MI355X (csrc/groundtruth_match_dev.hip, the
    labelled instantiation).  Returns a [num_nodes, num_queries] int64 tensor on ``device``.  Each labelled class is
    matched once and its column copied to every query of the class.  The CSR entries are cut into slices of
    ``slice_entries`` (default: ``_MATCH_SLICE_WAVES`` waves per launch, a wave being one (entry, record slot of the
    largest label bucket) pair), one launch each, synchronised and checked; the slicing does not change the result.
    ``induced=False``: the non-induced labelled counts (the kernel's fourth instantiation; same plan, same slices)."""
    lab = _Labelled(graphs, queries, node_feat_key)
    _require_no_nan(lab, "canonical_counts_match_labelled_device")
    dev = torch.device(device)
    out, coq = _labelled_match_device(graphs, lab, dev, slice_entries, induced)
    return out.index_select(1, torch.from_numpy(coq).long().to(dev))


def canonical_counts_match_labelled(graphs: GraphSet, queries: Sequence, node_feat_key: str = "feat",
                                    backend: str = "auto", num_threads: int = 0, slice_entries=None,
                                    induced: bool = True) -> torch.Tensor:
    """Labelled canonical counts (as ``canonical_counts_labelled``) by the pattern-guided matcher: [num_nodes,
    num_queries] double tensor on the CPU.  Labelled queries of 2..16 nodes (small ones too, to be checked against the
    labelled ESU path), any number of them, any number of distinct labels; isomorphic labelled copies are matched once.
    ``backend``: "host" (OpenMP over graphs, ``num_threads`` threads), "device" (HIP kernel) or "auto": the device when
    a GPU is present and the adjacency bitsets fit ``_DEVICE_BITSET_LIMIT_WORDS``, else the host.
    ``last_labelled_match_backend`` names the one that served the call.  Features with NaN are refused (VF2 only).
    ``induced=False``: label-preserving monomorphisms instead of induced embeddings, as ``canonical_counts_labelled``."""
    global last_labelled_match_backend
    if backend not in ("host", "device", "auto"):
        raise ValueError(f"unknown backend {backend!r}")
    lab = _Labelled(graphs, queries, node_feat_key)
    _require_no_nan(lab, "canonical_counts_match_labelled")
    if backend == "auto":
        fits = int(_bitset_words(graphs).sum()) <= _DEVICE_BITSET_LIMIT_WORDS
        backend = "device" if torch.cuda.is_available() and fits else "host"
    last_labelled_match_backend = backend
    if backend == "device":
        # expanded to query columns and converted on the device, in row chunks within the labelled paths' byte budget
        # (int64 + double copy of a chunk), each copied straight into its rows of the result
        dev = torch.device("cuda")
        out, coq = _labelled_match_device(graphs, lab, dev, slice_entries, induced)
        coq_d = torch.from_numpy(coq).long().to(dev)
        res = torch.empty((graphs.num_nodes, lab.num_queries), dtype=torch.double)
        rows = max(_DEVICE_LABEL_CHUNK_BYTES // (16 * max(lab.num_queries, 1)), 1)
        for n0 in range(0, graphs.num_nodes, rows):
            res[n0:n0 + rows].copy_(out[n0:n0 + rows].index_select(1, coq_d).double())
        return res
    plan, coq = _match_plan_labelled(lab)
    out = np.zeros((graphs.num_nodes, int(plan[0])), dtype=np.int64)
    head = (graphs.graph_ptr.ctypes.data, graphs.num_graphs, graphs.rowptr.ctypes.data, graphs.col.ctypes.data,
            lab.node_labels.ctypes.data, plan.ctypes.data, len(plan), int(plan[0]))
    if induced:
        _lib.check(_lib.lib().desco_canonical_counts_match_labelled(*head, num_threads, out.ctypes.data),
                   "desco_canonical_counts_match_labelled")
    else:
        _lib.check(_lib.lib().desco_canonical_counts_match_labelled_mode(*head, 0, num_threads, out.ctypes.data),
                   "desco_canonical_counts_match_labelled_mode")
    return torch.from_numpy(out)[:, torch.from_numpy(coq).long()].double()


def _canonical_counts_labelled_vf2(graphs: GraphSet, queries: Sequence, node_feat_key: str = "feat",
                                   induced: bool = True) -> torch.Tensor:
    """The reference's own procedure: networkx VF2 with ``node_match`` on the feature (workload.py:327-348)
    divided by the labelled symmetry factor (data.py:61-68).  One matcher per (query, graph) in Python: the
    reference every native path is tested against, and the path for features that contain NaN."""
    import networkx as nx
    if graphs.node_feat is None:
        raise ValueError("labelled ground truth needs GraphSet.node_feat")
    match = lambda a, b: a[node_feat_key] == b[node_feat_key]     # noqa: E731
    targets = []
    for g, (n, edges) in enumerate(graphs.edge_lists()):
        t = nx.Graph()
        base = int(graphs.graph_ptr[g])
        for v in range(n):
            t.add_node(v, **{node_feat_key: [float(x) for x in graphs.node_feat[base + v]]})
        t.add_edges_from(edges)
        targets.append(t)
    out = torch.zeros((graphs.num_nodes, len(queries)), dtype=torch.double)
    for qi, q in enumerate(queries):
        qq = nx.Graph()
        for v in q.nodes:
            qq.add_node(v, **{node_feat_key: [float(x) for x in np.asarray(q.nodes[v][node_feat_key]).reshape(-1)]})
        qq.add_edges_from(q.edges())
        sym = sum(1 for _ in nx.algorithms.isomorphism.GraphMatcher(qq, qq, node_match=match)
                  .subgraph_isomorphisms_iter())
        for g, t in enumerate(targets):
            base = int(graphs.graph_ptr[g])
            gm = nx.algorithms.isomorphism.GraphMatcher(t, qq, node_match=match)
            for vmap in (gm.subgraph_isomorphisms_iter() if induced else gm.subgraph_monomorphisms_iter()):
                out[base + max(vmap.keys()), qi] += 1
        out[:, qi] /= sym
    return out


# ---- occurrence listing (desco_amd/occurrences.py, which is built on this module: re-exported on first use) ----------
_OCCURRENCE_NAMES = ("Occurrences", "list_occurrences", "list_occurrences_device", "iter_occurrences")


def __getattr__(name):
    if name in _OCCURRENCE_NAMES:
        from . import occurrences
        return getattr(occurrences, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
