"""Comparing networks by their graphlet degree vectors: graphlet correlation matrices and the graphlet correlation
distance (GCD; Yaveroglu et al., "Revealing the hidden language of complex networks", 2014).

Per segment of an orbit table (``groundtruth.orbit_counts``; by default one segment per graph) the graphlet correlation
matrix is Spearman's rho between the orbit columns over the segment's nodes, and the distance between two segments is
the Euclidean distance of the upper triangles of their matrices.  The arithmetic is defined in include/desco_hip.h,
"GRAPHLET CORRELATION", so that the host twin (csrc/graphlet_correlation.cpp, OpenMP) and the gfx950 kernels
(csrc/graphlet_correlation_dev.hip) return the same bits: integer ranks, an int64 matrix S, one rounded operation per
step of rho, and one fma chain in a fixed order per distance.

``dummy_row`` (default on) gives every segment one extra row of ones, so that a column of zeros is not constant.  That
is the convention of the published GCD scripts as far as this project knows it; it is stated, not pinned against them.

Column sets are selected by structure, in this project's own orbit numbering (``groundtruth.orbit_columns``):
"all5" the 73 orbits of the graphs of 2..5 nodes, "all4" the 15 of 2..4 nodes, "gcd11" those 15 without the triangle's
orbit, the diamond's two (the 4-node graph with 5 edges) and K4's -- the non-redundant eleven of the paper -- or an
explicit list of column indices.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from . import groundtruth as gt
from .graphs import GraphSet

# who served the last graphlet_correlation / gcd / nearest / dataset_gcd call (or graphlet_distribution / gdd_agreement /
# gdd_nearest / dataset_gdda): "host", "device", or "device+host" when segments above the device's row bound were computed
# by the host twin and merged
last_backend = None

MAX_COLUMNS = 128                   # DESCO_GCM_MAX_COLUMNS (include/desco_hip.h)
DEVICE_MAX_ROWS = 20480             # DESCO_GCM_DEV_MAX_ROWS: one int64 column in the 160 KiB of LDS
WAVE_ROWS = 256                     # DESCO_GCM_WAVE_ROWS: a launch bound up to this runs one wave per column
HOST_MAX_ROWS = 2097151             # n'^3 < 2^63
NOT_LAUNCHED = 1                    # ``status`` of a segment that no launch of the call held
_BACKENDS = ("auto", "host", "device")
# what "auto" does with a GPU present, per stage: the device only where it won on both measured shapes
# (tools/bench_graph_comparison.py)
AUTO_DEVICE = {"gcm": True, "gcd": True,
               # the degree distributions (tools/bench_gdd.py): "gdd" the builder, "gdda" the agreement
               "gdd": True, "gdda": True}


def _check_backend(backend):
    if backend not in _BACKENDS:
        raise ValueError(f"unknown backend {backend!r}: one of {_BACKENDS}")


def _use_device(backend: str, stage: str) -> bool:
    return backend == "device" or (backend == "auto" and AUTO_DEVICE[stage] and torch.cuda.is_available())


def orbit_set(orbits="gcd11") -> np.ndarray:
    """int32 column indices, into ``orbit_columns()``, of a named set ("all5", "all4", "gcd11") or of an explicit list."""
    if isinstance(orbits, str):
        flat, cols = gt._orbit_queries(None), gt.orbit_columns()
        size = lambda qi: flat[qi][0]                                                    # noqa: E731
        edges = lambda qi: len(flat[qi][1])                                              # noqa: E731
        if orbits == "all5":
            keep = [True] * len(cols)
        elif orbits == "all4":
            keep = [size(qi) <= 4 for qi, _, _ in cols]
        elif orbits == "gcd11":     # without the triangle, the diamond (4 nodes, 5 edges) and K4 (4 nodes, 6 edges)
            keep = [size(qi) <= 4 and (size(qi), edges(qi)) not in ((3, 3), (4, 5), (4, 6)) for qi, _, _ in cols]
        else:
            raise ValueError(f"unknown orbit set {orbits!r}: 'all5', 'all4', 'gcd11' or a list of column indices")
        return np.flatnonzero(keep).astype(np.int32)
    idx = np.asarray(orbits, dtype=np.int64).reshape(-1)
    if len(idx) and (idx.min() < 0 or idx.max() >= len(gt.orbit_columns())):
        raise ValueError("orbit column index outside orbit_columns()")
    if len(idx) > MAX_COLUMNS:
        raise ValueError(f"at most {MAX_COLUMNS} columns")
    return idx.astype(np.int32)


def _table_queries(columns: np.ndarray):
    """The queries whose orbit table holds ``columns``: the graphs of 2..4 nodes (15 columns, a prefix of the 73) when
    that is enough, else all of 2..5."""
    kmax = 4 if (len(columns) == 0 or int(columns.max()) < 15) else 5
    return [(k, tuple(e)) for k in range(2, kmax + 1) for _, e in gt.census_classes(k)]


def _host_table(graphs: GraphSet, flat, induced: bool, num_threads: int) -> np.ndarray:
    """``groundtruth.orbit_counts`` on the host, kept as int64."""
    reps, index, sizes, first, width = gt._orbit_select(flat, induced)
    raw = gt._orbit_host_raw(graphs, reps, num_threads)
    if not induced:
        raw = np.concatenate([raw[:, first[k]:first[k] + width[k]] @ gt.orbit_noninduced_matrix(k) for k in sizes],
                             axis=1)
    return np.ascontiguousarray(raw[:, index])


def _segments(graphs, segments, num_rows: int) -> np.ndarray:
    seg = np.ascontiguousarray(graphs.graph_ptr if segments is None else segments, dtype=np.int64).reshape(-1)
    if len(seg) < 1 or seg[0] < 0 or (np.diff(seg) < 0).any() or seg[-1] > num_rows:
        raise ValueError("segments must be a monotone row pointer inside the table")
    return seg


def _upper(C: int):
    return np.triu_indices(C, 1)


class GraphletCorrelation:
    """Graphlet correlation matrices of S segments over C orbit columns: ``S`` int64 [S, C, C], ``rho`` float64
    [S, C, C], ``columns`` int32 [C] (indices into ``orbit_columns()``), ``vector()`` float64 [S, C (C - 1) / 2] -- the
    upper triangles in row-major order, what ``gcd`` compares.  numpy arrays from ``graphlet_correlation``, tensors on
    the GPU from ``graphlet_correlation_device`` (``cpu()`` brings them over), which also sets ``status`` int32 [S]: 0
    for a computed segment, -1 for one the kernel refused, ``NOT_LAUNCHED`` for one outside ``segment_ids``."""

    def __init__(self, S, rho, columns, vec=None, status=None, backend=None):
        self.S, self.rho, self.columns, self._vec, self.status, self.last_backend = S, rho, columns, vec, status, backend

    def vector(self):
        if self._vec is None:
            iu = _upper(len(self.columns))
            if isinstance(self.rho, torch.Tensor):
                self._vec = self.rho[:, torch.as_tensor(iu[0], device=self.rho.device),
                                     torch.as_tensor(iu[1], device=self.rho.device)].contiguous()
            else:
                self._vec = np.ascontiguousarray(self.rho[:, iu[0], iu[1]])
        return self._vec

    def cpu(self) -> "GraphletCorrelation":
        host = lambda x: x.cpu().numpy() if isinstance(x, torch.Tensor) else x          # noqa: E731
        return GraphletCorrelation(host(self.S), host(self.rho), self.columns, host(self._vec), host(self.status),
                                   self.last_backend)

    def __len__(self):
        return self.S.shape[0]


def _gcm_host(table: np.ndarray, seg: np.ndarray, columns: np.ndarray, dummy_row: bool, num_threads: int):
    """desco_graphlet_correlation on an int64 table: (S, rho) numpy arrays."""
    nseg, C = len(seg) - 1, len(columns)
    S = np.zeros((nseg, C, C), dtype=np.int64)
    rho = np.zeros((nseg, C, C), dtype=np.float64)
    table = np.ascontiguousarray(table, dtype=np.int64)
    if (np.diff(seg) + int(dummy_row) > HOST_MAX_ROWS).any():
        raise ValueError(f"a segment has more than {HOST_MAX_ROWS} rows")
    ptr = lambda a: a.ctypes.data if a.size else None                                   # noqa: E731
    _lib.check(_lib.lib().desco_graphlet_correlation(seg.ctypes.data, nseg, ptr(table), table.shape[1], ptr(columns),
                                                     C, int(dummy_row), ptr(S), ptr(rho), num_threads),
               "desco_graphlet_correlation")
    return S, rho


def _gcm_device(table: torch.Tensor, seg: np.ndarray, columns: np.ndarray, dummy_row: bool, ids=None,
                max_rows: int = None, keep_ranks: bool = False) -> GraphletCorrelation:
    """The kernels on the segments ``ids`` (default: all) of an int64 table on the GPU.  One launch pair per size class:
    the segments up to WAVE_ROWS rows, and the others with the bound min(largest, DEVICE_MAX_ROWS) -- a segment above
    it is refused by the kernel (status -1).  ``max_rows``: one launch pair with that bound instead.  ``keep_ranks``: the
    result's ``ranks`` is the int32 workspace [N + S, C] of the doubled ranks, segment s from row seg[s] + s."""
    L = _lib.lib()
    dev = table.device
    if table.dtype != torch.int64 or table.dim() != 2 or not table.is_cuda:
        raise RuntimeError("graphlet_correlation_device takes an int64 [N, columns] table on the GPU (no CPU fallback)")
    table = table.contiguous()
    N, ld = table.shape
    nseg, C = len(seg) - 1, len(columns)
    P = C * (C - 1) // 2
    S = torch.zeros((nseg, C, C), dtype=torch.int64, device=dev)
    rho = torch.zeros((nseg, C, C), dtype=torch.float64, device=dev)
    vec = torch.zeros((nseg, P), dtype=torch.float64, device=dev)
    status = torch.full((nseg,), NOT_LAUNCHED, dtype=torch.int32, device=dev)
    ids = np.arange(nseg, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    if len(ids) and (ids.min() < 0 or ids.max() >= nseg):
        raise ValueError("segment_ids outside the segments")
    if len(ids) == 0 or C == 0:
        if C == 0:
            status[torch.from_numpy(ids).to(dev)] = 0
        return GraphletCorrelation(S, rho, columns, vec, status, "device")
    rows = np.diff(seg) + int(dummy_row)
    seg_d = gt._put(seg, np.int64, dev)
    work = torch.empty((N + nseg, C), dtype=torch.int32, device=dev)
    if max_rows is not None:
        launches = [(ids, int(max_rows))]
    else:
        small, large = ids[rows[ids] <= WAVE_ROWS], ids[rows[ids] > WAVE_ROWS]
        launches = [(small, int(rows[small].max()) if len(small) else 0),
                    (large, min(int(rows[large].max()), DEVICE_MAX_ROWS) if len(large) else 0)]
    keep = []
    ptr = lambda x: x.data_ptr() if x.numel() else None                                 # noqa: E731
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        for mine, bound in launches:
            if len(mine) == 0:
                continue
            every = len(mine) == nseg and (mine == np.arange(nseg)).all()
            ids_d = None if every else gt._put(mine, np.int64, dev)
            keep.append(ids_d)
            _lib.check(L.desco_graphlet_correlation_dev(seg_d.data_ptr(), nseg, N, ptr(table), ld, columns.ctypes.data,
                                                        C, int(dummy_row), None if every else ids_d.data_ptr(),
                                                        len(mine), bound, work.data_ptr(), S.data_ptr(),
                                                        rho.data_ptr(), ptr(vec), status.data_ptr(), stream),
                       "desco_graphlet_correlation_dev")
        torch.cuda.current_stream(dev).synchronize()                # the id lists and the workspace are released here
    res = GraphletCorrelation(S, rho, columns, vec, status, "device")
    if keep_ranks:
        res.ranks = work
    return res


def graphlet_correlation_device(graphs: GraphSet = None, orbits="gcd11", induced: bool = True, dummy_row: bool = True,
                                segments=None, device="cuda", table: torch.Tensor = None,
                                segment_ids=None) -> GraphletCorrelation:
    """``graphlet_correlation`` by the gfx950 kernels, everything kept on the GPU.  ``table``: an int64 orbit table that
    is there already (``groundtruth.orbit_counts_device``; the columns of ``orbits`` index it), otherwise it is computed
    from ``graphs``.  ``segment_ids``: only these segments are computed and written.  A segment of more than
    ``DEVICE_MAX_ROWS`` rows, the dummy row included, is refused by the kernel: its ``status`` is -1 and its rows hold
    zeros -- ``graphlet_correlation(backend="auto")`` sends those to the host twin instead."""
    columns = orbit_set(orbits)
    if table is None:
        if graphs is None:
            raise ValueError("graphlet_correlation_device needs graphs or a table")
        table = gt.orbit_counts_device(graphs, _table_queries(columns), device, induced)
    if len(columns) and int(columns.max()) >= table.shape[1]:
        raise ValueError("the table does not hold the columns asked for")
    if graphs is None and segments is None:
        raise ValueError("a table without graphs needs segments")
    return _gcm_device(table, _segments(graphs, segments, table.shape[0]), columns, dummy_row, segment_ids)


def _merge_refused(res: GraphletCorrelation, table: torch.Tensor, seg: np.ndarray, dummy_row: bool,
                   num_threads: int) -> GraphletCorrelation:
    """``res`` on the host, the segments the kernel refused computed by the twin."""
    out = res.cpu()
    refused = np.flatnonzero(out.status == -1)
    if len(refused) == 0:
        return out
    vec = out.vector()
    iu = _upper(len(out.columns))
    for s in refused:
        part = table[int(seg[s]):int(seg[s + 1])].cpu().numpy()
        S, rho = _gcm_host(part, np.array([0, part.shape[0]], dtype=np.int64), out.columns, dummy_row, num_threads)
        out.S[s], out.rho[s], out.status[s] = S[0], rho[0], 0
        vec[s] = rho[0][iu]
    out.last_backend = "device+host"
    return out


def graphlet_correlation(graphs: GraphSet, orbits="gcd11", induced: bool = True, dummy_row: bool = True,
                         segments=None, backend: str = "auto", num_threads: int = 0) -> GraphletCorrelation:
    """The graphlet correlation matrix of every segment of ``graphs`` (default: of every graph) over the orbit columns
    ``orbits`` (module docstring), numpy arrays in a ``GraphletCorrelation``.  ``induced=False`` passes through to the
    orbit counts.  ``segments``: an int64 row pointer [S + 1] over the nodes instead of ``graph_ptr``.

    ``backend``: "host" (OpenMP twin, ``num_threads`` threads, orbit counts on the host too), "device" (HIP kernels;
    every segment must fit ``DEVICE_MAX_ROWS``), or "auto": the device when there is one, the orbit table staying
    there, segments above its row bound going to the host twin and being merged (``last_backend`` then reads
    "device+host")."""
    global last_backend
    _check_backend(backend)
    columns = orbit_set(orbits)
    flat = _table_queries(columns)
    if not _use_device(backend, "gcm"):
        if backend == "auto" and torch.cuda.is_available():
            table = gt.orbit_counts_device(graphs, flat, "cuda", induced).cpu().numpy()
        else:
            table = _host_table(graphs, flat, induced, num_threads)
        seg = _segments(graphs, segments, table.shape[0])
        S, rho = _gcm_host(table, seg, columns, dummy_row, num_threads)
        res = GraphletCorrelation(S, rho, columns, None, None, "host")
    else:
        table = gt.orbit_counts_device(graphs, flat, "cuda", induced)
        seg = _segments(graphs, segments, table.shape[0])
        res = _gcm_device(table, seg, columns, dummy_row)
        if backend == "device":
            if bool((res.status != 0).any()):
                raise RuntimeError(f"graphlet_correlation: a segment has more than {DEVICE_MAX_ROWS} rows "
                                   "(DESCO_GCM_DEV_MAX_ROWS); use backend='auto' or 'host'")
            res = res.cpu()
        else:
            res = _merge_refused(res, table, seg, dummy_row, num_threads)
    last_backend = res.last_backend
    return res


def _vectors(a):
    return a.vector() if isinstance(a, GraphletCorrelation) else a


def _gcd_host(x: np.ndarray, y: np.ndarray, num_threads: int = 0, out: np.ndarray = None) -> np.ndarray:
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    if x.ndim != 2 or y.ndim != 2 or x.shape[1] != y.shape[1]:
        raise ValueError("gcd takes two [G, P] arrays of one width")
    if out is None:
        out = np.empty((x.shape[0], y.shape[0]), dtype=np.float64)
    ptr = lambda a: a.ctypes.data if a.size else None                                   # noqa: E731
    _lib.check(_lib.lib().desco_gcd_matrix(ptr(x), x.shape[0], ptr(y), y.shape[0], x.shape[1], ptr(out),
                                           out.strides[0] // 8 if out.size else y.shape[0], num_threads),
               "desco_gcd_matrix")
    return out


def gcd_device(a, b=None, out: torch.Tensor = None, device="cuda") -> torch.Tensor:
    """``gcd`` by the gfx950 kernel: float64 [Ga, Gb] on the GPU.  ``a`` / ``b``: ``GraphletCorrelation`` objects or
    [G, P] arrays or tensors (host ones are uploaded).  ``out``: a float64 view on the GPU with unit column stride to
    write into (a block of a larger matrix); only its [Ga, Gb] elements are written."""
    dev = torch.device(device)
    put = lambda v: (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))).to(      # noqa: E731
        dev, torch.float64).contiguous()
    x = put(_vectors(a))
    y = x if b is None else put(_vectors(b))
    if x.dim() != 2 or y.dim() != 2 or x.shape[1] != y.shape[1]:
        raise ValueError("gcd takes two [G, P] arrays of one width")
    if out is None:
        out = torch.empty((x.shape[0], y.shape[0]), dtype=torch.float64, device=x.device)
    if (not out.is_cuda or out.dtype != torch.float64 or out.shape != (x.shape[0], y.shape[0]) or
            (out.numel() and out.stride(1) != 1)):
        raise RuntimeError("gcd_device: out must be a float64 [Ga, Gb] view on the GPU with unit column stride")
    ptr = lambda t: t.data_ptr() if t.numel() else None                                 # noqa: E731
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().desco_gcd_matrix_dev(ptr(x), x.shape[0], ptr(y), y.shape[0], x.shape[1], ptr(out),
                                                   out.stride(0) if out.numel() else y.shape[0],
                                                   torch.cuda.current_stream(x.device).cuda_stream),
                   "desco_gcd_matrix_dev")
        if not (isinstance(_vectors(a), torch.Tensor) and (b is None or isinstance(_vectors(b), torch.Tensor))):
            torch.cuda.current_stream(x.device).synchronize()       # uploaded operands are released on return
    return out


def gcd(a, b=None, backend: str = "auto", num_threads: int = 0) -> np.ndarray:
    """The graphlet correlation distances between the segments of ``a`` and of ``b`` (default: ``a`` against itself):
    float64 [Ga, Gb].  ``a`` / ``b``: ``GraphletCorrelation`` objects or [G, P] arrays of vectors."""
    global last_backend
    _check_backend(backend)
    if _use_device(backend, "gcd"):
        out = gcd_device(a, b).cpu().numpy()
        last_backend = "device"
    else:
        host = lambda v: v.cpu().numpy() if isinstance(v, torch.Tensor) else v          # noqa: E731
        x = host(_vectors(a))
        out = _gcd_host(x, x if b is None else host(_vectors(b)), num_threads)
        last_backend = "host"
    return out


def nearest(train, target, k: int = 1, backend: str = "auto", num_threads: int = 0, chunk_rows: int = 2048):
    """For every segment of ``target`` its ``k`` nearest segments of ``train``: (indices int64 [Gt, k], distances
    float64 [Gt, k]), nearest first, equal distances in ascending index.  The distance matrix is built ``chunk_rows``
    target rows at a time and never held whole."""
    global last_backend
    _check_backend(backend)
    host = lambda v: v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)  # noqa: E731
    use_dev = _use_device(backend, "gcd")
    x, y = _vectors(target), _vectors(train)
    if use_dev:
        put = lambda v: (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))).to(  # noqa: E731
            "cuda", torch.float64).contiguous()
        x, y = put(x), put(y)
    else:
        x, y = host(x), host(y)
    Gt, Gr = x.shape[0], y.shape[0]
    if k < 1 or k > Gr:
        raise ValueError("k must be in 1 .. the number of training segments")
    idx = np.zeros((Gt, k), dtype=np.int64)
    dist = np.zeros((Gt, k), dtype=np.float64)
    for r0 in range(0, Gt, max(int(chunk_rows), 1)):
        r1 = min(Gt, r0 + max(int(chunk_rows), 1))
        if use_dev:
            d, order = torch.sort(gcd_device(x[r0:r1], y), dim=1, stable=True)
            idx[r0:r1], dist[r0:r1] = order[:, :k].cpu().numpy(), d[:, :k].cpu().numpy()
        else:
            d = _gcd_host(x[r0:r1], y, num_threads)
            order = np.argsort(d, axis=1, kind="stable")[:, :k]
            idx[r0:r1], dist[r0:r1] = order, np.take_along_axis(d, order, axis=1)
    last_backend = "device" if use_dev else "host"
    return idx, dist


def dataset_gcd(a, b=None, orbits="gcd11", induced: bool = True, dummy_row: bool = True, backend: str = "auto",
                num_threads: int = 0) -> np.ndarray:
    """Distances between whole data sets: ``a`` and ``b`` (default: ``a``) are lists of GraphSets, and all the nodes of
    a set form ONE segment.  float64 [len(a), len(b)].  A set of more than ``DEVICE_MAX_ROWS`` nodes -- the
    Syn_1827-shaped set has 246 473 -- is above the kernel's row bound, so with "auto" its matrix comes from the host
    twin (the orbit counts still from the device)."""
    global last_backend
    one = lambda g: graphlet_correlation(g, orbits, induced, dummy_row,                 # noqa: E731
                                         np.array([0, g.num_nodes], dtype=np.int64), backend, num_threads)
    ra = [one(g) for g in ([a] if isinstance(a, GraphSet) else a)]
    rb = ra if b is None else [one(g) for g in ([b] if isinstance(b, GraphSet) else b)]
    used = {r.last_backend for r in ra + rb}
    va, vb = np.concatenate([r.vector() for r in ra]), np.concatenate([r.vector() for r in rb])
    out = _gcd_host(va, vb, num_threads)
    last_backend = used.pop() if len(used) == 1 else "device+host"
    return out


# ---- graphlet degree distributions and their agreement (GDDA; Przulj 2007) ------------------------------------------------
# Where the correlation matrices above compare the SHAPE of the orbit columns -- two complete graphs of different sizes are
# at distance 0 -- the degree distributions compare their magnitudes: per segment and column the list of (k, N(k)), how
# much of the segment touches the orbit k times, and per pair of segments 1 - the scaled Euclidean distance of the two
# lists, averaged over the columns.  The arithmetic is defined in include/desco_hip.h, "GRAPHLET DEGREE DISTRIBUTION";
# the host twin (csrc/graphlet_distribution.cpp) and the gfx950 kernels (csrc/graphlet_distribution_dev.hip) return the
# same bits.  mean="geometric" is formed here from the per-orbit agreements and is NOT bit-defined.

class GraphletDistribution:
    """The graphlet degree distributions of S segments over C orbit columns in the layout of the C ABI: ``len`` int32
    [S, C], ``key`` int64 [N * C], ``val`` float64 [N * C] -- the list of (s, c) starts at ``seg[s] * C + c * n_s`` --,
    ``seg`` int64 [S + 1] (always a numpy array), ``columns`` int32 [C].  numpy arrays from ``graphlet_distribution``,
    tensors on the GPU from ``graphlet_distribution_device`` (``cpu()`` / ``cuda()`` move them), which also sets
    ``status`` int32 [S]: 0 computed, -1 refused by the kernel, ``NOT_LAUNCHED`` outside ``segment_ids``."""

    def __init__(self, len_, key, val, seg, columns, status=None, backend=None):
        self.len, self.key, self.val, self.seg, self.columns = len_, key, val, seg, columns
        self.status, self.last_backend = status, backend
        self._seg_dev = None

    @property
    def on_device(self) -> bool:
        return isinstance(self.key, torch.Tensor)

    def cpu(self) -> "GraphletDistribution":
        host = lambda x: x.cpu().numpy() if isinstance(x, torch.Tensor) else x          # noqa: E731
        return GraphletDistribution(host(self.len), host(self.key), host(self.val), self.seg, self.columns,
                                    host(self.status), self.last_backend)

    def cuda(self, device="cuda") -> "GraphletDistribution":
        if self.on_device:
            return self
        put = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(device)   # noqa: E731
        return GraphletDistribution(put(self.len), put(self.key), put(self.val), self.seg, self.columns,
                                    put(self.status), self.last_backend)

    def rows(self, r0: int, r1: int) -> "GraphletDistribution":
        """The segments r0 .. r1 - 1 as a view: the same key / val arrays, a slice of ``seg`` and ``len``."""
        return GraphletDistribution(self.len[r0:r1], self.key, self.val, self.seg[r0:r1 + 1], self.columns,
                                    None if self.status is None else self.status[r0:r1], self.last_backend)

    def lists(self, s: int):
        """[(keys, vals)] of segment s, one pair of arrays per column."""
        C, a, n = len(self.columns), int(self.seg[s]), int(self.seg[s + 1] - self.seg[s])
        host = lambda x: x.cpu().numpy() if isinstance(x, torch.Tensor) else x          # noqa: E731
        ln = host(self.len[s])
        key, val = host(self.key[a * C:(a + n) * C]), host(self.val[a * C:(a + n) * C])
        return [(key[c * n:c * n + int(ln[c])].copy(), val[c * n:c * n + int(ln[c])].copy()) for c in range(C)]

    def __len__(self):
        return self.len.shape[0]


def _gdd_columns(orbits) -> np.ndarray:
    columns = orbit_set(orbits)
    if len(columns) < 1:
        raise ValueError("the degree distributions need at least one orbit column")
    return columns


def _gdd_host(table: np.ndarray, seg: np.ndarray, columns: np.ndarray, num_threads: int):
    """desco_gdd_build on an int64 table: (len, key, val) numpy arrays."""
    nseg, C = len(seg) - 1, len(columns)
    table = np.ascontiguousarray(table, dtype=np.int64)
    N = table.shape[0]
    ln = np.zeros((nseg, C), dtype=np.int32)
    key = np.zeros(N * C, dtype=np.int64)
    val = np.zeros(N * C, dtype=np.float64)
    ptr = lambda a: a.ctypes.data if a.size else None                                   # noqa: E731
    _lib.check(_lib.lib().desco_gdd_build(seg.ctypes.data, nseg, ptr(table), table.shape[1], ptr(columns), C, ptr(ln),
                                          ptr(key), ptr(val), num_threads), "desco_gdd_build")
    return ln, key, val


def _gdd_device(table: torch.Tensor, seg: np.ndarray, columns: np.ndarray, ids=None,
                max_rows: int = None) -> GraphletDistribution:
    """The builder kernel on the segments ``ids`` (default: all) of an int64 table on the GPU.  One launch per size
    class: the segments up to WAVE_ROWS rows, and the others with the bound min(largest, DEVICE_MAX_ROWS) -- a segment
    above it is refused by the kernel (status -1).  ``max_rows``: one launch with that bound instead."""
    L = _lib.lib()
    if not isinstance(table, torch.Tensor) or table.dtype != torch.int64 or table.dim() != 2 or not table.is_cuda:
        raise RuntimeError("graphlet_distribution_device takes an int64 [N, columns] table on the GPU (no CPU fallback)")
    dev = table.device
    table = table.contiguous()
    N, ld = table.shape
    nseg, C = len(seg) - 1, len(columns)
    ln = torch.zeros((nseg, C), dtype=torch.int32, device=dev)
    key = torch.zeros(N * C, dtype=torch.int64, device=dev)
    val = torch.zeros(N * C, dtype=torch.float64, device=dev)
    status = torch.full((nseg,), NOT_LAUNCHED, dtype=torch.int32, device=dev)
    ids = np.arange(nseg, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    if len(ids) and (ids.min() < 0 or ids.max() >= nseg):
        raise ValueError("segment_ids outside the segments")
    res = GraphletDistribution(ln, key, val, seg, columns, status, "device")
    if len(ids) == 0:
        return res
    rows = np.diff(seg)
    seg_d = gt._put(seg, np.int64, dev)
    res._seg_dev = seg_d
    if max_rows is not None:
        launches = [(ids, int(max_rows))]
    else:
        small, large = ids[rows[ids] <= WAVE_ROWS], ids[rows[ids] > WAVE_ROWS]
        launches = [(small, int(rows[small].max()) if len(small) else 0),
                    (large, min(int(rows[large].max()), DEVICE_MAX_ROWS) if len(large) else 0)]
    keep = []
    ptr = lambda x: x.data_ptr() if x.numel() else None                                 # noqa: E731
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        for mine, bound in launches:
            if len(mine) == 0:
                continue
            every = len(mine) == nseg and (mine == np.arange(nseg)).all()
            ids_d = None if every else gt._put(mine, np.int64, dev)
            keep.append(ids_d)
            _lib.check(L.desco_gdd_build_dev(seg_d.data_ptr(), nseg, N, ptr(table), ld, columns.ctypes.data, C,
                                             None if every else ids_d.data_ptr(), len(mine), bound, ln.data_ptr(),
                                             ptr(key), ptr(val), status.data_ptr(), stream), "desco_gdd_build_dev")
        torch.cuda.current_stream(dev).synchronize()                # the id lists are released here
    return res


def graphlet_distribution_device(graphs: GraphSet = None, orbits="all5", induced: bool = True, segments=None,
                                 device="cuda", table: torch.Tensor = None, segment_ids=None) -> GraphletDistribution:
    """``graphlet_distribution`` by the gfx950 kernel, everything kept on the GPU.  ``table``: an int64 orbit table that
    is there already (``groundtruth.orbit_counts_device``; the columns of ``orbits`` index it), otherwise it is computed
    from ``graphs``.  ``segment_ids``: only these segments are computed and written.  A segment of more than
    ``DEVICE_MAX_ROWS`` rows is refused by the kernel: its ``status`` is -1 and its slots hold zeros --
    ``graphlet_distribution(backend="auto")`` sends those to the host twin instead."""
    columns = _gdd_columns(orbits)
    if table is None:
        if graphs is None:
            raise ValueError("graphlet_distribution_device needs graphs or a table")
        table = gt.orbit_counts_device(graphs, _table_queries(columns), device, induced)
    if int(columns.max()) >= table.shape[1]:
        raise ValueError("the table does not hold the columns asked for")
    if graphs is None and segments is None:
        raise ValueError("a table without graphs needs segments")
    return _gdd_device(table, _segments(graphs, segments, table.shape[0]), columns, segment_ids)


def _gdd_merge_refused(res: GraphletDistribution, table: torch.Tensor, num_threads: int) -> GraphletDistribution:
    """``res`` on the host, the segments the kernel refused computed by the twin."""
    out = res.cpu()
    refused = np.flatnonzero(out.status == -1)
    if len(refused) == 0:
        return out
    C = len(out.columns)
    for s in refused:
        a, b = int(out.seg[s]), int(out.seg[s + 1])
        part = table[a:b].cpu().numpy()
        ln, key, val = _gdd_host(part, np.array([0, b - a], dtype=np.int64), out.columns, num_threads)
        out.len[s], out.key[a * C:b * C], out.val[a * C:b * C], out.status[s] = ln[0], key, val, 0
    out.last_backend = "device+host"
    return out


def graphlet_distribution(graphs: GraphSet, orbits="all5", induced: bool = True, segments=None, backend: str = "auto",
                          num_threads: int = 0) -> GraphletDistribution:
    """The graphlet degree distribution of every segment of ``graphs`` (default: of every graph) over the orbit columns
    ``orbits``: per column the values k >= 1 that occur, ascending, with N(k) = (d_k / k) / sum_k (d_k / k), d_k the
    nodes that touch the orbit k times.  numpy arrays in a ``GraphletDistribution``.  ``backend`` as for
    ``graphlet_correlation``: with "auto" segments above ``DEVICE_MAX_ROWS`` go to the host twin and are merged
    (``last_backend`` then reads "device+host")."""
    global last_backend
    _check_backend(backend)
    columns = _gdd_columns(orbits)
    flat = _table_queries(columns)
    if not _use_device(backend, "gdd"):
        if backend == "auto" and torch.cuda.is_available():
            table = gt.orbit_counts_device(graphs, flat, "cuda", induced).cpu().numpy()
        else:
            table = _host_table(graphs, flat, induced, num_threads)
        seg = _segments(graphs, segments, table.shape[0])
        res = GraphletDistribution(*_gdd_host(table, seg, columns, num_threads), seg, columns, None, "host")
    else:
        table = gt.orbit_counts_device(graphs, flat, "cuda", induced)
        seg = _segments(graphs, segments, table.shape[0])
        res = _gdd_device(table, seg, columns)
        if backend == "device":
            if bool((res.status != 0).any()):
                raise RuntimeError(f"graphlet_distribution: a segment has more than {DEVICE_MAX_ROWS} rows "
                                   "(DESCO_GCM_DEV_MAX_ROWS); use backend='auto' or 'host'")
            res = res.cpu()
        else:
            res = _gdd_merge_refused(res, table, num_threads)
    last_backend = res.last_backend
    return res


def _geometric(per: "np.ndarray | torch.Tensor"):
    """exp(mean(log A_c)) over the last axis, 0 where any A_c is 0.  Not bit-defined: log and exp are library calls."""
    if isinstance(per, torch.Tensor):
        zero = (per == 0).any(dim=-1)
        g = torch.exp(torch.log(torch.where(per == 0, torch.ones_like(per), per)).mean(dim=-1))
        return torch.where(zero, torch.zeros_like(g), g)
    zero = (per == 0).any(axis=-1)
    g = np.exp(np.log(np.where(per == 0, 1.0, per)).mean(axis=-1))
    return np.where(zero, 0.0, g)


def _gdda_host(a: GraphletDistribution, b: GraphletDistribution, per_orbit: bool, num_threads: int = 0,
               out: np.ndarray = None):
    """desco_gdd_agreement: (agree [Ga, Gb], per_orbit [Ga, Gb, C] or None)."""
    Ga, Gb, C = len(a), len(b), len(a.columns)
    if out is None:
        out = np.empty((Ga, Gb), dtype=np.float64)
    per = np.empty((Ga, Gb, C), dtype=np.float64) if per_orbit else None
    ptr = lambda x: x.ctypes.data if x is not None and x.size else None                 # noqa: E731
    cont = lambda x, t: np.ascontiguousarray(x, dtype=t)                                # noqa: E731
    al, bl, aseg, bseg = cont(a.len, np.int32), cont(b.len, np.int32), cont(a.seg, np.int64), cont(b.seg, np.int64)
    _lib.check(_lib.lib().desco_gdd_agreement(aseg.ctypes.data, ptr(al), ptr(a.key), ptr(a.val), Ga, bseg.ctypes.data,
                                              ptr(bl), ptr(b.key), ptr(b.val), Gb, C, ptr(out),
                                              out.strides[0] // 8 if out.size else Gb, ptr(per), num_threads),
               "desco_gdd_agreement")
    return out, per


def _seg_on(d: GraphletDistribution, dev) -> torch.Tensor:
    if d._seg_dev is None or d._seg_dev.device != dev or d._seg_dev.numel() != len(d.seg):
        d._seg_dev = gt._put(np.ascontiguousarray(d.seg, dtype=np.int64), np.int64, dev)
    return d._seg_dev


def _gdda_device(a: GraphletDistribution, b: GraphletDistribution, per_orbit: bool, out: torch.Tensor = None):
    """desco_gdd_agreement_dev: (agree [Ga, Gb], per_orbit [Ga, Gb, C] or None), tensors on the GPU."""
    for d in (a, b):
        if not d.on_device or not d.key.is_cuda:
            raise RuntimeError("gdd_agreement_device takes distributions on the GPU (no CPU fallback); "
                               "GraphletDistribution.cuda() uploads host-built ones")
    dev = a.key.device
    Ga, Gb, C = len(a), len(b), len(a.columns)
    if out is None:
        out = torch.empty((Ga, Gb), dtype=torch.float64, device=dev)
    if (not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.float64 or
            tuple(out.shape) != (Ga, Gb) or (out.numel() and out.stride(1) != 1)):
        raise RuntimeError("gdd_agreement_device: out must be a float64 [Ga, Gb] view on the GPU with unit column stride")
    per = torch.empty((Ga, Gb, C), dtype=torch.float64, device=dev) if per_orbit else None
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None               # noqa: E731
    al, bl = a.len.contiguous(), b.len.contiguous()
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().desco_gdd_agreement_dev(_seg_on(a, dev).data_ptr(), ptr(al), ptr(a.key), ptr(a.val), Ga,
                                                      _seg_on(b, dev).data_ptr(), ptr(bl), ptr(b.key), ptr(b.val), Gb,
                                                      C, ptr(out), out.stride(0) if out.numel() else Gb, ptr(per),
                                                      torch.cuda.current_stream(dev).cuda_stream),
                   "desco_gdd_agreement_dev")
        if al.data_ptr() != a.len.data_ptr() or bl.data_ptr() != b.len.data_ptr():
            torch.cuda.current_stream(dev).synchronize()            # contiguous copies are released on return
    return out, per


def _gdd_pair(a, b):
    b = a if b is None else b
    if not isinstance(a, GraphletDistribution) or not isinstance(b, GraphletDistribution):
        raise ValueError("gdd_agreement takes GraphletDistribution objects")
    if not np.array_equal(a.columns, b.columns):
        raise ValueError("the two distributions are over different orbit columns")
    return a, b


def _check_mean(mean):
    if mean not in ("arithmetic", "geometric"):
        raise ValueError(f"unknown mean {mean!r}: 'arithmetic' or 'geometric'")


def _gdda(one, a, b, mean, per_orbit, chunk_rows, out, empty, cat):
    """The agreement matrix of ``a`` x ``b`` by ``one(a_rows, b, per_orbit, out_rows)``.  The arithmetic mean needs no
    per-orbit values; the geometric mean is formed ``chunk_rows`` rows of ``a`` at a time so that [Ga, Gb, C] is held
    whole only where the caller asked for it."""
    Ga, Gb = len(a), len(b)
    if mean == "arithmetic":
        return one(a, b, per_orbit, out)
    if out is None:
        out = empty((Ga, Gb))
    step, pers = max(int(chunk_rows), 1), []
    for r0 in range(0, Ga, step):
        r1 = min(Ga, r0 + step)
        _, per = one(a.rows(r0, r1), b, True, None)
        out[r0:r1] = _geometric(per)
        if per_orbit:
            pers.append(per)
    return out, (cat(pers) if per_orbit else None)


def gdd_agreement_device(a: GraphletDistribution, b: GraphletDistribution = None, mean: str = "arithmetic",
                         per_orbit: bool = False, out: torch.Tensor = None, chunk_rows: int = 256):
    """``gdd_agreement`` by the gfx950 kernel on distributions that are on the GPU: float64 [Ga, Gb] there (and the
    per-orbit tensor with ``per_orbit``).  ``out``: a float64 view on the GPU with unit column stride to write into;
    only its [Ga, Gb] elements are written."""
    _check_mean(mean)
    a, b = _gdd_pair(a, b)
    dev = a.key.device if a.on_device else "cpu"
    agree, per = _gdda(_gdda_device, a, b, mean, per_orbit, chunk_rows, out,
                       lambda shape: torch.empty(shape, dtype=torch.float64, device=dev),
                       lambda ps: torch.cat(ps) if ps else torch.empty((0, len(b), len(a.columns)), dtype=torch.float64,
                                                                       device=dev))
    return (agree, per) if per_orbit else agree


def gdd_agreement(a: GraphletDistribution, b: GraphletDistribution = None, mean: str = "arithmetic",
                  per_orbit: bool = False, backend: str = "auto", num_threads: int = 0, chunk_rows: int = 256):
    """The graphlet degree distribution agreement between the segments of ``a`` and of ``b`` (default: ``a`` against
    itself): float64 [Ga, Gb] in 0 .. 1, 1 for equal distributions; with ``per_orbit`` also the agreements A_c per
    column, [Ga, Gb, C].  ``mean``: "arithmetic" (Przulj's, bit-defined) or "geometric" -- exp(mean(log A_c)), 0 if any
    A_c is 0, formed in Python from the per-orbit values and not bit-defined."""
    global last_backend
    _check_backend(backend)
    _check_mean(mean)
    a, b = _gdd_pair(a, b)
    if _use_device(backend, "gdda"):
        same = b is a
        a = a.cuda()
        b = a if same else b.cuda()
        res = gdd_agreement_device(a, b, mean, per_orbit, None, chunk_rows)
        res = tuple(r.cpu().numpy() for r in res) if per_orbit else res.cpu().numpy()
        last_backend = "device"
    else:
        same = b is a
        a = a.cpu()
        b = a if same else b.cpu()
        agree, per = _gdda(lambda x, y, po, out: _gdda_host(x, y, po, num_threads, out), a, b, mean, per_orbit,
                           chunk_rows, None, lambda shape: np.empty(shape, dtype=np.float64),
                           lambda ps: np.concatenate(ps) if ps else np.empty((0, len(b), len(a.columns))))
        res = (agree, per) if per_orbit else agree
        last_backend = "host"
    return res


def gdd_nearest(train: GraphletDistribution, target: GraphletDistribution, k: int = 1, backend: str = "auto",
                num_threads: int = 0, chunk_rows: int = 2048):
    """For every segment of ``target`` the ``k`` segments of ``train`` it agrees with best: (indices int64 [Gt, k],
    agreements float64 [Gt, k]), largest agreement first, equal agreements in ascending index.  The matrix is built
    ``chunk_rows`` target rows at a time and never held whole."""
    global last_backend
    _check_backend(backend)
    target, train = _gdd_pair(target, train)
    use_dev = _use_device(backend, "gdda")
    x, y = (target.cuda(), train.cuda()) if use_dev else (target.cpu(), train.cpu())
    Gt, Gr = len(x), len(y)
    if k < 1 or k > Gr:
        raise ValueError("k must be in 1 .. the number of training segments")
    idx = np.zeros((Gt, k), dtype=np.int64)
    agree = np.zeros((Gt, k), dtype=np.float64)
    step = max(int(chunk_rows), 1)
    for r0 in range(0, Gt, step):
        r1 = min(Gt, r0 + step)
        if use_dev:
            d, order = torch.sort(_gdda_device(x.rows(r0, r1), y, False)[0], dim=1, descending=True, stable=True)
            idx[r0:r1], agree[r0:r1] = order[:, :k].cpu().numpy(), d[:, :k].cpu().numpy()
        else:
            d, _ = _gdda_host(x.rows(r0, r1), y, False, num_threads)
            order = np.argsort(-d, axis=1, kind="stable")[:, :k]
            idx[r0:r1], agree[r0:r1] = order, np.take_along_axis(d, order, axis=1)
    last_backend = "device" if use_dev else "host"
    return idx, agree


def _gdd_concat(parts) -> GraphletDistribution:
    """Host distributions that each cover their whole table, as one: the tables stacked."""
    C = len(parts[0].columns)
    seg, base = [np.zeros(1, dtype=np.int64)], 0
    for p in parts:
        if int(p.seg[0]) != 0 or int(p.seg[-1]) * C != len(p.key):
            raise ValueError("only distributions over whole tables can be joined")
        seg.append(np.asarray(p.seg[1:], dtype=np.int64) + base)
        base += int(p.seg[-1])
    return GraphletDistribution(np.concatenate([p.len for p in parts]), np.concatenate([p.key for p in parts]),
                                np.concatenate([p.val for p in parts]), np.concatenate(seg), parts[0].columns)


def dataset_gdda(a, b=None, orbits="all5", induced: bool = True, mean: str = "arithmetic", backend: str = "auto",
                 num_threads: int = 0) -> np.ndarray:
    """Agreement between whole data sets: ``a`` and ``b`` (default: ``a``) are lists of GraphSets, and all the nodes of a
    set form ONE segment.  float64 [len(a), len(b)].  A set of more than ``DEVICE_MAX_ROWS`` nodes is above the
    builder kernel's row bound, so with "auto" its distribution comes from the host twin, as in ``dataset_gcd``."""
    global last_backend
    one = lambda g: graphlet_distribution(g, orbits, induced, np.array([0, g.num_nodes], dtype=np.int64),     # noqa: E731
                                          backend, num_threads)
    ra = [one(g) for g in ([a] if isinstance(a, GraphSet) else a)]
    rb = ra if b is None else [one(g) for g in ([b] if isinstance(b, GraphSet) else b)]
    used = {r.last_backend for r in ra + rb}
    da = _gdd_concat(ra)
    out = gdd_agreement(da, da if b is None else _gdd_concat(rb), mean, False, backend, num_threads)
    used.add(last_backend)
    last_backend = used.pop() if len(used) == 1 else "device+host"
    return out
