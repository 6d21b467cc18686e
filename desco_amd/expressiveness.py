"""Expressiveness bounds: which neighborhoods (or whole graphs) a model family cannot tell apart whatever its weights.

A layer of every model here maps a row to a function of its own state and, per relation slot, the SUM over its
neighbours' states; the head reads the anchor row and the sum over the count rows.  Two neighborhoods that agree under L
rounds of colour refinement (1-WL on the typed CSR, the relation slots grouped the way the family groups them) therefore
get the same prediction from every L-layer model of that family, and where their exact counts differ that difference is
an error floor.  ``refine`` runs the refinement (definition: include/desco_hip.h, "COLOUR REFINEMENT") with the host twin
(csrc/wl_refine.cpp, OpenMP over segments) or the gfx950 kernel (csrc/wl_refine_dev.hip: all rounds of a segment in one
launch, both colour buffers in LDS); every sum is modulo 2^64, so the two agree bit for bit.  The colours are 64-bit
hashes: the classes are exact up to a hash collision, which would merge two of them.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .batch import GraphBatch, NeighborhoodBatch
from .graphs import GraphSet
from .partition import NeighborhoodPartition, build_partition, build_partition_device

# the relation slots a family pools together, by name.  "shmp": every slot its own group (the SHMP model); "hetero": the
# triangle / tride bit merged (use_tconv=False; the 4-slot neighborhood layout only); "plain": all slots merged (the
# homogeneous SAGE / GIN / GCN models)
VIEWS = ("shmp", "hetero", "plain")

# who served the last call: "host", "device", or "device+host" when segments above the device's bound were refined by the
# host twin and merged
last_backend = None

MAX_ROUNDS = 64                     # DESCO_WL_MAX_ROUNDS (include/desco_hip.h)
DEVICE_MAX_ROWS = 10236             # DESCO_WL_DEV_MAX_ROWS: the rows, anchor included, of the largest segment the kernel takes
WAVE_ROWS = 128                     # DESCO_WL_WAVE_ROWS: a launch bound up to this runs one wave per segment
_BUCKETS = (WAVE_ROWS, 1024, 4096, DEVICE_MAX_ROWS)         # rows per segment: one launch per bucket
_BACKENDS = ("auto", "host", "device")
NOT_LAUNCHED = 1                    # ``status`` of a segment that no launch of the call held

Block = namedtuple("Block", "vrowptr vcol num_rows slots seg_ptr anchor_base")
Block.__doc__ = """Explicit arrays for ``refine``: vrowptr int32 [slots * num_rows + 1], vcol int32 [E], seg_ptr int32 [S + 1]
(numpy arrays or tensors), anchor_base (-1: no anchors)."""


def view_groups(view, slots: int) -> tuple:
    """The ``group`` array of a view name (or of an explicit tuple, checked) on a ``slots``-slot layout."""
    if isinstance(view, str):
        if view not in VIEWS:
            raise ValueError(f"unknown view {view!r}: one of {VIEWS}")
        if view == "shmp":
            return tuple(range(slots))
        if view == "plain":
            return (0,) * slots
        if slots != 4:
            raise ValueError('view "hetero" merges the triangle / tride bit of the 4-slot neighborhood layout; it is not '
                             f"defined for a {slots}-slot block (whole graphs)")
        return (0, 0, 1, 1)
    group = tuple(int(g) for g in view)
    if len(group) != slots:
        raise ValueError(f"group has {len(group)} entries for {slots} slots")
    return group


def _block(batch) -> Block:
    if isinstance(batch, Block):
        return batch
    if isinstance(batch, NeighborhoodBatch):
        return Block(batch.vrowptr, batch.vcol, batch.num_rows, 4, batch.count_ptr, batch.num_count)
    if isinstance(batch, GraphBatch):
        return Block(batch.vrowptr, batch.vcol, batch.num_rows, 2, batch.graph_ptr, -1)
    if isinstance(batch, NeighborhoodPartition):
        da = batch.device_arrays
        if da is not None:
            return Block(da["vrowptr"], da["vcol"], batch.num_rows, 4, da["count_ptr"], batch.num_count)
        return Block(batch.vrowptr, batch.vcol, batch.num_rows, 4, batch.count_ptr, batch.num_count)
    raise TypeError(f"refine: a NeighborhoodBatch, GraphBatch, NeighborhoodPartition or Block, not {type(batch).__name__}")


def _np(a, dt):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=dt)


def _dev(a, dt, dev):
    if isinstance(a, torch.Tensor):
        return a.to(device=dev, dtype=dt).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)


class Refinement:
    """``signature`` int64 [S]; ``colours`` int64 [R], the rows' final colours (None unless asked for); ``status`` int32
    [S]: 0 for a refined segment, -1 for one that breaks the guard (an entry of vcol outside its segment, or a segment
    over the launch's bound) and of which nothing else was written, ``NOT_LAUNCHED`` for one outside the launch.  numpy
    arrays from ``refine``, tensors on the GPU from ``refine_device``."""

    def __init__(self, signature, colours, status, backend):
        self.signature, self.colours, self.status, self.last_backend = signature, colours, status, backend

    def cpu(self) -> "Refinement":
        host = lambda x: x.cpu().numpy() if isinstance(x, torch.Tensor) else x          # noqa: E731
        return Refinement(host(self.signature), host(self.colours), host(self.status), self.last_backend)


def _check(rounds, backend):
    if backend not in _BACKENDS:
        raise ValueError(f"unknown backend {backend!r}: one of {_BACKENDS}")
    if not 0 <= int(rounds) <= MAX_ROUNDS:
        raise ValueError(f"rounds = {rounds} is outside 0..{MAX_ROUNDS} (DESCO_WL_MAX_ROUNDS)")


def _host_arrays(b: Block, init):
    return (_np(b.vrowptr, np.int32), _np(b.vcol, np.int32), _np(b.seg_ptr, np.int32),
            None if init is None else _np(init, np.int64))


def _host_call(arrays, b: Block, group, rounds, num_threads, sig, colours, status, i0, i1):
    """the twin on segments [i0, i1): every array is indexed globally, so a range is a matter of where the per-segment
    pointers start"""
    vr, vc, sp, init = arrays
    g = np.asarray(group, dtype=np.int32)
    shift = lambda a, k: a.ctypes.data + k * a.itemsize                                 # noqa: E731
    _lib.check(_lib.lib().desco_wl_refine(
        vr.ctypes.data, vc.ctypes.data if vc.size else None, b.num_rows, b.slots, g.ctypes.data, shift(sp, i0), i1 - i0,
        b.anchor_base + i0 if b.anchor_base >= 0 else -1, None if init is None else init.ctypes.data, int(rounds),
        num_threads, shift(sig, i0), None if colours is None else colours.ctypes.data, shift(status, i0)),
        "desco_wl_refine")


def _host(b: Block, group, rounds, init, keep_colours, num_threads) -> Refinement:
    arrays = _host_arrays(b, init)
    S = len(arrays[2]) - 1
    sig, status = np.zeros(S, dtype=np.int64), np.full(S, NOT_LAUNCHED, dtype=np.int32)
    colours = np.zeros(b.num_rows, dtype=np.int64) if keep_colours else None
    _host_call(arrays, b, group, rounds, num_threads, sig, colours, status, 0, S)
    return Refinement(sig, colours, status, "host")


def segment_rows(b: Block):
    """rows of every segment, anchor included (what DEVICE_MAX_ROWS bounds); a tensor or an array like ``seg_ptr``"""
    sp = b.seg_ptr
    extra = 1 if b.anchor_base >= 0 else 0
    if isinstance(sp, torch.Tensor):
        sp = sp.to(torch.int64)
        return sp[1:] - sp[:-1] + extra
    sp = np.asarray(sp, dtype=np.int64)
    return np.diff(sp) + extra


def _launches(rows: torch.Tensor, ids, launch_bound=None) -> list:
    """[(seg_ids tensor or None = all, bound)]: the launches of one device call over the segments ``ids`` of a block
    whose segments have ``rows`` rows -- one launch when all of them fit one wave (or with ``launch_bound``), else one per
    row bucket, the larger segments of a bucket first."""
    if launch_bound is not None:
        return [(ids, int(launch_bound))]
    mine = rows if ids is None else rows[ids]
    mx = int(mine.max().item())
    if mx <= WAVE_ROWS:
        return [(ids, mx)]
    launches, lo = [], -1
    for hi in _BUCKETS + (mx,):
        if hi <= lo:
            continue
        pick = torch.nonzero((mine > lo) & (mine <= hi)).flatten()
        lo = hi
        if pick.numel() == 0:
            continue
        sub = mine[pick]
        if hi > WAVE_ROWS:
            order = torch.argsort(sub, descending=True, stable=True)
            pick, sub = pick[order], sub[order]
        launches.append(((pick if ids is None else ids[pick]).contiguous(), int(sub.max().item())))
    return launches


def _device(b: Block, group, rounds, init, keep_colours, dev, ids=None, launch_bound=None, fill: int = 0,
            out=None) -> Refinement:
    """The kernel on the segments ``ids`` (a tensor / array of int64, None = all), everything on ``dev``: one launch per
    row bucket -- or, with ``launch_bound``, one launch with that bound.  Entries of other segments hold ``fill``.
    ``out``: (sig, colours or None, status) tensors to write into."""
    L = _lib.lib()
    dev = torch.device(dev)
    vr, vc, sp = _dev(b.vrowptr, torch.int32, dev), _dev(b.vcol, torch.int32, dev), _dev(b.seg_ptr, torch.int32, dev)
    init_d = None if init is None else _dev(init, torch.int64, dev)
    S = sp.numel() - 1
    if out is None:
        sig = torch.full((S,), fill, dtype=torch.int64, device=dev)
        colours = torch.full((b.num_rows,), fill, dtype=torch.int64, device=dev) if keep_colours else None
        status = torch.full((S,), NOT_LAUNCHED, dtype=torch.int32, device=dev)
    else:
        sig, colours, status = out
    g = np.asarray(group, dtype=np.int32)
    ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None               # noqa: E731
    if ids is not None:
        ids = _dev(ids, torch.int64, dev)
    if S and (ids is None or ids.numel()):
        launches = _launches(segment_rows(b._replace(seg_ptr=sp)), ids, launch_bound)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            for seg_ids, bound in launches:
                _lib.check(L.desco_wl_refine_dev(
                    vr.data_ptr(), ptr(vc), b.num_rows, b.slots, g.ctypes.data, sp.data_ptr(), S, b.anchor_base,
                    ptr(init_d), int(rounds), ptr(seg_ids), 0 if seg_ids is None else seg_ids.numel(), bound, sig.data_ptr(),
                    ptr(colours), status.data_ptr(), stream.cuda_stream), "desco_wl_refine_dev")
            stream.synchronize()                        # the id lists and converted inputs are released when this returns
    return Refinement(sig, colours, status, "device")


def _limit(max_rows):
    if max_rows is None:
        return DEVICE_MAX_ROWS
    if max_rows < 0:
        raise ValueError("max_rows is negative")
    return min(int(max_rows), DEVICE_MAX_ROWS)


def refine_device(batch, view="shmp", rounds: int = 8, device="cuda", init=None, keep_colours: bool = False,
                  max_rows=None, seg_ids=None, fill: int = 0) -> Refinement:
    """``refine`` by the gfx950 kernel, the results kept on the GPU.  ``seg_ids``: only these segments are refined
    (default: all) and only their entries are written, the others hold ``fill``.  Every segment has to fit the kernel's
    bound (``max_rows`` lowers it); a larger one is refused by name -- ``refine(backend="auto")`` sends those to the host
    twin instead."""
    _check(rounds, "device")
    b = _block(batch)
    group = view_groups(view, b.slots)
    limit = _limit(max_rows)
    rows = segment_rows(b)
    if seg_ids is not None:
        ids = np.asarray(seg_ids.cpu() if isinstance(seg_ids, torch.Tensor) else seg_ids, dtype=np.int64)
        if len(ids) and (ids.min() < 0 or ids.max() >= len(rows)):
            raise ValueError("seg_ids outside the block's segments")
        rows = rows[torch.from_numpy(ids).to(rows.device) if isinstance(rows, torch.Tensor) else ids]
        seg_ids = ids
    if len(rows) and int(rows.max()) > limit and limit < DEVICE_MAX_ROWS:
        raise RuntimeError(f"refine_device: a segment of {int(rows.max())} rows, anchor included, exceeds the device bound "
                           f"DESCO_WL_DEV_MAX_ROWS ({DEVICE_MAX_ROWS}) as lowered by max_rows = {limit}; "
                           'backend="auto" refines it with desco_wl_refine')
    return _device(b, group, rounds, init, keep_colours, device, ids=seg_ids, fill=fill)


def _merged(b: Block, group, rounds, init, keep_colours, num_threads, limit) -> Refinement:
    """Device for the segments within ``limit`` rows, host twin for the others."""
    rows = segment_rows(b)
    fit = (rows <= limit)
    fit = fit.cpu().numpy() if isinstance(fit, torch.Tensor) else fit
    if fit.all():
        return _device(b, group, rounds, init, keep_colours, "cuda").cpu()
    d = _device(b, group, rounds, init, keep_colours, "cuda", ids=np.flatnonzero(fit).astype(np.int64)).cpu()
    arrays = _host_arrays(b, init)
    rest = np.flatnonzero(~fit)
    for run in np.split(rest, np.flatnonzero(np.diff(rest) != 1) + 1):          # one call of the twin per run of segments
        _host_call(arrays, b, group, rounds, num_threads, d.signature, d.colours, d.status, int(run[0]),
                   int(run[-1]) + 1)
    d.last_backend = "device+host"
    return d


def refine(batch, view="shmp", rounds: int = 8, backend: str = "auto", init=None, keep_colours: bool = False,
           max_rows=None, num_threads: int = 0) -> Refinement:
    """``rounds`` rounds of colour refinement of every segment of ``batch`` -- a ``NeighborhoodBatch`` (or a
    ``NeighborhoodPartition``): one segment per neighborhood, its canonical row the anchor; a ``GraphBatch``: one segment
    per graph, no anchor; or a ``Block`` of explicit arrays.  ``view``: one of ``VIEWS`` or an explicit ``group`` tuple.
    ``init`` int64 [R]: the rows' initial colours (default: 1 for an anchor row, 0 for any other).

    ``backend``: "host" (OpenMP twin), "device" (HIP kernel; every segment must fit ``DEVICE_MAX_ROWS``, or ``max_rows``
    when that is lower), or "auto": the device when there is one, segments above its bound going to the host twin and
    being merged (``last_backend`` then reads "device+host")."""
    global last_backend
    _check(rounds, backend)
    b = _block(batch)
    group = view_groups(view, b.slots)
    if backend == "host" or (backend == "auto" and not torch.cuda.is_available()):
        res = _host(b, group, rounds, init, keep_colours, num_threads)
    elif backend == "device":
        res = refine_device(b, group, rounds, "cuda", init, keep_colours, max_rows).cpu()
    else:
        res = _merged(b, group, rounds, init, keep_colours, num_threads, _limit(max_rows))
    last_backend = res.last_backend
    return res


# ---- colour classes of a data set ------------------------------------------------------------------------------------
class Classes:
    """``signature`` int64 [S]; ``class_id`` int64 [S]: the rank of the set's signature among the sorted distinct
    signatures (so host and device name the classes alike); ``num_classes``; ``class_size`` int64 [num_classes];
    ``neigh_index`` int64 [S, 2] = (graph, node in graph) of every neighborhood (None for whole graphs).  numpy arrays, or
    tensors on the GPU from the ``*_device`` variants (``cpu()`` brings them over)."""

    def __init__(self, signature, class_id, class_size, neigh_index, level, view, rounds, backend):
        self.signature, self.class_id, self.class_size, self.neigh_index = signature, class_id, class_size, neigh_index
        self.level, self.view, self.rounds, self.last_backend = level, view, rounds, backend

    @property
    def num_classes(self) -> int:
        return int(self.class_size.shape[0])

    @property
    def num_sets(self) -> int:
        return int(self.signature.shape[0])

    def cpu(self) -> "Classes":
        host = lambda x: x.cpu().numpy() if isinstance(x, torch.Tensor) else x          # noqa: E731
        return Classes(host(self.signature), host(self.class_id), host(self.class_size), host(self.neigh_index),
                       self.level, self.view, self.rounds, self.last_backend)


def classes_of(signature, neigh_index=None, level="neighborhood", view=None, rounds=None, backend=None) -> Classes:
    """The partition into equal-signature classes (``torch.unique`` on the card for a tensor, ``numpy.unique`` for an
    array: both rank the distinct int64 signatures in ascending order)."""
    if isinstance(signature, torch.Tensor):
        _, inv, size = torch.unique(signature, sorted=True, return_inverse=True, return_counts=True)
        return Classes(signature, inv.to(torch.int64), size.to(torch.int64), neigh_index, level, view, rounds, backend)
    _, inv, size = np.unique(signature, return_inverse=True, return_counts=True)
    return Classes(signature, inv.reshape(-1).astype(np.int64), size.astype(np.int64), neigh_index, level, view, rounds,
                   backend)


def _require_refined(res: Refinement, what: str):
    bad = res.status != 0
    if bool(bad.any()):
        raise RuntimeError(f"{what}: {int(bad.sum())} segments were not refined (status -1: an entry outside its segment)")


def neighborhood_classes_device(graphs: GraphSet, depth: int = 4, rounds: int = 8, view="shmp",
                                restricted: bool = False, device="cuda", part: NeighborhoodPartition = None) -> Classes:
    """``neighborhood_classes`` on the GPU, tensors in the result: the partition is built by the device builder (or is
    ``part``, already resident), refined by the kernel, and the signatures stay on the card until ``class_id`` is
    formed."""
    _check(rounds, "device")
    if part is None:
        part = build_partition_device(graphs, depth, device, restricted=restricted)
    res = refine_device(NeighborhoodBatch(part, device), view, rounds, device)
    _require_refined(res, "neighborhood_classes_device")
    return classes_of(res.signature, part.device_arrays["neigh_index"], "neighborhood", view, rounds, "device")


def neighborhood_classes(graphs: GraphSet, depth: int = 4, rounds: int = 8, view="shmp", restricted: bool = False,
                         backend: str = "auto", num_threads: int = 0) -> Classes:
    """The colour classes of the canonical neighborhoods of ``graphs`` (``restricted``: the homogeneous ablation's
    neighborhood definition) after ``rounds`` rounds under ``view``.  "auto": the device when there is one -- the
    partition built there; graphs above the device builder's workspace or neighborhoods above ``DEVICE_MAX_ROWS`` take
    the host builder / the host twin and are merged."""
    global last_backend
    _check(rounds, backend)
    view_groups(view, 4)
    if backend == "device" or (backend == "auto" and torch.cuda.is_available()):
        try:
            part = build_partition_device(graphs, depth, "cuda", restricted=restricted)
        except ValueError:
            if backend == "device":
                raise
            part = None
        if part is not None and (backend == "device" or int(segment_rows(_block(part)).max().item() if part.num_neigh
                                                            else 0) <= DEVICE_MAX_ROWS):
            out = neighborhood_classes_device(graphs, depth, rounds, view, restricted, "cuda", part).cpu()
            last_backend = out.last_backend
            return out
        if part is None:
            part = build_partition(graphs, depth, num_threads=num_threads, restricted=restricted)
        res = refine(part, view, rounds, "auto", num_threads=num_threads)
    else:
        part = build_partition(graphs, depth, num_threads=num_threads, restricted=restricted)
        res = refine(part, view, rounds, "host", num_threads=num_threads)
    _require_refined(res, "neighborhood_classes")
    last_backend = res.last_backend
    return classes_of(res.signature, np.asarray(part.neigh_index), "neighborhood", view, rounds, res.last_backend)


def graph_classes_device(graphs: GraphSet, rounds: int = 8, view="shmp", device="cuda") -> Classes:
    """``graph_classes`` on the GPU, tensors in the result (the typed CSR is built there from the set's device CSR)."""
    _check(rounds, "device")
    view_groups(view, 2)
    res = refine_device(GraphBatch(graphs, device), view, rounds, device)
    _require_refined(res, "graph_classes_device")
    return classes_of(res.signature, None, "graph", view, rounds, "device")


def graph_classes(graphs: GraphSet, rounds: int = 8, view="shmp", backend: str = "auto",
                  num_threads: int = 0) -> Classes:
    """The colour classes of the whole graphs of ``graphs`` (the model without canonical partition: 2 relation slots, no
    anchor) after ``rounds`` rounds under ``view`` ("shmp" or "plain")."""
    global last_backend
    _check(rounds, backend)
    view_groups(view, 2)
    on_device = backend == "device" or (backend == "auto" and torch.cuda.is_available())
    res = refine(GraphBatch(graphs, "cuda" if on_device else "cpu"), view, rounds, backend, num_threads=num_threads)
    _require_refined(res, "graph_classes")
    last_backend = res.last_backend
    return classes_of(res.signature, None, "graph", view, rounds, res.last_backend)


# ---- what the classes cost: the error floor --------------------------------------------------------------------------
class ErrorFloor:
    """Per query (arrays of length Q): ``ambiguous_classes`` int64, the classes whose members do not all share one
    count; ``ambiguous_sets`` int64, the members of those classes; ``sse_floor``, ``mse_floor``, ``norm_mse_floor``
    float64.  ``num_sets``, ``num_classes``, ``space``."""

    def __init__(self, classes: Classes, space, ambiguous_classes, ambiguous_sets, sse, mse, norm_mse):
        self.num_sets, self.num_classes, self.space = classes.num_sets, classes.num_classes, space
        self.level, self.view, self.rounds = classes.level, classes.view, classes.rounds
        self.ambiguous_classes, self.ambiguous_sets = ambiguous_classes, ambiguous_sets
        self.sse_floor, self.mse_floor, self.norm_mse_floor = sse, mse, norm_mse

    def table(self, names=None) -> list:
        """One dict per query: the rows the driver writes."""
        Q = len(self.ambiguous_sets)
        names = list(range(Q)) if names is None else list(names)
        return [{"query": names[q], "ambiguous_sets": int(self.ambiguous_sets[q]),
                 "ambiguous_classes": int(self.ambiguous_classes[q]), "sse_floor": float(self.sse_floor[q]),
                 "mse_floor": float(self.mse_floor[q]), "norm_mse_floor": float(self.norm_mse_floor[q])}
                for q in range(Q)]


def error_floor(classes: Classes, truth, space: str = "log2") -> ErrorFloor:
    """The error that ``classes`` force on ANY model that cannot tell the members of a class apart: it predicts one
    value per class, and the best one is the class mean.  ``truth`` int64 [S, Q]: for neighborhoods the canonical
    counts at ``neigh_index``, for graphs the per-graph sums.  ``space``: "log2" -- y = log2(1 + count), the target of
    the neighborhood loss -- or "count".  ``sse_floor`` is the within-class sum of squares of y, ``mse_floor`` that over
    S, and ``norm_mse_floor`` that over Var(y) (``analysis.norm_mse``'s normalisation; nan where y is constant).

    The integer fields are exact.  The float fields are one numpy float64 code path on host arrays whatever backend made
    the classes; a class that is not ambiguous contributes exactly 0.  A floor is a lower bound for that depth and
    family, not a prediction."""
    if space not in ("log2", "count"):
        raise ValueError(f"unknown space {space!r}: 'log2' or 'count'")
    c = classes.cpu()
    cid = np.asarray(c.class_id, dtype=np.int64)
    truth = truth.cpu().numpy() if isinstance(truth, torch.Tensor) else np.asarray(truth)
    if truth.ndim != 2 or truth.shape[0] != len(cid):
        raise ValueError(f"truth must be [{len(cid)}, Q], got {truth.shape}")
    if not np.issubdtype(truth.dtype, np.integer):
        if not np.array_equal(truth, np.rint(truth)):
            raise ValueError("truth holds values that are no integers")
    truth = truth.astype(np.int64)
    S, Q = truth.shape
    C = c.num_classes
    size = np.asarray(c.class_size, dtype=np.int64)
    amb_c, amb_s = np.zeros(Q, dtype=np.int64), np.zeros(Q, dtype=np.int64)
    sse = np.zeros(Q, dtype=np.float64)
    mse, nmse = np.zeros(Q, dtype=np.float64), np.zeros(Q, dtype=np.float64)
    for q in range(Q):
        t = truth[:, q]
        lo = np.full(C, np.iinfo(np.int64).max, dtype=np.int64)
        hi = np.full(C, np.iinfo(np.int64).min, dtype=np.int64)
        np.minimum.at(lo, cid, t)
        np.maximum.at(hi, cid, t)
        amb = lo != hi
        amb_c[q], amb_s[q] = int(amb.sum()), int(size[amb].sum())
        y = np.log2(1.0 + t.astype(np.float64)) if space == "log2" else t.astype(np.float64)
        mean = np.bincount(cid, weights=y, minlength=C) / np.maximum(size, 1)
        res = np.where(amb[cid], y - mean[cid], 0.0)
        sse[q] = float(np.sum(res * res))
        mse[q] = sse[q] / S if S else 0.0
        var = float(np.var(y)) if S else 0.0
        nmse[q] = mse[q] / var if var > 0 else (0.0 if sse[q] == 0 else np.nan)
    return ErrorFloor(c, space, amb_c, amb_s, sse, mse, nmse)


def neighborhood_truth(graphs: GraphSet, classes: Classes, queries, backend: str = "auto") -> np.ndarray:
    """int64 [S, Q]: the exact canonical counts of ``queries`` at every neighborhood's canonical node."""
    from . import groundtruth
    counts = groundtruth.canonical_counts(graphs, queries, backend=backend).numpy()
    ni = np.asarray(classes.cpu().neigh_index, dtype=np.int64)
    return np.rint(counts[graphs.graph_ptr[ni[:, 0]] + ni[:, 1]]).astype(np.int64)


def graph_truth(graphs: GraphSet, queries, backend: str = "auto") -> np.ndarray:
    """int64 [G, Q]: the exact canonical counts of ``queries`` summed over every graph's nodes."""
    from . import groundtruth
    counts = np.rint(groundtruth.canonical_counts(graphs, queries, backend=backend).numpy()).astype(np.int64)
    out = np.zeros((graphs.num_graphs, counts.shape[1]), dtype=np.int64)
    np.add.at(out, graphs.node_graph_ids(), counts)
    return out
