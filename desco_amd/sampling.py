"""Sampled subgraph counts: RAND-ESU (Wernicke, "Efficient detection of network motifs", 2006) estimates with error bars.

Every other counter of this package is exact.  This one walks the enumeration tree of the exact census and keeps every
tree edge with a probability that depends only on its depth; a dropped edge takes its whole subtree along.  The kept
subsets are tallied per class, and a tally divided by the product of the probabilities along the path is an unbiased
estimate of the exact count.  ``replicas`` independent walks give the mean and its standard error.

The host twin (csrc/sampled_counts.cpp) and the gfx950 kernel (csrc/sampled_counts_dev.hip) agree bit for bit, because
every keep / drop decision is a function of (seed, replica, graph, the sequence of chosen nodes) alone
(include/desco_hip.h, "SAMPLED COUNTS").  Unlabelled graphs, canonical counts only; 2..5 nodes on the device, 6 on the
host.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from . import _lib
from . import groundtruth as gt
from .graphs import GraphSet

# who served the last sampled_tallies / estimate_counts call: "host", "device", or "device+host" when graphs above the
# device's bitset limit went to the host twin and were merged
last_backend = None

_BACKENDS = ("auto", "host", "device")
_ONE = 1 << 32
DEFAULT_MAX_BYTES = 1 << 30         # tallies one launch writes: replicas go in chunks of what this holds

# What "auto" does with a GPU present, from tools/bench_sampled_counts.py: the device only where it
# beat the 16-thread twin on both benchmark shapes.
AUTO_USES_DEVICE = True


def schedule(kmax: int, fraction: float = None, probs: Sequence[float] = None):
    """The thresholds of a sampling schedule for subsets of up to ``kmax`` (2..6) nodes: ``(thr, probs, weights)``.

    Exactly one of ``probs`` -- the kmax - 1 probabilities of the levels 2..kmax (level d decides node number d of a
    subset) -- and ``fraction`` -- the uniform schedule p_d = fraction ** (1 / (kmax - 1)), under which a kmax-subset
    survives with probability ``fraction``.  Probabilities lie in [0, 1]; they are quantised to integer thresholds
    ``thr[d] = floor(p_d * 2^32)``, 1 becoming 2^32 exactly (always kept) and 0 never.
    Returns ``thr`` int64 [kmax + 1] (entries 0 and 1 unused), the EFFECTIVE probabilities thr[2:] / 2^32 as float64
    [kmax - 1], and ``weights`` float64 [kmax + 1]: weights[j] = prod_{d=2..j} 2^32 / thr[d], what a tally of j-node
    subsets is multiplied with (inf where a level at or above j has probability 0; weights[0] = weights[1] = 1)."""
    if not 2 <= int(kmax) <= 6:
        raise ValueError("schedule: kmax must be 2..6")
    if (fraction is None) == (probs is None):
        raise ValueError("schedule: give exactly one of fraction and probs")
    kmax = int(kmax)
    if probs is None:
        f = float(fraction)
        if not 0.0 <= f <= 1.0:
            raise ValueError("schedule: fraction must lie in [0, 1]")
        p = [f ** (1.0 / (kmax - 1))] * (kmax - 1)
    else:
        p = [float(x) for x in probs]
        if len(p) != kmax - 1:
            raise ValueError(f"schedule: probs must hold the {kmax - 1} probabilities of the levels 2..{kmax}")
        if any(not 0.0 <= x <= 1.0 for x in p):
            raise ValueError("schedule: probabilities must lie in [0, 1]")
    thr = np.zeros(kmax + 1, dtype=np.int64)
    for d, x in enumerate(p, start=2):
        thr[d] = _ONE if x >= 1.0 else int(x * float(_ONE))
    return thr, thr[2:].astype(np.float64) / float(_ONE), _weights(thr)


def _weights(thr: np.ndarray) -> np.ndarray:
    w = np.ones(len(thr), dtype=np.float64)
    with np.errstate(divide="ignore"):
        for d in range(2, len(thr)):
            w[d] = w[d - 1] * (float(_ONE) / float(thr[d]) if thr[d] else np.inf)
    return w


def _queries(queries):
    """[(k, edge tuple)], checked: connected, loop-free, 2..6 nodes.  None: the 30 connected graphs of 2..5 nodes."""
    if queries is None:
        return [(k, tuple(e)) for k in (2, 3, 4, 5) for _, e in gt.census_classes(k)]
    flat = gt._flatten_queries(queries)[0]
    if any(n < 2 or n > 6 for n, _ in flat):
        raise RuntimeError("sampled counts take queries of 2..6 nodes (2..5 nodes on the device)")
    if flat:
        gt.match_plan(flat)                 # refuses disconnected queries and loops, naming the reason
    return [(n, tuple((int(a), int(b)) for a, b in e)) for n, e in flat]


def _plan(flat):
    """Every query is computed as its census class, so duplicates and isomorphic queries get equal columns.  Returns
    (classes, sizes, index): the census classes of every size in use (census order, size by size), the size of every
    class column, and the class column of every query."""
    classes, start = [], {}
    for k in sorted({n for n, _ in flat}):
        start[k] = len(classes)
        classes += [(n, list(e)) for n, e in gt.census_classes(k)]
    index = np.array([start[k] + gt._census_class_of_mask(k)[gt._orbit_structure(k, tuple(e))[2]] for k, e in flat],
                     dtype=np.int64)
    return classes, np.array([n for n, _ in classes], dtype=np.int64), index


def _resolve(flat, fraction, probs):
    """(kmax, thr, probs, weights) of a call: kmax is the largest query; of ``probs`` the first kmax - 1 are used (the
    decisions of a level do not depend on the deeper ones, so the columns are those of the longer schedule)."""
    kmax = max((n for n, _ in flat), default=2)
    if probs is not None and fraction is None:
        probs = list(probs)
        if len(probs) < kmax - 1:
            raise ValueError(f"probs must hold the probabilities of the levels 2..{kmax}")
        probs = probs[:kmax - 1]
    return (kmax,) + schedule(kmax, fraction, probs)


def _check(replicas, backend, level, graph_base, replica_base):
    if backend not in _BACKENDS:
        raise ValueError(f"unknown backend {backend!r}: one of {_BACKENDS}")
    if level not in ("graph", "node"):
        raise ValueError(f"unknown level {level!r}: 'graph' or 'node'")
    if replicas < 0 or graph_base < 0 or replica_base < 0:
        raise ValueError("replicas, graph_base and replica_base must not be negative")


def _tallies_host(graphs: GraphSet, classes, kmax, thr, replicas, seed, graph_base, replica_base, num_threads,
                  level) -> np.ndarray:
    """desco_sampled_counts on the census classes: int64 [R, G or N, C] (the twin sums a graph's rows itself)."""
    _, q_nodes, q_edge_ptr, q_edges = gt._flatten_queries(classes)
    G, C = graphs.num_graphs, len(classes)
    out = np.zeros((replicas, G if level == "graph" else graphs.num_nodes, C), dtype=np.int64)
    if out.size:
        _lib.check(_lib.lib().desco_sampled_counts(
            graphs.graph_ptr.ctypes.data, G, graphs.rowptr.ctypes.data, graphs.col.ctypes.data,
            q_nodes.ctypes.data, q_edge_ptr.ctypes.data, q_edges.ctypes.data, C, kmax, thr.ctypes.data,
            seed & (2 ** 64 - 1), graph_base, replica_base, replicas, int(level == "graph"), num_threads,
            out.ctypes.data), "desco_sampled_counts")
    return out


def _tallies_device(graphs: GraphSet, classes, kmax, thr, replicas, seed, graph_base, replica_base, level, max_bytes,
                    dev) -> torch.Tensor:
    """desco_sampled_counts_dev on the census classes: int64 [R, G or N, C] on ``dev``.  For level "graph" the kernel
    adds a wave's tallies straight into its graph's row (integer atomics: exact in any order), so [R, N, C] never
    exists.  Replicas go in chunks of what ``max_bytes`` of tallies hold, written into the one result."""
    N, G, C = graphs.num_nodes, graphs.num_graphs, len(classes)
    rows = G if level == "graph" else N
    out = torch.empty((replicas, rows, C), dtype=torch.int64, device=dev)
    if replicas == 0 or N == 0 or C == 0:
        return out.zero_()
    table, table_kmax, _ = gt._class_table(classes)
    assert table_kmax == kmax
    d = gt._DeviceGraphs(graphs, dev)
    cls = d.put(table, np.int16)
    chunk = int(max(1, min(replicas, max_bytes // (8 * rows * C))))
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        for r0 in range(0, replicas, chunk):
            rc = min(chunk, replicas - r0)
            _lib.check(_lib.lib().desco_sampled_counts_dev(
                *d.head, cls.data_ptr(), kmax, C, thr.ctypes.data, seed & (2 ** 64 - 1), graph_base,
                replica_base + r0, rc, int(level == "graph"), out[r0:r0 + rc].data_ptr(), stream),
                "desco_sampled_counts_dev")
        torch.cuda.current_stream(dev).synchronize()            # the graph and the table are released when this returns
    return out


def _device_runs(graphs: GraphSet):
    """Splits the set for the device's bitset workspace (``groundtruth._DEVICE_BITSET_LIMIT_WORDS``): a list of
    (g0, g1, fits) -- runs of consecutive graphs whose bitset rows fit together, and single graphs that do not fit."""
    limit = gt._DEVICE_BITSET_LIMIT_WORDS
    words = gt._bitset_words(graphs)
    runs, g0, acc = [], 0, 0
    for g, w in enumerate(words):
        if w > limit:
            if g > g0:
                runs.append((g0, g, True))
            runs.append((g, g + 1, False))
            g0, acc = g + 1, 0
        elif acc + w > limit:
            runs.append((g0, g, True))
            g0, acc = g, int(w)
        else:
            acc += int(w)
    if len(words) > g0:
        runs.append((g0, len(words), True))
    return runs


def _run(graphs, flat, fraction, probs, replicas, seed, backend, level, graph_base, replica_base, num_threads,
         max_bytes, dev, keep_on_device):
    """The class tallies of a call, [R, G or N, C] (a tensor on ``dev`` if ``keep_on_device``, else numpy), with the
    plan and the schedule: (tallies, classes, sizes, index, thr, probs, weights)."""
    global last_backend
    classes, sizes, index = _plan(flat)
    kmax, thr, p, w = _resolve(flat, fraction, probs)
    N, G, C = graphs.num_nodes, graphs.num_graphs, len(classes)
    rows = G if level == "graph" else N
    if backend == "device" and kmax > 5:
        raise RuntimeError("sampled counts on the device take queries of 2..5 nodes (6 nodes: backend='host')")
    if backend == "auto":
        backend = "device" if AUTO_USES_DEVICE and kmax <= 5 and flat and torch.cuda.is_available() else "host"
        merge = True
    else:
        merge = False
    args = (classes, kmax, thr, replicas, seed)
    if backend == "host":
        t = _tallies_host(graphs, *args, graph_base, replica_base, num_threads, level)
        last_backend = "host"
        t = torch.from_numpy(t).to(dev) if keep_on_device else t
    else:
        runs = _device_runs(graphs) if merge else [(0, G, True)]
        if len(runs) <= 1 and all(fits for _, _, fits in runs):
            t = _tallies_device(graphs, *args, graph_base, replica_base, level, max_bytes, dev)
            last_backend = "device"
        else:
            parts = []
            for g0, g1, fits in runs:
                sub = graphs.subset(g0, g1)
                if fits:
                    parts.append(_tallies_device(sub, *args, graph_base + g0, replica_base, level, max_bytes, dev))
                else:
                    parts.append(torch.from_numpy(_tallies_host(sub, *args, graph_base + g0, replica_base, num_threads,
                                                                level)).to(dev))
            t = torch.cat(parts, dim=1) if parts else torch.zeros((replicas, rows, C), dtype=torch.int64, device=dev)
            last_backend = "device+host" if any(not fits for _, _, fits in runs) else "device"
        t = t if keep_on_device else t.cpu().numpy()
    return t, classes, sizes, index, thr, p, w


def sampled_tallies(graphs: GraphSet, queries: Sequence = None, *, probs: Sequence[float] = None,
                    fraction: float = None, replicas: int = 16, seed: int = 0, backend: str = "auto",
                    level: str = "graph", graph_base: int = 0, replica_base: int = 0, num_threads: int = 0,
                    max_bytes: int = DEFAULT_MAX_BYTES) -> torch.Tensor:
    """The integer tallies of ``replicas`` sampled walks: int64 [R, G, Q] on the CPU -- per replica and graph, the kept
    subsets whose induced subgraph is of the query's class -- or, for ``level="node"``, [R, N, Q]: the kept subsets by
    their largest node (the canonical counts' convention).

    ``queries``: networkx graphs or (n, edges) pairs, connected, 2..6 nodes, duplicates and isomorphic ones allowed;
    None = ``census_classes(2..5)``, 30 columns.  ``probs`` / ``fraction``: the schedule (``schedule``), for the levels
    2..kmax where kmax is the largest query.  The result is a function of (seed, ``replica_base`` + replica,
    ``graph_base`` + graph, the graph) alone: not of the backend, the thread count, the chunking, or which other graphs
    and replicas the call holds.  Multiply by ``schedule(...)[2][size of the query]`` for the unbiased estimate, or
    call ``estimate_counts``.

    ``backend``: "host" (the OpenMP twin), "device" (the HIP kernel; refuses 6-node queries), or "auto": the device
    when ``AUTO_USES_DEVICE`` holds, a GPU is present and no query has 6 nodes -- graphs whose adjacency bitsets exceed
    the device's limit then go to the twin and are merged (``last_backend`` reads "device+host") -- else the twin.
    ``max_bytes``: the tallies one device launch writes; replicas go in chunks of that."""
    _check(replicas, backend, level, graph_base, replica_base)
    flat = _queries(queries)
    t, _, _, index, _, _, _ = _run(graphs, flat, fraction, probs, replicas, seed, backend, level, graph_base,
                                   replica_base, num_threads, max_bytes, torch.device("cuda"), False)
    return torch.from_numpy(np.ascontiguousarray(t[:, :, index]))


def sampled_tallies_device(graphs: GraphSet, queries: Sequence = None, *, probs: Sequence[float] = None,
                           fraction: float = None, replicas: int = 16, seed: int = 0, level: str = "graph",
                           graph_base: int = 0, replica_base: int = 0, max_bytes: int = DEFAULT_MAX_BYTES,
                           device="cuda") -> torch.Tensor:
    """``sampled_tallies`` by the gfx950 kernel, the result kept on the GPU: int64 [R, G or N, Q] on ``device``.
    Queries of 2..5 nodes; the whole set has to fit the device's bitset workspace."""
    _check(replicas, "device", level, graph_base, replica_base)
    flat = _queries(queries)
    dev = torch.device(device)
    t, _, _, index, _, _, _ = _run(graphs, flat, fraction, probs, replicas, seed, "device", level, graph_base,
                                   replica_base, 0, max_bytes, dev, True)
    return t.index_select(2, torch.from_numpy(index).to(dev))


class SampledCounts:
    """Estimates of Q queries in G graphs (or at N nodes) from R sampled walks: ``estimate`` and ``stderr`` float64
    [G or N, Q] -- the mean over the replicas of tally x weight and its standard error, std(ddof = 1) / sqrt(R) (NaN
    for R = 1); ``tallies`` int64 [R, G or N, Q] for induced counts, or for non-induced ones the class tallies
    [R, G or N, C] the estimate was transformed from; ``probs`` the effective level probabilities, ``weights`` the
    weight of every subset size, ``columns`` the queries as (n, edges), ``last_backend`` who computed it.  A column
    whose schedule has a zero at or above its size has no estimate: NaN."""

    def __init__(self, columns, estimate, stderr, tallies, probs, weights, last_backend):
        self.columns, self.estimate, self.stderr, self.tallies = list(columns), estimate, stderr, tallies
        self.probs, self.weights, self.last_backend = probs, weights, last_backend
        self.replicas = int(tallies.shape[0])

    def table(self) -> dict:
        """One row per (graph or node, query), row-major: columns graph, query, estimate, stderr."""
        G, Q = self.estimate.shape
        return {"graph": np.repeat(np.arange(G), Q), "query": np.tile(np.arange(Q), G),
                "estimate": self.estimate.ravel(), "stderr": self.stderr.ravel()}


def estimate_counts(graphs: GraphSet, queries: Sequence = None, *, fraction: float = None,
                    probs: Sequence[float] = None, replicas: int = 16, seed: int = 0, backend: str = "auto",
                    induced: bool = True, level: str = "graph", num_threads: int = 0,
                    max_bytes: int = DEFAULT_MAX_BYTES) -> SampledCounts:
    """Unbiased estimates of the canonical counts of ``queries`` with their standard errors (``SampledCounts``).

    The schedule is ``probs`` or ``fraction`` (default: fraction 0.01); the other arguments are ``sampled_tallies``'.
    ``induced=False``: the NON-INDUCED counts (``canonical_counts(induced=False)``).  The whole census of every size in
    use is estimated and the float64 estimates are multiplied, replica by replica, with ``noninduced_matrix(k)``; the
    transform is linear, so the result stays unbiased, and ``stderr`` is taken over the transformed replicas."""
    if fraction is None and probs is None:
        fraction = 0.01
    _check(replicas, backend, level, 0, 0)
    flat = _queries(queries)
    t, classes, sizes, index, thr, p, w = _run(graphs, flat, fraction, probs, replicas, seed, backend, level, 0, 0,
                                               num_threads, max_bytes, torch.device("cuda"), False)
    with np.errstate(invalid="ignore"):
        per_replica = t.astype(np.float64) * w[sizes]               # [R, rows, C]; 0 * inf = NaN: no estimate
        if induced:
            per_replica, tallies = per_replica[:, :, index], np.ascontiguousarray(t[:, :, index])
        else:
            M = np.zeros((len(classes), len(flat)), dtype=np.float64)
            start = {k: int(np.flatnonzero(sizes == k)[0]) for k in sorted(set(sizes.tolist()))}
            for q, (k, e) in enumerate(flat):
                M[start[k]:start[k] + len(gt.census_classes(k)), q] = gt._noninduced_rows([(k, list(e))])[0]
            per_replica, tallies = per_replica @ M, t
        R = per_replica.shape[0]
        estimate = per_replica.mean(axis=0) if R else np.full(per_replica.shape[1:], np.nan)
        stderr = per_replica.std(axis=0, ddof=1) / np.sqrt(R) if R > 1 else np.full(per_replica.shape[1:], np.nan)
    return SampledCounts(flat, estimate, stderr, tallies, p, w, last_backend)
