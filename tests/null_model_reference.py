"""The degree-preserving null model's chain in plain Python: the yardstick of the host twin (and, through it, of the
kernel).  Philox from oracle.dropout, sets for the adjacency, strictly one attempt at a time (include/desco_hip.h,
"NULL MODEL")."""
import numpy as np

from oracle.dropout import philox4x32_10

MASK32 = 0xFFFFFFFF


def draws(seed: int, graph: int, replica: int, t, m: int):
    """(i, j, flip), int64 arrays, of the attempts ``t`` (array of Python ints or uint64) of chain (graph, replica)
    over m slots.  Only the generator is evaluated for many attempts at once; the chain below takes them one by one."""
    t = np.asarray(t, dtype=np.uint64)
    w = philox4x32_10((t & np.uint64(MASK32), t >> np.uint64(32), np.uint64(graph & MASK32),
                       np.uint64(replica & MASK32)), (seed & MASK32, (seed >> 32) & MASK32))
    w0, w1, w2 = (x.astype(np.uint64) for x in w[:3])
    return ((w0 * np.uint64(m)) >> np.uint64(32)).astype(np.int64), \
        ((w1 * np.uint64(m)) >> np.uint64(32)).astype(np.int64), (w2 & np.uint64(1)).astype(np.int64)


def draw(seed: int, graph: int, replica: int, t: int, m: int):
    """(i, j, flip) of attempt t of chain (graph, replica) over m slots"""
    i, j, flip = draws(seed, graph, replica, [t], m)
    return int(i[0]), int(j[0]), int(flip[0])


def rewire_graph(n: int, rows, seed: int, graph: int, replica: int, swaps_per_edge: int):
    """One chain.  ``rows``: the ascending neighbour lists (local ids) of the n nodes.  Returns (new rows, accepted)."""
    slots = [(u, v) for v in range(n) for u in rows[v] if u < v]            # CSR order of the entries (v, u), u < v
    m = len(slots)
    if m < 2:
        return [list(r) for r in rows], 0
    edges = {frozenset(s) for s in slots}
    accepted = 0
    di, dj, dflip = draws(seed, graph, replica, np.arange(swaps_per_edge * m, dtype=np.uint64), m)
    for t in range(swaps_per_edge * m):
        i, j, flip = int(di[t]), int(dj[t]), int(dflip[t])
        if i == j:
            continue
        (a, b), (c, d) = slots[i], slots[j]
        if flip:
            c, d = d, c
        if a == d or c == b or frozenset((a, d)) in edges or frozenset((c, b)) in edges:
            continue
        edges -= {frozenset((a, b)), frozenset((c, d))}
        edges |= {frozenset((a, d)), frozenset((c, b))}
        slots[i], slots[j] = (a, d), (c, b)
        accepted += 1
    new = [[] for _ in range(n)]
    for e in edges:
        x, y = tuple(e)
        new[x].append(y)
        new[y].append(x)
    return [sorted(r) for r in new], accepted


def rewire(graphs, replicas: int, swaps_per_edge: int, seed: int, graph_base: int = 0, replica_base: int = 0):
    """(col int32 [replicas, E], accepted int32 [replicas, G]) of a GraphSet, as desco_null_model_rewire defines them."""
    G, E = graphs.num_graphs, graphs.num_directed_edges
    col = np.zeros((replicas, E), dtype=np.int32)
    accepted = np.zeros((replicas, G), dtype=np.int32)
    for g in range(G):
        n0, n1 = int(graphs.graph_ptr[g]), int(graphs.graph_ptr[g + 1])
        rows = [[int(u) - n0 for u in graphs.col[graphs.rowptr[v]:graphs.rowptr[v + 1]]] for v in range(n0, n1)]
        for r in range(replicas):
            new, accepted[r, g] = rewire_graph(n1 - n0, rows, seed, graph_base + g, replica_base + r, swaps_per_edge)
            flat = [u + n0 for row in new for u in row]
            col[r, graphs.rowptr[n0]:graphs.rowptr[n1]] = flat
    return col, accepted


# ---- the graphs both test files run: small enough for the Python chain, chosen for what can go wrong -------------------
def _gnm(n, m, seed):
    rng = np.random.default_rng(seed)
    have = set()
    while len(have) < m:
        a, b = (int(x) for x in rng.integers(0, n, 2))
        if a != b:
            have.add((min(a, b), max(a, b)))
    return n, sorted(have)


def _hub(n, extra, seed):
    """node 0 joined to every other node, a path through the others, and ``extra`` random chords"""
    rng = np.random.default_rng(seed)
    have = {(0, v) for v in range(1, n)} | {(v, v + 1) for v in range(1, n - 1)}
    while len(have) < 2 * n - 3 + extra:
        a, b = (int(x) for x in rng.integers(1, n, 2))
        if a != b:
            have.add((min(a, b), max(a, b)))
    return n, sorted(have)


def ladder():
    """name -> GraphSet.  ``fixed``: graphs no switch can change (accepted must be 0)."""
    from desco_amd.graphs import GraphSet
    from desco_amd.groundtruth import census_classes
    return {
        "edges0123": GraphSet.from_edge_lists([(3, []), (2, [(0, 1)]), (4, [(0, 1), (2, 3)]),
                                               (5, [(0, 1), (1, 2), (3, 4)]), (4, [(0, 1), (1, 2), (2, 3)])]),
        "fixed": GraphSet.from_edge_lists([(3, [(0, 1), (1, 2), (0, 2)]),
                                           (4, [(a, b) for a in range(4) for b in range(a + 1, 4)]),
                                           (4, [(0, 1), (0, 2), (0, 3)])]),
        "small": GraphSet.from_edge_lists([(4, [(0, 1), (1, 2), (2, 3)]), (6, [(i, (i + 1) % 6) for i in range(6)]),
                                           (5, [(0, 1), (1, 2), (0, 2), (2, 3), (3, 4), (2, 4)])]),
        "classes": GraphSet.from_edge_lists([(k, list(e)) for k in (2, 3, 4, 5) for _, e in census_classes(k)]),
        "gnm40": GraphSet.from_edge_lists([_gnm(40, 100, 7)]),
        "hub": GraphSet.from_edge_lists([_hub(48, 30, 11), _hub(70, 10, 12)]),
    }
