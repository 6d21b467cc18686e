"""Plain-Python k-core and k-truss peels, written for the decomposition tests and nothing else, and the named graph
families the tests run on: the smallest shapes at which a peel can go wrong."""
import numpy as np

from desco_amd.graphs import GraphSet


def core_numbers(n, edges):
    """Core number of every node of one graph: repeatedly remove the nodes of degree <= k, then raise k."""
    adj = [set() for _ in range(n)]
    for a, b in edges:
        adj[a].add(b), adj[b].add(a)
    core, live, k = [0] * n, set(range(n)), 0
    while live:
        low = [v for v in live if len(adj[v]) <= k]
        if not low:
            k += 1
            continue
        for v in low:
            core[v] = k
            live.discard(v)
            for u in adj[v]:
                adj[u].discard(v)
            adj[v] = set()
    return core


def truss_numbers(n, edges):
    """{(a, b), a < b: (support, truss number)} of one graph: repeatedly remove the edges of support <= k - 2 while
    decrementing the two other edges of each destroyed triangle, then raise k."""
    adj = [set() for _ in range(n)]
    for a, b in edges:
        adj[a].add(b), adj[b].add(a)
    key = lambda a, b: (min(a, b), max(a, b))                                            # noqa: E731
    sup = {key(a, b): len(adj[a] & adj[b]) for a, b in edges}
    support, truss, k = dict(sup), {}, 2
    while sup:
        low = [e for e, s in sup.items() if s <= k - 2]
        if not low:
            k += 1
            continue
        for a, b in low:
            if (a, b) not in sup:
                continue
            for w in adj[a] & adj[b]:
                sup[key(a, w)] -= 1
                sup[key(b, w)] -= 1
            adj[a].discard(b), adj[b].discard(a)
            del sup[(a, b)]
            truss[(a, b)] = k
    return {e: (support[e], truss[e]) for e in support}


def decompose(graphs: GraphSet):
    """(core int32 [N], truss int32 [M], support int32 [M]) of a graph set, rows as groundtruth.edge_orbit_rows."""
    core, truss, support = [], [], []
    for g, (n, edges) in enumerate(graphs.edge_lists()):
        core += core_numbers(n, edges)
        st = truss_numbers(n, edges)
        for b, a in sorted((b, a) for a, b in st):                # the CSR entries (v, u), u < v, in CSR order
            support.append(st[(a, b)][0]), truss.append(st[(a, b)][1])
    return np.array(core, np.int32), np.array(truss, np.int32), np.array(support, np.int32)


# ---- the named families ------------------------------------------------------------------------------------------------
def clique(k, base=0):
    return [(base + a, base + b) for a in range(k) for b in range(a + 1, k)]


def gnp(n, p, seed):
    rng = np.random.default_rng(seed)
    return n, [(a, b) for a in range(n) for b in range(a + 1, n) if rng.random() < p]


def family_graphs():
    """[(name, n, edges)]"""
    out = [(f"K{k}", k, clique(k)) for k in range(2, 7)]
    out.append(("K5 minus an edge", 5, clique(5)[1:]))
    out.append(("path 7", 7, [(i, i + 1) for i in range(6)]))
    out.append(("cycle 7", 7, [(i, (i + 1) % 7) for i in range(7)]))
    out.append(("empty 5", 5, []))
    out.append(("single node", 1, []))
    out.append(("isolated nodes between components", 9, clique(3, 1) + [(5, 6), (6, 7)]))
    out.append(("two K4 sharing an edge", 6, sorted(set(clique(4) + [(0, 1), (0, 4), (0, 5), (1, 4), (1, 5), (4, 5)]))))
    out.append(("two K5 sharing a triangle", 7,
                sorted(set(clique(5) + [tuple(sorted((a, b))) for a in (0, 1, 2, 5, 6) for b in (0, 1, 2, 5, 6) if a < b]))))
    out.append(("K3,3 plus an edge", 6, [(a, b) for a in range(3) for b in range(3, 6)] + [(0, 1)]))
    out.append(("triangle strip 40", 42, [(i, i + 1) for i in range(41)] + [(i, i + 2) for i in range(40)]))
    out.append(("wheel W7", 8, [(0, v) for v in range(1, 8)] + [(v, v % 7 + 1) for v in range(1, 8)]))
    out.append(("windmill 150", 301, [e for t in range(150) for e in ((0, 2 * t + 1), (0, 2 * t + 2),
                                                                     (2 * t + 1, 2 * t + 2))]))
    out.append(("star 300", 301, [(0, v) for v in range(1, 301)]))
    out.append(("G(120, 0.5)",) + gnp(120, 0.5, 7))
    return out


def families() -> GraphSet:
    return GraphSet.from_edge_lists([(n, e) for _, n, e in family_graphs()])


def dense_random() -> GraphSet:
    """The three dense random graphs of test_groundtruth_dev_gpu.py's "dense" case (same generator, same draws: the last
    node of each stays isolated), without its single-node and two-node graphs."""
    rng = np.random.default_rng(1)
    graphs = []
    for n, p in [(30, 0.4), (70, 0.15), (1, 0.0), (45, 0.25), (2, 1.0)]:
        e = [(a, b) for a in range(n) for b in range(a + 1, n) if rng.random() < p and b != n - 1]
        if n > 2:
            graphs.append((n, e))
    return GraphSet.from_edge_lists(graphs)
