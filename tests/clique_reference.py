"""Plain-Python clique counts, written for the clique census tests and nothing else: networkx's clique enumeration for
totals and per-node columns, a direct restatement of the pass-index peel key, and the named families with closed forms.
All counts are taken modulo 2^64 and returned as the int64 bit patterns the library stores."""
from math import comb

import networkx as nx
import numpy as np

from decomposition_reference import clique, gnp  # noqa: F401
from desco_amd.graphs import GraphSet

MASK = (1 << 64) - 1


def as_i64(x: int) -> int:
    """The int64 bit pattern of x mod 2^64"""
    x &= MASK
    return x - (1 << 64) if x >> 63 else x


def nx_graph(n, edges):
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_edges_from(edges)
    return g


def clique_counts(n, edges, kmax):
    """(totals [kmax], per node [n][kmax], omega) of one graph by listing every clique (Python ints)."""
    totals, nodes, omega = [0] * kmax, [[0] * kmax for _ in range(n)], 0
    for c in nx.enumerate_all_cliques(nx_graph(n, edges)):
        omega = max(omega, len(c))
        if len(c) <= kmax:
            totals[len(c) - 1] += 1
            for v in c:
                nodes[v][len(c) - 1] += 1
    return totals, nodes, omega


def peel_key(n, edges):
    """(key, core) of one graph: at level k a pass removes every node whose remaining degree is <= k at the START of
    the pass; a level repeats passes until one removes nothing; only passes that remove a node are numbered."""
    adj = [set() for _ in range(n)]
    for a, b in edges:
        adj[a].add(b), adj[b].add(a)
    key, core, live, k, index = [0] * n, [0] * n, set(range(n)), 0, 0
    while live:
        low = [v for v in live if len(adj[v]) <= k]
        if not low:
            k += 1
            continue
        for v in low:
            key[v], core[v] = index, k
            live.discard(v)
        for v in low:
            for u in adj[v]:
                adj[u].discard(v)
            adj[v] = set()
        index += 1
    return key, core


def census(graphs: GraphSet, kmax: int):
    """(graph_cliques int64 [G, kmax], node_cliques int64 [N, kmax], omega int32 [G], key int32 [N], core int32 [N])"""
    gc, nc, om, key, core = [], [], [], [], []
    for n, edges in graphs.edge_lists():
        t, per, w = clique_counts(n, edges, kmax)
        k, c = peel_key(n, edges)
        assert c == [nx.core_number(nx_graph(n, edges))[v] for v in range(n)]
        gc.append([as_i64(x) for x in t]), om.append(w)
        nc += [[as_i64(x) for x in row] for row in per]
        key += k
        core += c
    return (np.array(gc, np.int64).reshape(-1, kmax), np.array(nc, np.int64).reshape(-1, kmax), np.array(om, np.int32),
            np.array(key, np.int32), np.array(core, np.int32))


# ---- the named families with closed forms ------------------------------------------------------------------------------
def multipartite(parts):
    """(n, edges) of the complete multipartite graph with these part sizes"""
    part = [i for i, s in enumerate(parts) for _ in range(s)]
    n = len(part)
    return n, [(a, b) for a in range(n) for b in range(a + 1, n) if part[a] != part[b]]


def elementary_symmetric(values, kmax):
    """e_1 .. e_kmax of the values"""
    e = [1] + [0] * kmax
    for x in values:
        for k in range(kmax, 0, -1):
            e[k] += e[k - 1] * x
    return e[1:]


def complete_closed_form(n, kmax):
    """(totals, per-node row, omega) of K_n"""
    return [as_i64(comb(n, k)) for k in range(1, kmax + 1)], [as_i64(comb(n - 1, k - 1)) for k in range(1, kmax + 1)], n


def multipartite_closed_form(parts, kmax):
    """(totals, {part index: per-node row}, omega): a k-clique takes one node from each of k parts"""
    totals = [as_i64(x) for x in elementary_symmetric(parts, kmax)]
    rows = {}
    for i in range(len(parts)):
        rest = elementary_symmetric(parts[:i] + parts[i + 1:], kmax)
        rows[i] = [as_i64(x) for x in [1] + rest[:kmax - 1]]
    return totals, rows, len(parts)


def star(leaves):
    return leaves + 1, [(0, v) for v in range(1, leaves + 1)]


def family_graphs():
    """[(name, n, edges)]: every out-degree at which the kernel changes its launch (K9 .. K65), a graph that branches at
    every level, a hub above a wave's lanes, more roots than lanes, and the empty shapes."""
    out = [(f"K{k}", k, clique(k)) for k in (1, 2, 3, 5, 9, 10, 17, 18, 33, 34, 64, 65)]
    out.append(("K3x7", *multipartite([3] * 7)))
    out.append(("K2x12", *multipartite([2] * 12)))
    out.append(("star 200", *star(200)))
    out.append(("empty 5", 5, []))
    out.append(("single edge", 2, [(0, 1)]))
    out.append(("path 150", 150, [(i, i + 1) for i in range(149)]))
    out.append(("two K5 sharing a triangle", 7,
                sorted(set(clique(5) + [tuple(sorted((a, b))) for a in (0, 1, 2, 5, 6) for b in (0, 1, 2, 5, 6) if a < b]))))
    out.append(("G(90, 0.3)",) + gnp(90, 0.3, 11))
    return out


def families() -> GraphSet:
    return GraphSet.from_edge_lists([(n, e) for _, n, e in family_graphs()])


def dense_random() -> GraphSet:
    """Random graphs dense enough to branch deeply: G(n, p) with n <= 28"""
    return GraphSet.from_edge_lists([gnp(n, p, seed) for seed, (n, p) in enumerate(
        [(28, 0.1), (27, 0.3), (28, 0.6), (26, 0.85), (20, 0.6), (14, 0.85), (9, 0.3), (28, 0.85)])])
