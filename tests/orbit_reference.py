"""Brute-force yardstick of the orbit counts (groundtruth.orbit_counts): networkx + itertools, no code of the library.

Induced: every k-subset of a graph is tested for connectivity and matched against the queries with ``GraphMatcher``;
every member is tallied in the orbit of the query position it maps to.  Non-induced: every monomorphism of the query
into the graph tallies every image node in the orbit of its pre-image, and the tally is divided by |Aut(q)|.  Orbits are
those of Aut(q) on the query's positions, numbered in ascending order of their smallest member; columns are the queries
in order and, inside a query, its orbits in order."""
import itertools

import networkx as nx
import numpy as np

GM = nx.algorithms.isomorphism.GraphMatcher


def as_nx(q):
    """(n, edges) or nx.Graph -> nx.Graph on positions 0..n-1 (positions of a graph: list(q.nodes))"""
    if hasattr(q, "nodes"):
        nodes = list(q.nodes)
        idx = {v: i for i, v in enumerate(nodes)}
        n, edges = len(nodes), [(idx[a], idx[b]) for a, b in q.edges()]
    else:
        n, edges = int(q[0]), list(q[1])
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_edges_from(edges)
    return g


def automorphisms(q):
    return [dict(m) for m in GM(q, q).isomorphisms_iter()]


def orbits(q):
    """(orbit index of every position, list of member tuples) of nx.Graph ``q`` on 0..n-1"""
    low = {i: i for i in q.nodes}
    for m in automorphisms(q):
        for i, j in m.items():
            low[i] = min(low[i], j)
    firsts = sorted(set(low.values()))
    orbit_of = [firsts.index(low[i]) for i in range(len(q))]
    return orbit_of, [tuple(i for i in range(len(q)) if orbit_of[i] == o) for o in range(len(firsts))]


def columns(queries):
    return [(qi, o, mem) for qi, q in enumerate(queries) for o, mem in enumerate(orbits(as_nx(q))[1])]


def orbit_counts_reference(graphs, queries, induced=True):
    """int64 [total nodes, columns]; ``graphs``: list of (n, edges)"""
    qs = [as_nx(q) for q in queries]
    orb = [orbits(q)[0] for q in qs]
    first = np.concatenate([[0], np.cumsum([max(o) + 1 for o in orb])]).astype(int)
    total = sum(n for n, _ in graphs)
    out = np.zeros((total, first[-1]), dtype=np.int64)
    base = 0
    for n, edges in graphs:
        g = as_nx((n, edges))
        if induced:
            for k in sorted({len(q) for q in qs}):
                for sub in itertools.combinations(range(n), k):
                    h = g.subgraph(sub)
                    if h.number_of_edges() < k - 1 or not nx.is_connected(h):
                        continue
                    for qi, q in enumerate(qs):
                        if len(q) != k or q.number_of_edges() != h.number_of_edges():
                            continue
                        gm = GM(h, q)
                        if gm.is_isomorphic():
                            for v, pos in gm.mapping.items():
                                out[base + v, first[qi] + orb[qi][pos]] += 1
        else:
            for qi, q in enumerate(qs):
                aut = len(automorphisms(q))
                part = np.zeros((n, first[qi + 1] - first[qi]), dtype=np.int64)
                for vmap in GM(g, q).subgraph_monomorphisms_iter():
                    for v, pos in vmap.items():
                        part[v, orb[qi][pos]] += 1
                assert (part % aut == 0).all()
                out[base:base + n, first[qi]:first[qi + 1]] = part // aut
        base += n
    return out


def connected_subsets(n, edges, kmax=5):
    """number of connected node subsets of 2..kmax nodes (what a test pays for one graph)"""
    g = as_nx((n, edges))
    return sum(1 for k in range(2, kmax + 1) for s in itertools.combinations(range(n), k)
               if nx.is_connected(g.subgraph(s)))


def column_of(queries, pattern, node):
    """the column that counts ``node`` of nx.Graph ``pattern``: the first query isomorphic to it, the orbit of the
    position the node maps to"""
    col = 0
    for q in (as_nx(q) for q in queries):
        orbit_of, members = orbits(q)
        gm = GM(pattern, q)
        if len(q) == len(pattern) and gm.is_isomorphic():
            return col + orbit_of[gm.mapping[node]]
        col += len(members)
    raise KeyError("pattern not among the queries")
