"""Brute-force yardstick of the edge orbit counts (groundtruth.edge_orbit_counts): itertools only, no code of the library.

Induced: every k-subset of a graph's nodes (``itertools.combinations``) is tested for connectivity and mapped onto the
queries by trying every permutation; every edge of the subset is tallied in the orbit of the query edge it maps to.
Non-induced: every injective edge-preserving map of the query into the graph tallies every image edge in the orbit of
its pre-image, and the tally is divided by |Aut(q)|.  Edge orbits are those of Aut(q) on the query's edges: the edges
are ordered by b(b-1)/2 + a (a < b), the orbits numbered in ascending order of their smallest member; columns are the
queries in order and, inside a query, its edge orbits in order.  Rows are the edges (u, v), u < v, of all graphs in
ascending (v, u), graph after graph."""
import itertools

import numpy as np


def as_query(q):
    """(n, edges) or nx.Graph -> (n, sorted list of edges (a, b), a < b, on positions 0..n-1 = list(q.nodes))"""
    if hasattr(q, "nodes"):
        nodes = list(q.nodes)
        idx = {v: i for i, v in enumerate(nodes)}
        n, edges = len(nodes), [(idx[a], idx[b]) for a, b in q.edges()]
    else:
        n, edges = int(q[0]), list(q[1])
    return n, sorted({(min(a, b), max(a, b)) for a, b in edges}, key=rank)


def rank(e):
    a, b = min(e), max(e)
    return b * (b - 1) // 2 + a


def automorphisms(q):
    n, edges = as_query(q)
    es = set(edges)
    return [p for p in itertools.permutations(range(n))
            if {(min(p[a], p[b]), max(p[a], p[b])) for a, b in edges} == es]


def edge_orbits(q):
    """({edge: orbit index}, list of member tuples) of the query's edges"""
    n, edges = as_query(q)
    low = {e: rank(e) for e in edges}
    for p in automorphisms(q):
        for a, b in edges:
            low[(a, b)] = min(low[(a, b)], rank((p[a], p[b])))
    firsts = sorted(set(low.values()))
    orbit_of = {e: firsts.index(low[e]) for e in edges}
    return orbit_of, [tuple(e for e in edges if orbit_of[e] == o) for o in range(len(firsts))]


def columns(queries):
    return [(qi, o, mem) for qi, q in enumerate(queries) for o, mem in enumerate(edge_orbits(q)[1])]


def rows(graphs):
    """[(u, v)] global ids, u < v, ascending (v, u) inside a graph, graph after graph"""
    out, base = [], 0
    for n, edges in graphs:
        es = sorted({(max(a, b), min(a, b)) for a, b in edges})
        out += [(base + u, base + v) for v, u in es]
        base += n
    return out


def _connected(sub, adj):
    seen, todo = {sub[0]}, [sub[0]]
    while todo:
        x = todo.pop()
        for y in sub:
            if y not in seen and y in adj[x]:
                seen.add(y)
                todo.append(y)
    return len(seen) == len(sub)


def edge_orbit_counts_reference(graphs, queries, induced=True):
    """int64 [total edges, columns]; ``graphs``: list of (n, edges)"""
    qs = [as_query(q) for q in queries]
    orb = [edge_orbits(q)[0] for q in qs]
    auts = [len(automorphisms(q)) for q in qs]
    first = np.concatenate([[0], np.cumsum([max(o.values()) + 1 for o in orb])]).astype(int)
    row_of = {e: i for i, e in enumerate(rows(graphs))}
    out = np.zeros((len(row_of), first[-1]), dtype=np.int64)
    base = 0
    for n, edges in graphs:
        adj = [set() for _ in range(n)]
        for a, b in edges:
            adj[a].add(b)
            adj[b].add(a)
        row = lambda x, y: row_of[(base + min(x, y), base + max(x, y))]      # noqa: E731
        for qi, (k, qe) in enumerate(qs):
            part = np.zeros((len(row_of), first[qi + 1] - first[qi]), dtype=np.int64)
            for sub in itertools.combinations(range(n), k):
                if induced:
                    inside = sum(1 for a, b in itertools.combinations(sub, 2) if b in adj[a])
                    if inside != len(qe) or not _connected(sub, adj):
                        continue
                for f in itertools.permutations(sub):                  # query position a -> node f[a]
                    if all(f[b] in adj[f[a]] for a, b in qe):
                        for a, b in qe:
                            part[row(f[a], f[b]), orb[qi][(a, b)]] += 1
                        if induced:
                            break                                      # one isomorphism: the orbit does not depend on it
            if not induced:
                assert (part % auts[qi] == 0).all()
                part //= auts[qi]
            out[:, first[qi]:first[qi + 1]] += part
        base += n
    return out


def column_of(queries, pattern, edge):
    """the column that counts ``edge`` (a pair of positions) of the query ``pattern``, which must be among ``queries``
    up to isomorphism: the first query isomorphic to it, the orbit of the edge the pair maps to"""
    pn, pe = as_query(pattern)
    col = 0
    for q in queries:
        n, qe = as_query(q)
        orbit_of, members = edge_orbits(q)
        if n == pn and len(qe) == len(pe):
            qs = set(qe)
            for f in itertools.permutations(range(n)):                 # pattern position a -> query position f[a]
                if {(min(f[a], f[b]), max(f[a], f[b])) for a, b in pe} == qs:
                    a, b = edge
                    return col + orbit_of[(min(f[a], f[b]), max(f[a], f[b]))]
        col += len(members)
    raise KeyError("pattern not among the queries")
