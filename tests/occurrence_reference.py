"""The yardstick of the occurrence listers (desco_amd/occurrences.py): which occurrences a graph holds, found without
the project's matcher.

An occurrence is identified by a hashable KEY: induced -- the node set (a sorted tuple); non-induced -- the image edge
set (a sorted tuple of sorted pairs).  Every lister here returns ``{largest node: set of keys}`` with GLOBAL node ids;
``row_key`` turns a row of the listers under test into its key.

``vf2_groups``         networkx VF2: every isomorphism / monomorphism, grouped by key (|Aut(q)| maps per group)
``brute_force_groups`` itertools.combinations over the node subsets of graphs of at most 9 nodes
``star_total``         stars in stars, where VF2 would walk n (n-1) .. (n-m+1) maps: the count, and why it suffices
"""
import itertools
import math

import networkx as nx
import numpy as np

from desco_amd.graphs import GraphSet


def query_graph(query):
    k, edges = query
    q = nx.Graph()
    q.add_nodes_from(range(k))
    q.add_edges_from(edges)
    return q


def targets(graphs: GraphSet):
    """[(first global node id, networkx graph on local ids)]"""
    out = []
    for g, (n, edges) in enumerate(graphs.edge_lists()):
        t = nx.Graph()
        t.add_nodes_from(range(n))
        t.add_edges_from(edges)
        out.append((int(graphs.graph_ptr[g]), t))
    return out


def row_key(row, query, induced):
    """The key of the occurrence a row (images of query nodes 0..k-1) claims to be."""
    if induced:
        return tuple(sorted(int(x) for x in row))
    return tuple(sorted(tuple(sorted((int(row[a]), int(row[b])))) for a, b in query[1]))


def _add(groups, key, induced):
    v = max(key) if induced else max(max(e) for e in key)
    groups.setdefault(v, set()).add(key)


def vf2_groups(graphs: GraphSet, query, induced=True):
    q = query_graph(query)
    groups, maps = {}, 0
    GM = nx.algorithms.isomorphism.GraphMatcher
    for base, t in targets(graphs):
        gm = GM(t, q)
        for vmap in (gm.subgraph_isomorphisms_iter() if induced else gm.subgraph_monomorphisms_iter()):
            f = {a: base + u for u, a in vmap.items()}
            _add(groups, row_key([f[a] for a in range(query[0])], query, induced), induced)
            maps += 1
    # every group holds the same number of maps, |Aut(q)| (the count the reference divides by)
    sym = sum(1 for _ in GM(q, q).isomorphisms_iter())
    assert maps == sym * sum(len(s) for s in groups.values())
    return groups


def brute_force_groups(graphs: GraphSet, query, induced=True):
    """Every k-subset of every graph (at most 9 nodes each).  Induced: the subset is an occurrence iff its induced
    subgraph is isomorphic to the query.  Non-induced: every k-edge-count subset of the subset's edges that spans it and
    is isomorphic to the query is one occurrence."""
    q = query_graph(query)
    k, m = query[0], len(query[1])
    groups = {}
    for base, t in targets(graphs):
        assert t.number_of_nodes() <= 9, "brute force is for graphs of at most 9 nodes"
        for S in itertools.combinations(range(t.number_of_nodes()), k):
            sub = t.subgraph(S)
            if induced:
                if sub.number_of_edges() == m and nx.is_isomorphic(sub, q):
                    _add(groups, tuple(base + u for u in S), True)
                continue
            for es in itertools.combinations(sorted(tuple(sorted(e)) for e in sub.edges()), m):
                h = nx.Graph(list(es))
                if h.number_of_nodes() == k and nx.is_isomorphic(h, q):
                    _add(groups, tuple(sorted((base + a, base + b) for a, b in es)), False)
    return groups


def star_total(graphs: GraphSet, leaves_in_query: int) -> int:
    """The number of occurrences of the star K1,m (m = leaves_in_query >= 2) in a set of stars K1,n.  A star's only node
    of degree above 1 is its hub and its leaves are pairwise non-adjacent, so the query's hub lands on the hub and the
    occurrences -- induced and non-induced alike -- are exactly hub + every m-subset of the leaves: C(n, m) per star,
    where VF2 would walk n! / (n - m)! maps (22 million for K1,4 in K1,70).  A listing of pairwise different valid
    rows with this total therefore hits every occurrence exactly once."""
    assert leaves_in_query >= 2
    total = 0
    for _, t in targets(graphs):
        n = t.number_of_nodes()
        assert t.number_of_edges() == n - 1 and max(d for _, d in t.degree()) == n - 1, "not a star"
        total += math.comb(n - 1, leaves_in_query)
    return total


def adjacency(graphs: GraphSet) -> np.ndarray:
    """Dense bool adjacency over global ids (test-sized graph sets only)."""
    n = graphs.num_nodes
    a = np.zeros((n, n), dtype=bool)
    src = np.repeat(np.arange(n), np.diff(graphs.rowptr))
    a[src, graphs.col] = True
    return a
