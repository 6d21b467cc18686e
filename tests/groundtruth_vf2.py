"""Yardstick and inputs of the large-query ground-truth tests: networkx VF2 run as the reference runs it
(workload.py:327-348: one match per isomorphism, keyed by ``max(vmap.keys())``; data.py:61-67: divided by the query's
automorphism count), two graph sets and the ten queries.  Nothing here touches the package under test."""
import functools

import networkx as nx
import numpy as np

GM = nx.algorithms.isomorphism.GraphMatcher


def to_nx(n, edges):
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_edges_from(edges)
    return g


def vf2_counts(graphs, queries):
    """graphs: [(n, edges)], queries: [nx.Graph] -> int64 [sum n, len(queries)], rows in graph order."""
    targets = [to_nx(n, e) for n, e in graphs]
    out = np.zeros((sum(n for n, _ in graphs), len(queries)), dtype=np.int64)
    for qi, q in enumerate(queries):
        sym = sum(1 for _ in GM(q, q).subgraph_isomorphisms_iter())
        base = 0
        for t in targets:
            for vmap in GM(t, q).subgraph_isomorphisms_iter():
                out[base + max(vmap.keys()), qi] += 1
            base += t.number_of_nodes()
        assert (out[:, qi] % sym == 0).all()            # every subset is found once per automorphism
        out[:, qi] //= sym
    return out


def fused_rings():
    """Two 6-rings sharing an edge (10 nodes, 11 edges: the naphthalene skeleton)."""
    g = nx.cycle_graph(6)
    nx.add_path(g, [0, 6, 7, 8, 9, 5])
    return g


def triangle_bridge_ring():
    """A triangle joined to a 4-ring through a bridge: 7 nodes, 8 edges."""
    g = nx.cycle_graph(3)
    g.add_edges_from([(3, 4), (4, 5), (5, 6), (6, 3), (2, 3)])
    return g


def large_queries():
    """name -> query: sizes 7 (four of them), 8, 9, 10, 12 and 14, and C6 as a small control."""
    return {
        "P7": nx.path_graph(7),
        "C8": nx.cycle_graph(8),
        "K1,6": nx.star_graph(6),
        "tree7": nx.balanced_tree(2, 2),
        "fused": fused_rings(),
        "P12": nx.path_graph(12),
        "P14": nx.path_graph(14),
        "tri-bridge-C4": triangle_bridge_ring(),
        "lollipop(4,5)": nx.lollipop_graph(4, 5),
        "C6": nx.cycle_graph(6),
    }


# seeds for which VF2 alone meets the conditions of check_nonzero (chosen by running VF2, not the code under test)
SPARSE_SEED, DENSE_SEED = 28, 146


def _shuffled(rng, n, edges):
    perm = rng.permutation(n)
    return n, sorted({(int(min(perm[a], perm[b])), int(max(perm[a], perm[b]))) for a, b in edges})


def sparse_set(seed=SPARSE_SEED, count=12):
    """Molecule-like graphs of 20..45 nodes: a random tree with short back edges (node i hangs off the node before it,
    now and then off the second or third before it), plus n/6 extra edges that close rings of 3, 4, 6 (mostly) or 8
    nodes; ids shuffled."""
    rng = np.random.default_rng(seed)
    graphs = []
    for _ in range(count):
        n = int(rng.integers(20, 46))
        edges = {(i - min(i, int(rng.choice([1, 1, 1, 1, 2, 3]))), i) for i in range(1, n)}
        extra = 0
        while extra < n // 6:
            a = int(rng.integers(0, n - 2))
            b = min(a + int(rng.choice([2, 3, 5, 5, 5, 7])), n - 1)
            if (a, b) not in edges:
                edges.add((a, b))
                extra += 1
        graphs.append(_shuffled(rng, n, sorted(edges)))
    return graphs


def dense_set(seed=DENSE_SEED, count=3):
    """G(18, 0.3)."""
    rng = np.random.default_rng(seed)
    graphs = []
    for _ in range(count):
        edges = [(a, b) for a in range(18) for b in range(a + 1, 18) if rng.random() < 0.3]
        graphs.append((18, edges))
    return graphs


@functools.lru_cache(maxsize=None)
def yardstick(which):
    """(graphs, query names, queries, VF2 counts) of "sparse" or "dense", computed once per process."""
    graphs = sparse_set() if which == "sparse" else dense_set()
    qs = large_queries()
    return graphs, list(qs), list(qs.values()), vf2_counts(graphs, list(qs.values()))


def check_nonzero(per_set_counts, queries):
    """The conditions that keep an all-zero comparison from passing: per set at least 8 of the 10 query columns have a
    nonzero total, and every query size 7, 8, 10, 12, 14 has a nonzero total in at least one set."""
    sizes = set()
    for counts in per_set_counts:
        totals = counts.sum(axis=0)
        assert (totals > 0).sum() >= 8, totals.tolist()
        sizes |= {len(q) for q, t in zip(queries, totals) if t > 0}
    assert {7, 8, 10, 12, 14} <= sizes, sizes
