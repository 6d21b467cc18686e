"""Yardstick and inputs of the labelled large-query ground-truth tests: networkx VF2 with ``node_match`` on the label,
run as the reference runs it (workload.py:327-348: one match per isomorphism, keyed by ``max(vmap.keys())``;
data.py:61-68: divided by the labelled automorphism count), on the two graph sets of groundtruth_vf2.py with seeded
uniform labels and the ten large queries labelled from occurrences.  Nothing here touches the package under test."""
import functools
import itertools

import networkx as nx
import numpy as np

import groundtruth_vf2 as V

GM = nx.algorithms.isomorphism.GraphMatcher
KEY = "feat"


def _same(a, b):
    return a[KEY] == b[KEY]


def one_hot(label, F):
    return [1.0 if i == label else 0.0 for i in range(F)]


def seeded_labels(graphs, F, seed=11):
    """one int array of uniform labels 0..F-1 per graph"""
    rng = np.random.default_rng(seed)
    return [rng.integers(F, size=n) for n, _ in graphs]


def features(labels, F):
    """the labels as one-hot float32 rows, one array per graph (GraphSet.from_edge_lists(node_feat=...))"""
    return [np.eye(F, dtype=np.float32)[l] for l in labels]


def labelled(g, labels, F):
    """a copy of networkx graph g whose node v carries the one-hot feature of labels[v] (a dict or a sequence)"""
    out = nx.Graph()
    for v in g.nodes:
        out.add_node(v, **{KEY: one_hot(int(labels[v]), F)})
    out.add_edges_from(g.edges())
    return out


def expansion(q, F):
    """every labelling of q with F labels: F ** n labelled copies, most of them isomorphic to each other"""
    nodes = list(q.nodes)
    return [labelled(q, dict(zip(nodes, labs)), F) for labs in itertools.product(range(F), repeat=len(nodes))]


def vf2_counts_labelled(graphs, labels, F, queries):
    """graphs: [(n, edges)], labels: one int array per graph, queries: labelled nx graphs -> int64 [sum n, Q]"""
    targets = [labelled(V.to_nx(n, e), l, F) for (n, e), l in zip(graphs, labels)]
    out = np.zeros((sum(n for n, _ in graphs), len(queries)), dtype=np.int64)
    for qi, q in enumerate(queries):
        sym = sum(1 for _ in GM(q, q, node_match=_same).subgraph_isomorphisms_iter())
        base = 0
        for t in targets:
            for vmap in GM(t, q, node_match=_same).subgraph_isomorphisms_iter():
                out[base + max(vmap.keys()), qi] += 1
            base += t.number_of_nodes()
        assert (out[:, qi] % sym == 0).all()            # every occurrence is found once per labelled automorphism
        out[:, qi] //= sym
    return out


def occurrence_queries(graphs, labels, F, queries, unlabelled):
    """Random labellings of large queries almost never occur, so the labels are read off occurrences: for each query
    the first unlabelled VF2 match in the first graph that has one and in the second such graph (when one graph alone
    has occurrences: its first and its last match); the target's labels are copied onto the query.  Two labelled
    queries per query that occurs at all, none for the others.  ``unlabelled``: the unlabelled VF2 counts of the
    queries, which tell the graphs without any occurrence (not searched again)."""
    targets = [V.to_nx(n, e) for n, e in graphs]
    ptr = np.concatenate([[0], np.cumsum([n for n, _ in graphs])])
    out = []
    for qi, q in enumerate(queries):
        found = []                                                          # (graph, target node -> query node)
        for g, t in enumerate(targets):
            if unlabelled[ptr[g]:ptr[g + 1], qi].sum() == 0:
                continue
            found.append((g, next(GM(t, q).subgraph_isomorphisms_iter())))
            if len(found) == 2:
                break
        if len(found) == 1:
            g = found[0][0]
            for vmap in GM(targets[g], q).subgraph_isomorphisms_iter():
                pass
            found.append((g, vmap))
        out += [labelled(q, {qv: labels[g][tv] for tv, qv in vmap.items()}, F) for g, vmap in found]
    return out


@functools.lru_cache(maxsize=None)
def yardstick(which, F):
    """(graphs, labels, labelled queries, VF2 counts) of "sparse" or "dense" with F labels, computed once per process."""
    graphs, _, plain, unlabelled = V.yardstick(which)
    labels = seeded_labels(graphs, F)
    queries = occurrence_queries(graphs, labels, F, plain, unlabelled)
    counts = vf2_counts_labelled(graphs, labels, F, queries)
    assert len(queries) == (16 if which == "sparse" else 18)
    assert (counts.sum(axis=0) > 0).all(), counts.sum(axis=0).tolist()
    return graphs, labels, queries, counts


def check_nonzero(F):
    """The conditions that keep an all-zero comparison from passing, asserted on the VF2 side: every column of both
    sets is non-zero (yardstick) and the query sizes 7, 8, 9, 10, 12 and 14 are covered by the union of the sets."""
    sizes = set()
    for which in ("sparse", "dense"):
        _, _, queries, counts = yardstick(which, F)
        sizes |= {len(q) for q, t in zip(queries, counts.sum(axis=0)) if t > 0}
    assert {7, 8, 9, 10, 12, 14} <= sizes, sizes
