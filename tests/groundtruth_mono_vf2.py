"""Yardstick and inputs of the NON-INDUCED ground-truth tests: networkx VF2 monomorphisms
(``GraphMatcher(target, query).subgraph_monomorphisms_iter()``: injective maps that send every query edge onto a target
edge), keyed by ``max(vmap.keys())`` and divided by the query's automorphism count; with ``node_match`` for labelled
queries.  Nothing here touches the package under test.

Sizes.  VF2 walks every monomorphism, |Aut(q)| per occurrence.  The unlabelled targets are the whole sparse set of
groundtruth_vf2 (12 molecule-like graphs with shuffled ids, 433 nodes: 3 s for the 34 queries on one core of the build
box) and, so that the denser queries occur at all, the first graph (DENSE_COUNT = 1) of its dense set (G(18, 0.3): 18
nodes, 8 s -- P7 alone has 29 067 occurrences in it).  The labelled targets are the first LABELLED_COUNT = 6
sparse graphs (208 nodes, under a second)."""
import functools
import math

import networkx as nx
import numpy as np

import groundtruth_vf2 as V
import groundtruth_labelled_vf2 as LV
from helpers import standard_queries

GM = nx.algorithms.isomorphism.GraphMatcher
DENSE_COUNT, LABELLED_COUNT = 1, 6


def automorphisms(q, node_match=None):
    return sum(1 for _ in GM(q, q, node_match=node_match).isomorphisms_iter())


def mono_counts(graphs, queries, targets=None, node_match=None):
    """graphs: [(n, edges)], queries: [nx.Graph] -> int64 [sum n, len(queries)], rows in graph order.  ``targets``:
    the graphs as networkx graphs when they carry attributes (labelled runs)."""
    targets = targets if targets is not None else [V.to_nx(n, e) for n, e in graphs]
    out = np.zeros((sum(n for n, _ in graphs), len(queries)), dtype=np.int64)
    for qi, q in enumerate(queries):
        sym = automorphisms(q, node_match)
        base = 0
        for t in targets:
            for vmap in GM(t, q, node_match=node_match).subgraph_monomorphisms_iter():
                out[base + max(vmap.keys()), qi] += 1
            base += t.number_of_nodes()
        assert (out[:, qi] % sym == 0).all()            # every occurrence is found once per automorphism
        out[:, qi] //= sym
    return out


def standard_nx():
    """the 29 standard queries (3..5 nodes) as networkx graphs"""
    return [V.to_nx(n, e) for n, e in standard_queries()[1]]


def seven_node_queries():
    """name -> query: P7, C7, K1,6, the 7-node binary tree, a triangle bridged to a 4-ring"""
    return {"P7": nx.path_graph(7), "C7": nx.cycle_graph(7), "K1,6": nx.star_graph(6),
            "tree7": nx.balanced_tree(2, 2), "tri-bridge-C4": V.triangle_bridge_ring()}


def all_queries():
    return standard_nx() + list(seven_node_queries().values())


def targets(which):
    return V.sparse_set() if which == "sparse" else V.dense_set()[:DENSE_COUNT]


@functools.lru_cache(maxsize=None)
def yardstick(which):
    """(graphs, queries, VF2 monomorphism counts) of "sparse" or "dense", computed once per process"""
    graphs, queries = targets(which), all_queries()
    return graphs, queries, mono_counts(graphs, queries)


def twelve_six_node_queries():
    """a dozen 6-node queries, sparse to complete: every tenth connected 6-node atlas graph, the last replaced by K6"""
    from networkx.generators.atlas import graph_atlas_g
    six = [g for g in graph_atlas_g() if g.number_of_nodes() == 6 and nx.is_connected(g)]
    assert len(six) == 112
    picked = six[::10]
    assert len(picked) == 12 and six[-1].number_of_edges() == 15
    return picked[:-1] + [six[-1]]


def complete_graph_counts(n, q):
    """closed form on K_n with ids 0..n-1: count[v][q] = C(v, k-1) k! / |Aut(q)| for a k-node query q"""
    k = q.number_of_nodes()
    per_subset = math.factorial(k) // automorphisms(q)
    return [math.comb(v, k - 1) * per_subset for v in range(n)]


# ---- labelled ---------------------------------------------------------------------------------------------------------
def labelled_inputs(F=2):
    """(graphs, labels, networkx targets with one-hot features) of the labelled test"""
    graphs = V.sparse_set()[:LABELLED_COUNT]
    labels = LV.seeded_labels(graphs, F)
    targets = [LV.labelled(V.to_nx(n, e), l, F) for (n, e), l in zip(graphs, labels)]
    return graphs, labels, targets


def labelled_queries(F=2):
    """the F = 2 expansions of P2, P3, P4, C3, C4 and C5 (4 + 8 + 16 + 8 + 16 + 32 = 84 labelled copies) and the first
    16 copies of P7's expansion"""
    small = [nx.path_graph(2), nx.path_graph(3), nx.path_graph(4), nx.cycle_graph(3), nx.cycle_graph(4),
             nx.cycle_graph(5)]
    return [g for q in small for g in LV.expansion(q, F)] + LV.expansion(nx.path_graph(7), F)[:16]


@functools.lru_cache(maxsize=None)
def labelled_yardstick(F=2):
    graphs, labels, targets = labelled_inputs(F)
    queries = labelled_queries(F)
    return graphs, labels, queries, mono_counts(graphs, queries, targets, LV._same)
