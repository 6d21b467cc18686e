"""Exact ground truth for queries of 7..16 nodes on the host: the pattern-guided matcher (csrc/groundtruth_match.cpp)
against networkx VF2 run as the reference runs it (groundtruth_vf2.py), the reference's recorded counts and the ESU
enumerator.  Integers, bit-exact."""
import ctypes

import networkx as nx
import numpy as np
import pytest
import torch

import groundtruth_vf2 as V
from desco_amd import _lib, groundtruth
from desco_amd.graphs import GraphSet
from desco_amd.groundtruth import canonical_counts, canonical_counts_match, match_plan
from helpers import golden_graphs, standard_queries

HEAD, REC, NODE, PARENT, ADJ, LT, GT = 2, 84, 4, 20, 36, 52, 68


def test_vf2_yardstick_is_not_all_zero():
    """Asserted on the VF2 side alone, so that no comparison below passes on zeros."""
    _, _, queries, sparse = V.yardstick("sparse")
    dense = V.yardstick("dense")[3]
    V.check_nonzero([sparse, dense], queries)


@pytest.mark.parametrize("which", ["sparse", "dense"])
def test_large_queries_match_vf2(which):
    graphs, names, queries, want = V.yardstick(which)
    V.check_nonzero([V.yardstick("sparse")[3], V.yardstick("dense")[3]], queries)
    gs = GraphSet.from_edge_lists(graphs)
    got = canonical_counts_match(gs, queries, backend="host")
    assert got.dtype == torch.double and got.shape == want.shape
    assert got.long().tolist() == want.tolist()
    assert groundtruth.last_match_backend == "host"
    # the public entry: large columns to the matcher, C6 to ESU, joined in query order
    assert canonical_counts(gs, queries, backend="host").long().tolist() == want.tolist()
    # and the package's own vf2 backend is the same procedure
    if which == "dense":
        assert canonical_counts(gs, queries[:2], backend="vf2").long().tolist() == want[:, :2].tolist()


def test_matcher_equals_reference_vf2_golden(partition_golden, queries_golden, counts_golden):
    qs = [(q["n"], [tuple(e) for e in q["edges"]]) for q in queries_golden["queries"]]
    by_name = {g["name"]: g for g in partition_golden["graphs"]}
    graphs = [(by_name[c["name"]]["n"], [tuple(e) for e in by_name[c["name"]]["edges"]]) for c in counts_golden]
    got = canonical_counts_match(GraphSet.from_edge_lists(graphs), qs, backend="host")
    want = np.concatenate([np.array(c["count"]) for c in counts_golden])
    assert len(qs) == 29 and want.sum() > 1000
    assert got.long().tolist() == want.astype(np.int64).tolist()


def test_six_node_atlas_queries_equal_esu():
    from desco_amd.data import gen_query_ids, graph_atlas_plus
    queries = [graph_atlas_plus(i) for i in gen_query_ids([6])]
    assert len(queries) == 112
    gs = GraphSet.from_edge_lists(golden_graphs(max_n=40))
    esu = canonical_counts(gs, queries, backend="host")
    got = canonical_counts_match(gs, queries, backend="host")
    assert esu.sum() > 1000 and (esu.sum(0) > 0).sum() > 50
    assert got.long().tolist() == esu.long().tolist()


def test_duplicate_queries_get_equal_columns():
    graphs = V.dense_set()
    gs = GraphSet.from_edge_lists(graphs)
    p7 = nx.path_graph(7)
    relabelled = nx.relabel_nodes(p7, {0: 3, 3: 0, 1: 6, 6: 1})            # the same pattern, other node names
    got = canonical_counts_match(gs, [p7, nx.cycle_graph(8), relabelled, p7], backend="host").long()
    assert got[:, 0].sum() > 0
    assert got[:, 0].tolist() == got[:, 2].tolist() == got[:, 3].tolist()
    assert got[:, 0].tolist() != got[:, 1].tolist()


def test_routing_of_a_mixed_query_set():
    graphs, _, large, want = V.yardstick("dense")
    gs = GraphSet.from_edge_lists(graphs)
    _, std = standard_queries()
    small = std[:5] + [(6, [(i, (i + 1) % 6) for i in range(6)])]
    mixed = [large[0], small[0], small[1], large[1], small[2], small[3], small[4], large[4], small[5], large[7]]
    is_large = [True, False, False, True, False, False, False, True, False, True]
    got = canonical_counts(gs, mixed, backend="host").long()
    esu = canonical_counts(gs, small, backend="host").long()
    cols = iter(range(len(small)))
    for j, (q, big) in enumerate(zip(mixed, is_large)):
        if big:
            i = [k for k, g in enumerate(large) if g is q][0]
            assert got[:, j].tolist() == want[:, i].tolist(), j
        else:
            assert got[:, j].tolist() == esu[:, next(cols)].tolist(), j
    assert got.sum() > 1000


def test_workload_compute_groundtruth_with_large_queries(tmp_path):
    from desco_amd.workload import Workload
    graphs = V.dense_set()[:2]
    queries = [nx.path_graph(7), nx.cycle_graph(8)]
    want = V.vf2_counts(graphs, queries)
    assert (want.sum(0) > 0).all()
    w = Workload(GraphSet.from_edge_lists(graphs), str(tmp_path))
    assert not w.exist_groundtruth(None, queries)
    t = w.compute_groundtruth(queries=queries)
    assert t.dtype == torch.double and t.long().tolist() == want.tolist()
    assert (tmp_path / "CanonicalCountTruth" / "query_num_2_query_len_sum_15.pt").exists()
    w2 = Workload(GraphSet.from_edge_lists(graphs), str(tmp_path))
    assert w2.exist_groundtruth(None, queries) and torch.equal(w2.load_groundtruth(None, queries), t)


def test_refusals_name_the_limit():
    gs = GraphSet.from_edge_lists([(6, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)])])
    two_parts = nx.disjoint_union(nx.path_graph(4), nx.path_graph(4))
    loop = nx.path_graph(7)
    loop.add_edge(3, 3)
    for bad in (nx.path_graph(17), two_parts, loop):
        with pytest.raises(RuntimeError, match=r"connected and loop-free with 2\.\.16 nodes"):
            canonical_counts_match(gs, [nx.path_graph(7), bad], backend="host")
        with pytest.raises(RuntimeError, match=r"2\.\.16 nodes"):
            canonical_counts(gs, [nx.path_graph(3), bad], backend="host")
    with pytest.raises(RuntimeError, match="bad query edge"):
        canonical_counts_match(gs, [(7, [(0, 1), (1, 7)])], backend="host")
    with pytest.raises(ValueError, match="unknown backend"):
        canonical_counts_match(gs, [nx.path_graph(7)], backend="vf2")
    # the size call reports the same refusal, and a plan of another size is not accepted back
    L = _lib.lib()
    q_nodes, q_ptr = np.array([17], np.int32), np.array([0, 0], np.int32)
    assert L.desco_canonical_match_plan_size(q_nodes.ctypes.data, q_ptr.ctypes.data, None, 1) == -1
    assert b"2..16 nodes" in L.desco_last_error()
    plan = match_plan([nx.path_graph(7)])
    out = np.zeros((6, 1), np.int64)
    rc = L.desco_canonical_counts_match(gs.graph_ptr.ctypes.data, 1, gs.rowptr.ctypes.data, gs.col.ctypes.data,
                                        plan.ctypes.data, len(plan) - 1, 1, 1, out.ctypes.data)
    assert rc == -1 and b"desco_canonical_counts_match" in L.desco_last_error()
    # a 17-node query still has a way out
    assert canonical_counts(gs, [nx.path_graph(17)], backend="vf2").sum() == 0


def test_degenerate_graph_sets_give_zeros():
    queries = [nx.path_graph(7), nx.star_graph(6)]
    for graphs in ([(1, [])], [(9, [])], [(1, []), (1, []), (5, [])]):
        got = canonical_counts_match(GraphSet.from_edge_lists(graphs), queries, backend="host")
        assert got.shape == (sum(n for n, _ in graphs), 2) and got.abs().sum() == 0
    empty = GraphSet.from_edge_lists([])
    assert canonical_counts_match(empty, queries, backend="host").shape == (0, 2)
    one = GraphSet.from_edge_lists([(3, [(0, 1)])])
    assert canonical_counts_match(one, [], backend="host").shape == (3, 0)
    # a two-node query: every edge once, at its larger end
    assert canonical_counts_match(one, [nx.path_graph(2)], backend="host").reshape(-1).tolist() == [0, 1, 0]


def _records(plan):
    assert plan[1] >= 0 and len(plan) == HEAD + REC * plan[1]
    return [plan[HEAD + REC * a: HEAD + REC * (a + 1)] for a in range(plan[1])]


def test_plan_properties_through_the_c_abi():
    queries = list(V.large_queries().values()) + [nx.complete_graph(5), nx.star_graph(15), nx.petersen_graph(),
                                                  nx.path_graph(2), nx.hypercube_graph(4), nx.wheel_graph(9)]
    queries = [nx.convert_node_labels_to_integers(q) for q in queries]
    plan = match_plan(queries)
    assert plan.dtype == np.int32 and plan[0] == len(queries)
    recs = _records(plan)
    assert [int(r[0]) for r in recs] == sorted(int(r[0]) for r in recs)          # sorted by query
    for qi, q in enumerate(queries):
        k = q.number_of_nodes()
        mine = [r for r in recs if r[0] == qi]
        # anchors: exactly one per orbit of Aut(q) -- orbits from networkx, by first images of the automorphisms
        # (listing them all is out of reach for K1,15 and the 4-cube: degree and distance profiles separate theirs)
        if k <= 10:
            orbit = {v: {v} for v in q}
            for auto in V.GM(q, q).isomorphisms_iter():
                for a, b in auto.items():
                    orbit[a].add(b)
            orbits = {frozenset(o) for o in orbit.values()}
        else:
            dist = dict(nx.all_pairs_shortest_path_length(q))
            key = {v: (q.degree(v), tuple(sorted(dist[v].values()))) for v in q}
            orbits = {frozenset(u for u in q if key[u] == key[v]) for v in q}
            if k == 12 or k == 14:
                assert len(orbits) == k // 2                                     # a path: mirror pairs
        anchors = [int(r[2]) for r in mine]
        assert len(anchors) == len(orbits), (qi, anchors)
        assert {o for o in orbits if any(a in o for a in anchors)} == orbits
        assert all(a == min(o) for a in anchors for o in orbits if a in o)
        for r in mine:
            assert r[1] == k and r[3] == 1 and r[NODE] == r[2]
            order = [int(x) for x in r[NODE:NODE + k]]
            assert sorted(order) == list(range(k))
            for i in range(1, k):
                adj = {j for j in range(i) if q.has_edge(order[i], order[j])}
                assert adj, (qi, order)                                          # connected matching order
                assert int(r[ADJ + i]) == sum(1 << j for j in adj)
                assert int(r[PARENT + i]) in adj
                assert int(r[LT + i]) >> i == 0 and int(r[GT + i]) >> i == 0 and not int(r[LT + i]) & int(r[GT + i])
            assert r[LT + 1] == 0 and r[GT + 1] == 0                             # the anchor is never ordered


def test_symmetry_breaking_leaves_one_map_per_subset():
    """A star's 720 automorphisms are not enumerated: the leaves of K1,6 are totally ordered, and in K_15 on 16 nodes
    the matcher finds the 16 subsets without walking 15! maps."""
    plan = match_plan([nx.star_graph(6)])
    recs = _records(plan)
    assert len(recs) == 2                                                        # centre, leaf
    for r in recs:
        order = [int(x) for x in r[NODE:NODE + 7]]
        leaves = [i for i in range(1, 7) if order[i] != 0]
        chained = sum(bin(int(r[LT + i]) | int(r[GT + i])).count("1") for i in leaves)
        assert chained == len(leaves) * (len(leaves) - 1) // 2
    k16 = [(16, [(a, b) for a in range(16) for b in range(a + 1, 16)])]
    got = canonical_counts_match(GraphSet.from_edge_lists(k16), [nx.complete_graph(15), nx.complete_graph(16)],
                                 backend="host").long()
    assert got[:, 0].tolist() == [0] * 14 + [1, 15] and got[:, 1].tolist() == [0] * 15 + [1]
