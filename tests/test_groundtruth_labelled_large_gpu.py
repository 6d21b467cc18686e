"""Exact LABELLED ground truth for queries of 7..16 nodes on the MI355X: the labelled instantiation of the device
matcher (csrc/groundtruth_match_dev.hip) against the host labelled matcher and networkx VF2 with node_match run as
the reference runs it (groundtruth_labelled_vf2.py).  Integers, bit-exact.  Every case is sized so that VF2 or the
host matcher finishes it in seconds."""
import networkx as nx
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import groundtruth_labelled_vf2 as LV  # noqa: E402
import groundtruth_vf2 as V  # noqa: E402
from desco_amd import groundtruth as GT  # noqa: E402
from desco_amd import synthetic  # noqa: E402
from desco_amd.graphs import GraphSet  # noqa: E402
from desco_amd.groundtruth import (canonical_counts_labelled, canonical_counts_match_device,  # noqa: E402
                                   canonical_counts_match_labelled, canonical_counts_match_labelled_device,
                                   match_plan_labelled)
from test_groundtruth_large_gpu import hub_graph  # noqa: E402


def graph_set(graphs, labels, F):
    return GraphSet.from_edge_lists(graphs, node_feat=LV.features(labels, F))


def from_occurrence(graph, labels, q, F):
    """q labelled from its first unlabelled VF2 match in `graph` (n, edges)"""
    vmap = next(V.GM(V.to_nx(*graph), q).subgraph_isomorphisms_iter())
    return LV.labelled(q, {qv: labels[tv] for tv, qv in vmap.items()}, F)


@pytest.mark.parametrize("F", [2, 3])
@pytest.mark.parametrize("which", ["sparse", "dense"])
def test_device_equals_host_equals_labelled_vf2(which, F):
    LV.check_nonzero(F)
    graphs, labels, queries, want = LV.yardstick(which, F)
    gs = graph_set(graphs, labels, F)
    dev = canonical_counts_match_labelled_device(gs, queries)
    assert dev.dtype == torch.int64 and dev.is_cuda and dev.shape == want.shape
    assert dev.cpu().tolist() == want.tolist()
    assert canonical_counts_match_labelled(gs, queries, backend="host").long().tolist() == want.tolist()
    # the public entry on this box: columns above 6 nodes to the device matcher, the labelled C6 columns to ESU
    assert canonical_counts_labelled(gs, queries).long().tolist() == want.tolist()
    assert GT.last_labelled_match_backend == "device"
    large_only = [q for q in queries if len(q) > 6]
    canonical_counts_labelled(gs, large_only)
    assert GT.last_labelled_backend == "device"


def test_full_expansion_of_a_seven_node_query_on_the_device():
    graphs = V.dense_set()
    labels = LV.seeded_labels(graphs, 2)
    qs = LV.expansion(V.triangle_bridge_ring(), 2)
    want = LV.vf2_counts_labelled(graphs, labels, 2, qs)
    assert want.shape[1] == 128 and (want.sum(0) > 0).sum() == 57 and want.sum() == 175
    dev = canonical_counts_match_labelled_device(graph_set(graphs, labels, 2), qs)
    assert dev.cpu().tolist() == want.tolist()


def test_device_equals_host_on_a_labelled_hub_graph():
    graph = hub_graph()
    labels = LV.seeded_labels([graph], 2)
    gs = graph_set([graph], labels, 2)
    assert np.diff(gs.rowptr).max() >= 30
    plain = [nx.path_graph(7), nx.star_graph(6), nx.balanced_tree(2, 2)]
    queries = [from_occurrence(graph, labels[0], q, 2) for q in plain] + [LV.labelled(q, [0] * 7, 2) for q in plain]
    host = canonical_counts_match_labelled(gs, queries, backend="host", num_threads=16).long()
    assert (host.sum(0) > 0).all() and host.sum() > 10000
    dev = canonical_counts_match_labelled_device(gs, queries).cpu()
    assert dev.tolist() == host.tolist()


def test_device_equals_host_on_cox2_and_the_classes_sum_to_the_unlabelled_counts():
    plain = synthetic.WORKLOADS["cox2"]().subset(0, 64)
    graphs = plain.edge_lists()
    gs = graph_set(graphs, LV.seeded_labels(graphs, 2), 2)
    p7, c8 = nx.path_graph(7), nx.cycle_graph(8)
    queries = LV.expansion(p7, 2) + LV.expansion(c8, 2)
    plan, coq = match_plan_labelled(queries)
    assert len(queries) == 384 and plan[0] == 102
    host = canonical_counts_match_labelled(gs, queries, backend="host", num_threads=16).long()
    dev = canonical_counts_match_labelled_device(gs, queries)
    assert host.sum() > 0 and dev.cpu().tolist() == host.tolist()
    unl = canonical_counts_match_device(plain, [p7, c8]).cpu()
    assert (unl.sum(0) > 0).all()
    firsts = [coq.tolist().index(c) for c in range(102)]
    for col, block in ((0, range(0, 128)), (1, range(128, 384))):
        mine = [i for i in firsts if i in block]
        assert dev[:, mine].sum(dim=1).cpu().tolist() == unl[:, col].tolist()


def test_bitset_word_boundaries():
    """Graphs of 1, 2, 63, 64, 65 and 129 nodes, built as test_groundtruth_large_gpu.test_bitset_word_boundaries
    builds them, labelled: rows of one, two and three 64-bit words, in one set."""
    rng = np.random.default_rng(9)
    graphs = []
    for n in (1, 2, 63, 64, 65, 129):
        edges = {(int(rng.integers(0, i)), i) for i in range(1, n)}
        edges |= {(a, b) for a in range(n) for b in range(a + 1, n) if rng.random() < 2.0 / max(n, 1)}
        if n > 2:
            edges |= {(0, n - 1), (n - 2, n - 1), (min(62, n - 3), n - 1)}        # the last bit of the last word is used
        graphs.append((n, sorted(edges)))
    labels = LV.seeded_labels(graphs, 2)
    gs = graph_set(graphs, labels, 2)
    plain = [nx.path_graph(7), nx.cycle_graph(7), nx.balanced_tree(2, 2), nx.path_graph(2), nx.path_graph(3),
             V.triangle_bridge_ring()]
    queries = [from_occurrence(graphs[-1], labels[-1], q, 2) for q in plain]
    queries += [LV.labelled(q, [1] * len(q), 2) for q in plain]
    host = canonical_counts_match_labelled(gs, queries, backend="host").long()
    dev = canonical_counts_match_labelled_device(gs, queries).cpu()
    # (the all-1 forms are rarer: a few of them occur, every occurrence-labelled query does)
    assert (host[:, :6].sum(0) > 0).all() and (host[:, 6:].sum(0) > 0).sum() >= 4 and host[-129:].sum() > 1000
    assert dev.tolist() == host.tolist()


def test_two_launches_are_bit_identical_and_slicing_does_not_change_the_result():
    graphs = V.dense_set() + V.sparse_set()[:4]
    labels = LV.seeded_labels(graphs, 2)
    gs = graph_set(graphs, labels, 2)
    queries = LV.yardstick("dense", 2)[2] + LV.expansion(nx.path_graph(7), 2)[:40]
    plan, _ = match_plan_labelled(queries)
    buckets = plan[4 + 100 * int(plan[1]):].reshape(-1, 4)
    sizes = sorted({int(b[3] - b[2]) for b in buckets})
    assert len(buckets) >= 2 and len(sizes) >= 2, sizes               # label buckets of different sizes
    E = int(gs.col.shape[0])
    one = canonical_counts_match_labelled_device(gs, queries, slice_entries=E)
    again = canonical_counts_match_labelled_device(gs, queries, slice_entries=E)
    assert one.sum() > 100 and torch.equal(one, again)
    for slice_entries in (150, 97, 7):
        assert E > 3 * slice_entries
        cut = canonical_counts_match_labelled_device(gs, queries, slice_entries=slice_entries)
        assert torch.equal(cut, one), slice_entries
    assert torch.equal(canonical_counts_match_labelled(gs, queries, backend="device", slice_entries=50).long(), one.cpu())
    assert one.cpu().tolist() == canonical_counts_match_labelled(gs, queries, backend="host").long().tolist()
    assert torch.equal(canonical_counts_match_labelled_device(gs, queries), one)          # the default slicing


def test_auto_picks_the_device_and_the_host_above_the_bitset_limit(monkeypatch):
    graphs, labels, queries, want = LV.yardstick("dense", 2)
    gs = graph_set(graphs, labels, 2)
    queries = [q for q in queries if len(q) > 6]
    host = canonical_counts_match_labelled(gs, queries, backend="host")
    assert GT.last_labelled_match_backend == "host" and host.sum() > 0
    assert torch.equal(canonical_counts_match_labelled(gs, queries, backend="auto"), host)
    assert GT.last_labelled_match_backend == "device"
    monkeypatch.setattr(GT, "_DEVICE_BITSET_LIMIT_WORDS", 10)
    assert torch.equal(canonical_counts_match_labelled(gs, queries, backend="auto"), host)
    assert GT.last_labelled_match_backend == "host"
    assert torch.equal(canonical_counts_labelled(gs, queries), host)                      # routed the same way
    assert GT.last_labelled_match_backend == "host" == GT.last_labelled_backend


def test_degenerate_sets_and_refusals_on_the_device():
    eye = np.eye(2, dtype=np.float32)
    q7 = LV.labelled(nx.path_graph(7), [0, 1, 0, 0, 1, 1, 0], 2)
    queries = [q7, LV.labelled(nx.star_graph(6), [1] * 7, 2)]
    for g, feats in (([(1, [])], [eye[[0]]]), ([(9, [])], [eye[[0] * 9]]),
                     ([(1, []), (2, [(0, 1)])], [eye[[1]], eye[[0, 1]]])):
        got = canonical_counts_match_labelled_device(GraphSet.from_edge_lists(g, node_feat=feats), queries)
        assert got.shape == (sum(n for n, _ in g), 2) and got.sum() == 0
    empty = GraphSet.from_edge_lists([], node_feat=np.zeros((0, 2), dtype=np.float32))
    assert canonical_counts_match_labelled_device(empty, queries).shape == (0, 2)
    path = [(6, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)])]
    gs = GraphSet.from_edge_lists(path, node_feat=[eye[[0, 1, 0, 0, 1, 1]]])
    assert canonical_counts_match_labelled_device(gs, []).shape == (6, 0)
    with pytest.raises(RuntimeError, match=r"2\.\.16 nodes"):
        canonical_counts_match_labelled_device(gs, [LV.labelled(nx.path_graph(17), [0] * 17, 2)])
    with pytest.raises(RuntimeError, match=r"2\.\.16 nodes"):
        canonical_counts_labelled(gs, [LV.labelled(nx.path_graph(17), [0] * 17, 2)], backend="device")
    # a 6-node labelled query is still outside the ESU device path
    with pytest.raises(RuntimeError, match=r"2\.\.5 nodes"):
        canonical_counts_labelled(gs, [LV.labelled(nx.path_graph(6), [0, 1, 0, 0, 1, 1], 2), q7], backend="device")
    # the matcher itself takes small queries: the labelled path once, at node 5; a query label nobody carries: zero
    small = [LV.labelled(nx.path_graph(6), [0, 1, 0, 0, 1, 1], 2), LV.labelled(nx.path_graph(2), [0, 1], 2),
             LV.labelled(nx.path_graph(2), [0, 0], 2)]
    absent = q7.copy()
    absent.nodes[0]["feat"] = [0.0, 0.0]
    got = canonical_counts_match_labelled_device(gs, small + [absent]).cpu()
    assert got.sum(0).tolist() == [1, 3, 1, 0] and got[5, 0] == 1
