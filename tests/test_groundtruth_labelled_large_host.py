"""Exact LABELLED ground truth for queries of 7..16 nodes on the host: the labelled pattern-guided matcher
(csrc/groundtruth_match.cpp) against networkx VF2 with node_match run as the reference runs it
(groundtruth_labelled_vf2.py), the unlabelled matcher and the labelled ESU enumerator.  Integers, bit-exact."""
import ctypes
import os

import networkx as nx
import numpy as np
import pytest
import torch

import groundtruth_labelled_vf2 as LV
import groundtruth_vf2 as V
import test_groundtruth_labelled_host as H
from desco_amd import _lib
from desco_amd import groundtruth as GT
from desco_amd.graphs import GraphSet
from desco_amd.groundtruth import (canonical_counts_labelled, canonical_counts_match, canonical_counts_match_labelled,
                                   match_plan, match_plan_labelled)

HEAD, REC, NODE, PARENT, ADJ, LT, GT_, LABEL, BUCKET = 4, 100, 4, 20, 36, 52, 68, 84, 4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def graph_set(graphs, labels, F):
    return GraphSet.from_edge_lists(graphs, node_feat=LV.features(labels, F))


def records(plan):
    C, A, B = int(plan[0]), int(plan[1]), int(plan[2])
    assert len(plan) == HEAD + A * REC + B * BUCKET
    return plan[HEAD:HEAD + A * REC].reshape(A, REC), plan[HEAD + A * REC:].reshape(B, BUCKET)


def nm(a, b):
    return a["feat"] == b["feat"]


@pytest.mark.parametrize("F", [2, 3])
@pytest.mark.parametrize("which", ["sparse", "dense"])
def test_host_matcher_equals_labelled_vf2(which, F):
    """Fails on the parent commit: backend="host" refuses labelled queries above 6 nodes there."""
    LV.check_nonzero(F)
    graphs, labels, queries, want = LV.yardstick(which, F)
    gs = graph_set(graphs, labels, F)
    got = canonical_counts_match_labelled(gs, queries, backend="host")
    assert GT.last_labelled_match_backend == "host"
    assert got.dtype == torch.double and got.device.type == "cpu" and got.shape == want.shape
    assert got.long().tolist() == want.tolist()
    # the public entry: columns above 6 nodes to the matcher, the labelled C6 columns to ESU, joined in query order
    assert canonical_counts_labelled(gs, queries, backend="host").long().tolist() == want.tolist()
    assert GT.last_labelled_backend == "host"
    assert canonical_counts_labelled(gs, queries, backend="auto").long().tolist() == want.tolist()
    assert GT.last_labelled_backend in ("host", "device")
    large_only = [q for q in queries if len(q) > 6]
    canonical_counts_labelled(gs, large_only, backend="host")
    assert GT.last_labelled_backend == "host" == GT.last_labelled_match_backend


def test_full_expansion_of_a_seven_node_query():
    graphs = V.dense_set()
    labels = LV.seeded_labels(graphs, 2)
    gs = graph_set(graphs, labels, 2)
    qs = LV.expansion(V.triangle_bridge_ring(), 2)
    want = LV.vf2_counts_labelled(graphs, labels, 2, qs)
    assert want.shape[1] == 128 and (want.sum(0) > 0).sum() == 57 and want.sum() == 175
    got = canonical_counts_match_labelled(gs, qs, backend="host").long()
    assert got.tolist() == want.tolist()
    plan, coq = match_plan_labelled(qs)
    assert plan[0] == 72 and len(set(coq.tolist())) == 72
    for i in range(128):                                                 # duplicate columns are equal
        first = coq.tolist().index(coq[i])
        assert got[:, i].tolist() == got[:, first].tolist()


@pytest.mark.parametrize("name,want", [("P7", 72), ("C8", 30), ("K1,6", 14)])
def test_class_counts_of_the_expansions(name, want):
    """Recomputed here with networkx: two copies share a class iff is_isomorphic with node_match says so."""
    qs = LV.expansion(V.large_queries()[name], 2)
    plan, coq = match_plan_labelled(qs)
    ones = [sum(int(q.nodes[v]["feat"][1]) for v in q) for q in qs]
    reps = []                                                            # the first copy of every networkx class
    mine = []
    for i, q in enumerate(qs):
        c = next((j for j, r in enumerate(reps) if ones[r] == ones[i] and nx.is_isomorphic(qs[r], q, node_match=nm)),
                 None)
        if c is None:
            c = len(reps)
            reps.append(i)
        mine.append(c)
    assert len(reps) == want == plan[0]
    assert coq.tolist() == mine                                          # numbered in the order of their first query


@pytest.mark.parametrize("which,name,total", [("sparse", "P7", 1398), ("dense", "C8", 35)])
def test_every_occurrence_carries_exactly_one_labelling(which, name, total):
    """Sum over one column per labelled class of the F = 2 expansion == the unlabelled count, node by node."""
    graphs, names, _, unl = V.yardstick(which)
    labels = LV.seeded_labels(graphs, 2)
    gs = graph_set(graphs, labels, 2)
    q = V.large_queries()[name]
    qs = LV.expansion(q, 2)
    got = canonical_counts_match_labelled(gs, qs, backend="host").long()
    _, coq = match_plan_labelled(qs)
    firsts = [coq.tolist().index(c) for c in range(int(coq.max()) + 1)]
    per_node = got[:, firsts].sum(dim=1)
    assert per_node.tolist() == unl[:, names.index(name)].tolist() and int(per_node.sum()) == total
    assert per_node.tolist() == canonical_counts_match(gs, [q], backend="host").long()[:, 0].tolist()


def test_all_equal_labels_reproduce_the_unlabelled_plan_and_counts():
    graphs, _, queries, want = V.yardstick("dense")
    queries = [nx.convert_node_labels_to_integers(q) for q in queries]
    unl = match_plan(queries)
    unl_recs = unl[2:].reshape(-1, 84)
    for label in (0, 1):
        qs = [LV.labelled(q, [label] * len(q), 2) for q in queries]
        plan, coq = match_plan_labelled(qs)
        recs, buckets = records(plan)
        assert coq.tolist() == list(range(len(queries))) and plan[0] == len(queries)
        assert recs[:, :LABEL].tolist() == unl_recs.tolist()             # anchors, orders and LT / GT constraints
        assert all((r[LABEL:LABEL + r[1]] == 0).all() for r in recs)     # (the queries' only label has id 0)
        assert buckets.tolist() == [[0, 0, 0, len(recs)]] and plan[3] == len(recs)
        gs = graph_set(graphs, [np.full(n, label) for n, _ in graphs], 2)
        assert canonical_counts_match_labelled(gs, qs, backend="host").long().tolist() == want.tolist()
    # and on nodes of the other label nothing matches
    assert canonical_counts_match_labelled(graph_set(graphs, [np.zeros(n, int) for n, _ in graphs], 2), qs,
                                           backend="host").sum() == 0


def test_an_asymmetric_labelling_has_one_anchor_per_node_and_no_order_constraints():
    plan, _ = match_plan_labelled([LV.labelled(nx.path_graph(7), [0, 1, 0, 0, 1, 1, 0], 2)])
    recs, buckets = records(plan)
    assert plan[0] == 1 and len(recs) == 7 and sorted(int(r[2]) for r in recs) == list(range(7))
    assert (recs[:, LT:LT + 16] == 0).all() and (recs[:, GT_:GT_ + 16] == 0).all()
    assert (recs[:, 3] == 1).all()
    keys = [(int(r[LABEL]), int(r[LABEL + 1])) for r in recs]
    assert keys == sorted(keys)                                          # sorted by the labels of positions 0 and 1
    assert [(int(b[0]), int(b[1])) for b in buckets] == sorted(set(keys))
    assert all(keys[b[2]:b[3]] == [(b[0], b[1])] * (b[3] - b[2]) for b in buckets.tolist())
    assert plan[3] == max(b[3] - b[2] for b in buckets.tolist())
    # a palindromic labelling keeps the mirror: 4 anchors, and the mirror is broken once for the middle anchor
    plan, _ = match_plan_labelled([LV.labelled(nx.path_graph(7), [0, 1, 0, 1, 0, 1, 0], 2)])
    recs, _ = records(plan)
    assert sorted(int(r[2]) for r in recs) == [0, 1, 2, 3]
    assert [int((r[LT:LT + 16] != 0).sum() + (r[GT_:GT_ + 16] != 0).sum()) for r in recs if r[2] == 3] == [1]


def test_small_atlas_expansions_equal_the_labelled_esu_path():
    gs, qs, num_q, _, _ = H.table_case("golden8_f2")
    assert len(qs) == num_q == 80
    esu = canonical_counts_labelled(gs, qs, backend="host")
    assert GT.last_labelled_backend == "host" and esu.sum() > 0
    got = canonical_counts_match_labelled(gs, qs, backend="host")
    assert torch.equal(got, esu)


def test_routing_of_a_mixed_labelled_query_set():
    graphs, labels, queries, want = LV.yardstick("dense", 2)
    gs = graph_set(graphs, labels, 2)
    by_size = {len(q): i for i, q in enumerate(queries)}
    p3 = LV.labelled(nx.path_graph(3), [0, 1, 1], 2)
    mixed = [p3, queries[by_size[6]], queries[by_size[7]], queries[by_size[10]], queries[by_size[9]], p3]
    ref = LV.vf2_counts_labelled(graphs, labels, 2, [p3])
    want = np.concatenate([ref, want[:, [by_size[k] for k in (6, 7, 10, 9)]], ref], axis=1)
    assert (want.sum(0) > 0).all()
    for backend in ("host", "auto"):
        assert canonical_counts_labelled(gs, mixed, backend=backend).long().tolist() == want.tolist()
    assert canonical_counts_labelled(gs, mixed, backend="vf2").long().tolist() == want.tolist()


def test_edge_cases():
    graphs, labels, queries, want = LV.yardstick("dense", 2)
    gs = graph_set(graphs, labels, 2)
    q7 = [q for q in queries if len(q) == 7][0]
    absent = q7.copy()
    absent.nodes[3]["feat"] = [0.0, 0.0]                                 # a label no node of the dataset carries
    other_length = q7.copy()
    other_length.nodes[0]["feat"] = [1.0]
    got = canonical_counts_match_labelled(gs, [q7, absent, other_length], backend="host")
    assert got[:, 0].sum() > 0 and got[:, 1].sum() == 0 and got[:, 2].sum() == 0
    assert torch.equal(canonical_counts_labelled(gs, [q7, absent], backend="host"), got[:, :2])
    # degenerate graph sets
    qs = [q7, LV.labelled(nx.star_graph(6), [1] * 7, 2)]
    eye = np.eye(2, dtype=np.float32)
    for g, feats in (([(1, [])], [eye[[0]]]), ([(9, [])], [eye[[0] * 9]]),
                     ([(1, []), (1, []), (5, [])], [eye[[0]], eye[[1]], eye[[0, 1, 0, 1, 1]]])):
        for fn in (canonical_counts_match_labelled, canonical_counts_labelled):
            got = fn(GraphSet.from_edge_lists(g, node_feat=feats), qs, backend="host")
            assert got.shape == (sum(n for n, _ in g), 2) and got.abs().sum() == 0
    empty = GraphSet.from_edge_lists([], node_feat=np.zeros((0, 2), dtype=np.float32))
    assert canonical_counts_match_labelled(empty, qs, backend="host").shape == (0, 2)
    assert canonical_counts_labelled(empty, qs, backend="host").shape == (0, 2)
    assert canonical_counts_match_labelled(gs, [], backend="host").shape == (gs.num_nodes, 0)
    # a labelled two-node query: every edge with those labels once, at its larger end
    one = GraphSet.from_edge_lists([(3, [(0, 1), (1, 2)])], node_feat=[eye[[0, 1, 1]]])
    q2 = [LV.labelled(nx.path_graph(2), [0, 1], 2), LV.labelled(nx.path_graph(2), [1, 1], 2)]
    assert canonical_counts_match_labelled(one, q2, backend="host").long().tolist() == [[0, 0], [1, 0], [0, 1]]
    with pytest.raises(ValueError, match="unknown backend"):
        canonical_counts_match_labelled(gs, [q7], backend="vf2")


def test_nan_goes_to_vf2_and_seventeen_nodes_are_refused_or_go_to_vf2():
    graphs = V.dense_set()[:1]
    labels = LV.seeded_labels(graphs, 2)
    feats = LV.features(labels, 2)
    q7 = LV.occurrence_queries(graphs, labels, 2, [nx.path_graph(7)], V.vf2_counts(graphs, [nx.path_graph(7)]))[0]
    p17 = LV.labelled(nx.path_graph(17), [0] * 17, 2)
    gs = GraphSet.from_edge_lists(graphs, node_feat=feats)
    for backend in ("host", "device"):
        with pytest.raises(RuntimeError, match=r"2\.\.16 nodes"):
            canonical_counts_labelled(gs, [q7, p17], backend=backend)
    with pytest.raises(RuntimeError, match=r"2\.\.16 nodes"):
        canonical_counts_match_labelled(gs, [q7, p17], backend="host")
    got = canonical_counts_labelled(gs, [q7, p17], backend="auto")
    assert GT.last_labelled_backend == "vf2" and got[:, 0].sum() > 0 and got[:, 1].sum() == 0
    assert got[:, 0].tolist() == canonical_counts_labelled(gs, [q7], backend="host")[:, 0].tolist()
    feats[0][1, 0] = np.nan
    nan_gs = GraphSet.from_edge_lists(graphs, node_feat=feats)
    got = canonical_counts_labelled(nan_gs, [q7])
    assert GT.last_labelled_backend == "vf2"
    assert torch.equal(got, canonical_counts_labelled(nan_gs, [q7], backend="vf2"))
    with pytest.raises(RuntimeError, match="NaN"):
        canonical_counts_labelled(nan_gs, [q7], backend="host")
    with pytest.raises(RuntimeError, match="NaN"):
        canonical_counts_match_labelled(nan_gs, [q7], backend="host")


def test_unlabelled_plan_is_unchanged():
    """The unlabelled plan of the ten large queries, byte for byte as the commit before the labelled matcher made it."""
    recorded = np.load(os.path.join(GOLDEN, "match_plan_large_queries.npy"))
    plan = match_plan(list(V.large_queries().values()))
    assert plan.dtype == recorded.dtype == np.int32 and plan.tobytes() == recorded.tobytes()


# ---- C-ABI argument checks: every call differs from a valid one in exactly one way ---------------------------------------
class _Valid:
    """A valid call of each host entry point: a triangle with a tail, a labelled path of 3 and a labelled edge."""

    def __init__(self):
        gs = GraphSet.from_edge_lists([(4, [(0, 1), (1, 2), (0, 2), (2, 3)])])
        self.graph_ptr, self.rowptr, self.col = gs.graph_ptr, gs.rowptr, gs.col
        self.labels = np.array([0, 1, 1, 0], dtype=np.int32)
        self.q_nodes = np.array([3, 2, 2], dtype=np.int32)
        self.q_edge_ptr = np.array([0, 2, 3, 4], dtype=np.int32)
        self.q_edges = np.array([0, 1, 1, 2, 0, 1, 0, 1], dtype=np.int32)
        self.q_labels = np.array([0, 1, 1, 1, 0, 0, 1], dtype=np.int32)
        self.coq = np.full(3, -7, dtype=np.int32)
        self.c = ctypes.c_int(-1)
        L = _lib.lib()
        self.entries = L.desco_canonical_match_plan_labelled_size(*self.qargs().values())
        assert self.entries > 0, L.desco_last_error()
        self.plan = np.zeros(self.entries, dtype=np.int32)
        self.out = np.full((4, 2), -1, dtype=np.int64)

    def p(self, name):
        return getattr(self, name).ctypes.data

    def qargs(self):
        return dict(q_nodes=self.p("q_nodes"), q_edge_ptr=self.p("q_edge_ptr"), q_edges=self.p("q_edges"),
                    q_labels=self.p("q_labels"), num_queries=3)

    def size(self, **over):
        a = self.qargs()
        a.update(over)
        return _lib.lib().desco_canonical_match_plan_labelled_size(*a.values())

    def make(self, **over):
        a = dict(self.qargs(), plan=self.p("plan"), plan_entries=self.entries, coq=self.p("coq"),
                 c=ctypes.addressof(self.c))
        a.update(over)
        return _lib.lib().desco_canonical_match_plan_labelled(*a.values())

    def counts(self, **over):
        a = dict(graph_ptr=self.p("graph_ptr"), num_graphs=1, rowptr=self.p("rowptr"), col=self.p("col"),
                 labels=self.p("labels"), plan=self.p("plan"), plan_entries=self.entries, num_classes=2, num_threads=1,
                 out=self.p("out"))
        a.update(over)
        return _lib.lib().desco_canonical_counts_match_labelled(*a.values())


def _arr(*v):
    return np.array(v, dtype=np.int32)


def test_host_entry_points_reject_bad_arguments():
    L = _lib.lib()
    v = _Valid()
    assert v.make() == 0, L.desco_last_error()
    assert v.c.value == 2 and v.coq.tolist() == [0, 1, 1]                # 1 - 0 and 0 - 1 are one class
    assert v.counts() == 0, L.desco_last_error()
    # by hand, as test_groundtruth_labelled_host: the only induced path 0 - 1 - 1 is 3 - 2 - 1, keyed by node 3; the
    # edges with labels {0, 1} are (0,1), (0,2), (2,3), keyed by their larger node
    assert v.out.tolist() == [[0, 0], [0, 1], [0, 1], [1, 1]]
    keep = []

    def bad(**kw):
        out = {}
        for k, a in kw.items():
            keep.append(a)
            out[k] = a.ctypes.data if isinstance(a, np.ndarray) else a
        return out

    def corrupted(index, value):
        plan = v.plan.copy()
        plan[index] = value
        return bad(plan=plan)

    big = _arr(*([17] + [2, 2]))
    q_bad = [dict(q_nodes=None), dict(q_edge_ptr=None), dict(q_edges=None), dict(q_labels=None), dict(num_queries=-1),
             bad(q_nodes=_arr(1, 2, 2)), bad(q_nodes=big), bad(q_labels=_arr(0, 1, 1, 1, 0, 0, -1)),
             bad(q_edges=_arr(0, 1, 1, 3, 0, 1, 0, 1)), bad(q_edges=_arr(0, 1, 1, 1, 0, 1, 0, 1)),      # bad edge, loop
             bad(q_edges=_arr(0, 1, 0, 1, 0, 1, 0, 1))]                                                # disconnected
    rec0, bucket0 = HEAD, HEAD + int(v.plan[1]) * REC
    cases = {
        "desco_canonical_match_plan_labelled_size": (v.size, q_bad),
        "desco_canonical_match_plan_labelled": (v.make, q_bad + [
            dict(plan=None), dict(coq=None), dict(c=None), dict(plan_entries=v.entries - 1),
            dict(plan_entries=v.entries + 1)]),
        "desco_canonical_counts_match_labelled": (v.counts, [
            dict(graph_ptr=None), dict(rowptr=None), dict(labels=None), dict(plan=None), dict(out=None),
            dict(num_graphs=-1), dict(num_classes=-1), dict(num_classes=1), dict(num_classes=3),
            dict(plan_entries=v.entries - 1), dict(plan_entries=v.entries - BUCKET),
            corrupted(0, 3), corrupted(1, int(v.plan[1]) + 1), corrupted(2, int(v.plan[2]) - 1), corrupted(3, 7),
            corrupted(rec0 + 0, 2), corrupted(rec0 + 1, 17), corrupted(rec0 + 1, 1), corrupted(rec0 + 3, 2),
            corrupted(rec0 + PARENT + 1, 1), corrupted(rec0 + ADJ + 1, 0), corrupted(rec0 + LT + 1, 2),
            corrupted(rec0 + GT_ + 1, 4), corrupted(rec0 + LABEL, -1), corrupted(rec0 + LABEL + 1, 5),
            corrupted(bucket0 + 0, 9), corrupted(bucket0 + 2, 1), corrupted(bucket0 + 3, 0)]),
    }
    for name, (call, overs) in cases.items():
        for over in overs:
            L.desco_gemm_f32_multi(5, None, None)                        # (another entry point's message in between)
            assert call(**over) == -1, (name, over)
            assert name.encode() in L.desco_last_error(), (name, over, L.desco_last_error())
    assert b"2..16 nodes" in (v.size(**bad(q_nodes=big)), L.desco_last_error())[1]
    assert b"2..16 nodes" in (v.size(**bad(q_edges=_arr(0, 1, 0, 1, 0, 1, 0, 1))), L.desco_last_error())[1]
    assert b"non-negative" in (v.size(**bad(q_labels=_arr(0, 1, 1, 1, 0, 0, -1))), L.desco_last_error())[1]
    # label ids are any non-negative int32
    wide = bad(q_labels=_arr(2 ** 31 - 1, 7, 7, 7, 2 ** 31 - 1, 2 ** 31 - 1, 7), labels=_arr(2 ** 31 - 1, 7, 7, 2 ** 31 - 1))
    assert v.make(q_labels=wide["q_labels"]) == 0 and v.counts(labels=wide["labels"]) == 0
    assert v.out.tolist() == [[0, 0], [0, 1], [0, 1], [1, 1]]
    # no queries: an empty plan, and counting with it touches nothing
    head = np.full(HEAD, -1, np.int32)
    assert v.size(num_queries=0, q_labels=None, q_edges=None) == HEAD
    assert v.make(num_queries=0, q_labels=None, q_edges=None, coq=None, plan=head.ctypes.data, plan_entries=HEAD) == 0
    assert head.tolist() == [0, 0, 0, 0] and v.c.value == 0
    assert v.counts(plan=head.ctypes.data, plan_entries=HEAD, num_classes=0) == 0


def test_device_entry_point_rejects_bad_arguments_before_any_launch():
    """host memory stands in for device memory: every call must fail its argument check (no launch)"""
    L = _lib.lib()
    name = b"desco_canonical_counts_match_labelled_dev"
    v = _Valid()
    assert v.make() == 0
    buf = np.zeros(4096, np.int64)
    p = buf.ctypes.data

    def call(**over):
        a = dict(graph_ptr=p, num_graphs=1, num_nodes=4, rowptr=p, num_entries=8, col=p, node_graph=p, bit_off=p,
                 bits=p, num_words=4, labels=p, plan_host=v.p("plan"), plan_dev=p, plan_entries=v.entries,
                 num_classes=2, entry_begin=0, entry_end=8, out=p, stream=None)
        a.update(over)
        return L.desco_canonical_counts_match_labelled_dev(*a.values())

    broken = v.plan.copy()
    broken[HEAD + LABEL] = -1
    for over in (dict(graph_ptr=None), dict(rowptr=None), dict(col=None), dict(node_graph=None), dict(bit_off=None),
                 dict(bits=None), dict(labels=None), dict(plan_host=None), dict(plan_dev=None), dict(out=None),
                 dict(num_graphs=-1), dict(num_nodes=-1), dict(num_entries=-1), dict(num_words=-1), dict(num_classes=-1),
                 dict(num_classes=3), dict(plan_entries=v.entries - 1), dict(entry_begin=-1), dict(entry_begin=5, entry_end=4),
                 dict(entry_end=9), dict(plan_host=broken.ctypes.data)):
        L.desco_gemm_f32_multi(5, None, None)
        assert call(**over) == -1, over
        assert name in L.desco_last_error(), (over, L.desco_last_error())
    assert call(num_nodes=0, graph_ptr=None, out=None) == 0              # an empty input is a no-op
    assert call(num_classes=0, plan_host=None, out=None) == 0
