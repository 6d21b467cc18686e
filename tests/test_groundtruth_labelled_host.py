"""Labelled canonical counts (--use_node_feature) on the native host path (csrc/groundtruth_label.cpp) vs the
reference's procedure, networkx VF2 with node_match (``backend="vf2"``) -- integers, bit-exact (torch.equal) -- plus the
lookup-table helper the device kernel classifies with and the argument checks of the new C-ABI entry points."""
import ctypes
import itertools

import networkx as nx
import numpy as np
import pytest
import torch

from desco_amd import _lib, synthetic
from desco_amd import groundtruth as GT
from desco_amd.data import add_node_feat_to_networkx, graph_atlas_plus
from desco_amd.graphs import GraphSet
from desco_amd.groundtruth import canonical_counts, canonical_counts_labelled
from helpers import golden_graphs, standard_queries

ALL = standard_queries()[0]


def with_labels(gs_or_graphs, F):
    """seeded one-hot labels, as tests/test_node_feature.py::_featured_graphs"""
    graphs = gs_or_graphs.edge_lists() if isinstance(gs_or_graphs, GraphSet) else gs_or_graphs
    rng = np.random.default_rng(11)
    feats = [np.eye(F, dtype=np.float32)[rng.integers(F, size=n)] for n, _ in graphs]
    return GraphSet.from_edge_lists(graphs, node_feat=feats)


def expand(query_ids, F):
    eye = np.eye(F).tolist()
    return [g for q in query_ids for g in add_node_feat_to_networkx(graph_atlas_plus(q), eye, "feat")]


def table_case(name):
    if name == "golden8_f2":
        return with_labels(golden_graphs(max_n=30)[:8], 2), expand([6, 7, 13, 14, 15, 16], 2), 80, 712, 51
    if name == "golden4_f2_all":
        return with_labels(golden_graphs(max_n=30)[:4], 2), expand(ALL, 2), 784, 985, 87
    if name == "golden4_f3":
        return with_labels(golden_graphs(max_n=30)[:4], 3), expand([6, 7, 13, 14], 3), 216, 452, 91
    assert name == "cox2_6_f2"
    return with_labels(synthetic.WORKLOADS["cox2"]().subset(0, 6), 2), expand(ALL, 2), 784, 4027, None


TABLE_CASES = ["golden8_f2", "golden4_f2_all", "golden4_f3", "cox2_6_f2"]


def check_against_vf2(name, gs, qs, got_fn):
    ref = canonical_counts_labelled(gs, qs, backend="vf2")
    assert GT.last_labelled_backend == "vf2"
    total, nonzero = int(ref.sum().item()), int((ref.sum(dim=0) > 0).sum())
    print(f"[labelled] {name}: {len(qs)} labelled queries, reference total {total}, {nonzero} non-zero columns")
    got = got_fn()
    assert got.dtype == torch.double and got.device.type == "cpu" and got.shape == ref.shape
    assert torch.equal(got, ref), (got - ref).abs().max()
    return ref, total, nonzero


@pytest.mark.parametrize("name", TABLE_CASES)
def test_host_path_equals_vf2(name):
    gs, qs, num_q, want_total, want_nonzero = table_case(name)
    assert len(qs) == num_q
    ref, total, nonzero = check_against_vf2(name, gs, qs, lambda: canonical_counts_labelled(gs, qs, backend="host"))
    assert GT.last_labelled_backend == "host"
    assert total > 0 and total == want_total
    assert want_nonzero is None or nonzero == want_nonzero


def _labelled(n, edges, feats):
    g = nx.Graph()
    for v in range(n):
        g.add_node(v, feat=feats[v])
    g.add_edges_from(edges)
    return g


def _mixed_feature_set():
    """features that are not one-hot: three distinct rows, one with a negative zero"""
    graphs = golden_graphs(max_n=30)[:5]
    rows = np.array([[0.5, 2.0], [0.0, 1.0], [3.0, -0.0]], dtype=np.float32)
    rng = np.random.default_rng(5)
    return GraphSet.from_edge_lists(graphs, node_feat=[rows[rng.integers(3, size=n)] for n, _ in graphs]), rows


def test_explicit_queries_with_features_outside_the_dataset():
    gs, rows = _mixed_feature_set()
    a, b, c = ([float(x) for x in r] for r in rows)
    c = [3.0, 0.0]                               # equals the dataset's [3.0, -0.0] as floats
    absent = [7.0, 7.0]                          # no node carries it
    qs = [_labelled(2, [(0, 1)], [a, b]), _labelled(3, [(0, 1), (1, 2)], [a, b, c]),
          _labelled(3, [(0, 1), (1, 2), (0, 2)], [c, c, b]), _labelled(4, [(0, 1), (1, 2), (2, 3)], [a, a, b, c]),
          _labelled(3, [(0, 1), (1, 2)], [a, absent, b]), _labelled(4, [(0, 1), (0, 2), (0, 3)], [b, a, c, a]),
          _labelled(2, [(0, 1)], [c, [3.0]])]    # a feature of another length matches nothing
    ref, total, _ = check_against_vf2("explicit", gs, qs, lambda: canonical_counts_labelled(gs, qs, backend="host"))
    assert total > 0 and ref[:, 2].sum() + ref[:, 1].sum() > 0           # the -0.0 row did match
    assert ref[:, 4].sum() == 0 and ref[:, 6].sum() == 0


def test_six_node_labelled_query_on_the_host_path():
    gs = with_labels(golden_graphs(max_n=30)[:4], 2)
    e0, e1 = [1.0, 0.0], [0.0, 1.0]
    path6 = [(i, i + 1) for i in range(5)]
    qs = [_labelled(6, path6, [e0, e1, e0, e0, e1, e0]), _labelled(6, path6, [e0] * 6),
          _labelled(6, path6 + [(5, 0)], [e0, e0, e1, e0, e0, e1]), _labelled(6, [(0, i) for i in range(1, 6)], [e1] + [e0] * 5),
          _labelled(5, [(0, 1), (1, 2), (2, 3), (3, 4)], [e0, e1, e1, e0, e0])]
    _, total, _ = check_against_vf2("six nodes", gs, qs, lambda: canonical_counts_labelled(gs, qs, backend="host"))
    assert total > 0


def test_duplicates_get_equal_columns_and_absent_labels_zero_columns():
    gs = with_labels(golden_graphs(max_n=30)[:4], 2)
    e0, e1, e2 = [1.0, 0.0], [0.0, 1.0], [0.0, 0.0]
    qs = [_labelled(3, [(0, 1), (1, 2)], [e0, e1, e1]), _labelled(3, [(0, 1), (1, 2)], [e1, e1, e0]),     # a-b-b, b-b-a
          _labelled(3, [(2, 0), (0, 1)], [e1, e1, e0]),                                                     # the same, renumbered
          _labelled(3, [(0, 1), (1, 2)], [e0, e2, e1]), _labelled(2, [(0, 1)], [e0, e1])]
    ref, total, _ = check_against_vf2("duplicates", gs, qs, lambda: canonical_counts_labelled(gs, qs, backend="host"))
    got = canonical_counts_labelled(gs, qs, backend="host")
    assert total > 0 and got[:, 0].sum() > 0
    assert torch.equal(got[:, 0], got[:, 1]) and torch.equal(got[:, 0], got[:, 2])
    assert got[:, 3].sum() == 0


def test_degenerate_graph_sets():
    qs = expand([6, 7], 2) + [_labelled(2, [(0, 1)], [[1.0, 0.0], [0.0, 1.0]])]
    single = GraphSet.from_edge_lists([(1, [])], node_feat=[np.eye(2, dtype=np.float32)[[0]]])
    no_edges = GraphSet.from_edge_lists([(4, [])], node_feat=[np.eye(2, dtype=np.float32)[[0, 1, 1, 0]]])
    mixed = GraphSet.from_edge_lists([(1, []), (3, [(0, 1), (1, 2)]), (2, [])],
                                     node_feat=[np.eye(2, dtype=np.float32)[[0]], np.eye(2, dtype=np.float32)[[0, 1, 0]],
                                                np.eye(2, dtype=np.float32)[[1, 1]]])
    for name, gs, want in (("single node", single, 0), ("no edges", no_edges, 0), ("mixed", mixed, None)):
        for backend in ("host", "auto"):
            got = canonical_counts_labelled(gs, qs, backend=backend)
            ref = canonical_counts_labelled(gs, qs, backend="vf2")
            assert got.shape == (gs.num_nodes, len(qs)) and torch.equal(got, ref), name
            assert want is None or got.sum() == want
    assert canonical_counts_labelled(mixed, qs, backend="vf2").sum() > 0
    empty = GraphSet.from_edge_lists([], node_feat=np.zeros((0, 2), dtype=np.float32))
    for backend in ("host", "auto", "vf2"):
        assert canonical_counts_labelled(empty, qs, backend=backend).shape == (0, len(qs))
        assert canonical_counts_labelled(mixed, [], backend=backend).shape == (mixed.num_nodes, 0)


def test_nan_features_go_to_vf2():
    graphs = golden_graphs(max_n=30)[:2]
    feats = [np.eye(2, dtype=np.float32)[np.arange(n) % 2] for n, _ in graphs]
    feats[0][1, 0] = np.nan
    gs = GraphSet.from_edge_lists(graphs, node_feat=feats)
    qs = expand([6], 2)
    got = canonical_counts_labelled(gs, qs)
    assert GT.last_labelled_backend == "vf2"
    assert torch.equal(got, canonical_counts_labelled(gs, qs, backend="vf2")) and got.sum() > 0
    with pytest.raises(RuntimeError, match="NaN"):
        canonical_counts_labelled(gs, qs, backend="host")
    with pytest.raises(ValueError):
        canonical_counts_labelled(gs, qs, backend="cuda")


def test_workload_uses_the_native_path_and_its_thread_count():
    from desco_amd.workload import Workload
    gs = with_labels(golden_graphs(max_n=30)[:4], 2)
    qids = [6, 7, 13, 14]
    truth = Workload(gs, root=None, node_feat_len=2).compute_groundtruth(qids, num_workers=2)
    assert GT.last_labelled_backend in ("host", "device")
    assert torch.equal(truth, canonical_counts_labelled(gs, expand(qids, 2), backend="vf2")) and truth.sum() > 0


# ---- the lookup helper ------------------------------------------------------------------------------------------------
def _pair_bit(a, b):
    return b * (b - 1) // 2 + a


def _flat(patterns):
    """patterns: (k, mask, labels) -> the C ABI's query arrays"""
    q_nodes = np.array([k for k, _, _ in patterns], dtype=np.int32)
    edges = [[(a, b) for b in range(k) for a in range(b) if m >> _pair_bit(a, b) & 1] for k, m, _ in patterns]
    q_edge_ptr = np.concatenate([[0], np.cumsum([len(e) for e in edges])]).astype(np.int32)
    q_edges = np.array([x for es in edges for e in es for x in e], dtype=np.int32)
    q_labels = np.array([x for _, _, ls in patterns for x in ls], dtype=np.int32)
    return q_nodes, q_edge_ptr, q_edges, q_labels, edges


def _classes(patterns, num_labels):
    q_nodes, q_edge_ptr, q_edges, q_labels, _ = _flat(patterns)
    coq = np.full(len(patterns), -7, dtype=np.int32)
    c, kmax = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = _lib.lib().desco_canonical_label_classes(q_nodes.ctypes.data, q_edge_ptr.ctypes.data, q_edges.ctypes.data,
                                                  q_labels.ctypes.data, len(patterns), num_labels, coq.ctypes.data,
                                                  ctypes.byref(c), ctypes.byref(kmax))
    assert rc == 0, _lib.lib().desco_last_error()
    return coq, c.value, kmax.value


def test_lookup_table_agrees_with_networkx_isomorphism():
    """All connected labelled 3- and 4-node patterns at F = 2 (every mask x every labeling, i.e. every code the kernel
    can form): two codes read the same class from the table iff networkx calls them isomorphic with node_match, and
    class_of_query agrees with the table."""
    A = 2
    patterns, graphs = [], []
    for k in (3, 4):
        for m in range(1 << (k * (k - 1) // 2)):
            g0 = nx.Graph()
            g0.add_nodes_from(range(k))
            g0.add_edges_from((a, b) for b in range(k) for a in range(b) if m >> _pair_bit(a, b) & 1)
            if not nx.is_connected(g0):
                continue
            for labs in itertools.product(range(A), repeat=k):
                g = g0.copy()
                for v in range(k):
                    g.nodes[v]["l"] = labs[v]
                patterns.append((k, m, labs))
                graphs.append(g)
    assert len(patterns) == 4 * 8 + 38 * 16
    coq, C, kmax = _classes(patterns, A)
    assert kmax == 4 and coq.min() == 0 and coq.max() == C - 1 and len(set(coq.tolist())) == C
    L = _lib.lib()
    entries = L.desco_canonical_label_table_size(4, A)
    assert entries == 2 * A ** 2 + 8 * A ** 3 + 64 * A ** 4
    table = np.full(entries, -9, dtype=np.int32)
    q_nodes, q_edge_ptr, q_edges, q_labels, _ = _flat(patterns)
    assert L.desco_canonical_label_table(q_nodes.ctypes.data, q_edge_ptr.ctypes.data, q_edges.ctypes.data,
                                         q_labels.ctypes.data, len(patterns), A, coq.ctypes.data, C, 4,
                                         table.ctypes.data, entries) == 0, L.desco_last_error()
    off = {2: 0, 3: 2 * A ** 2, 4: 2 * A ** 2 + 8 * A ** 3}

    def read(k, m, labs):
        return int(table[off[k] + m * A ** k + sum(l * A ** j for j, l in enumerate(labs))])

    got = [read(*p) for p in patterns]
    assert got == coq.tolist()                                     # the table and class_of_query agree on every code
    nm = lambda a, b: a["l"] == b["l"]                             # noqa: E731
    reps = {}                                                      # class -> its first pattern
    for i, c in enumerate(got):
        # equal class <=> isomorphic, against the first pattern of every class seen so far (an equivalence relation
        # is fixed by that); patterns of different sizes never share a class
        for c2, j in reps.items():
            same = patterns[i][0] == patterns[j][0] and nx.is_isomorphic(graphs[i], graphs[j], node_match=nm)
            assert (c == c2) == same, (patterns[i], patterns[j])
        reps.setdefault(c, i)
    assert len(reps) == C
    # disconnected masks and the 2-node block belong to no query here
    used = {off[k] + m * A ** k + sum(l * A ** j for j, l in enumerate(labs)) for k, m, labs in patterns}
    assert all(table[i] == -1 for i in range(entries) if i not in used)


def test_class_of_query_groups_the_reference_expansion():
    qs = expand(ALL, 2)
    lab = GT._Labelled(with_labels(golden_graphs(max_n=30)[:1], 2), qs, "feat")
    coq = lab.classes()
    assert len(coq) == 784 and lab.num_classes == len(set(coq.tolist())) < 784
    nm = lambda a, b: a["feat"] == b["feat"]                      # noqa: E731
    start = 0
    for qid in ALL:                                                # copies of one query: same class iff isomorphic
        n = 2 ** len(graph_atlas_plus(qid).nodes)
        block = list(range(start, start + n))
        if n <= 16:
            for i, j in itertools.combinations(block, 2):
                assert (coq[i] == coq[j]) == nx.is_isomorphic(qs[i], qs[j], node_match=nm)
        start += n
    # copies of different queries never share a class
    owner = {}
    start = 0
    for qid in ALL:
        n = 2 ** len(graph_atlas_plus(qid).nodes)
        for i in range(start, start + n):
            assert owner.setdefault(int(coq[i]), qid) == qid
        start += n


def test_labelled_counts_sum_to_unlabelled_on_syn_shapes():
    """sum over labelings of count_lab * sym_lab / sym == the unlabelled count, at a size VF2 cannot reach."""
    gs = with_labels(synthetic.WORKLOADS["syn_1827"]().subset(300, 420), 2)
    assert gs.num_graphs == 120 and gs.num_nodes == 3020
    _, queries = standard_queries()
    qs = expand(ALL, 2)
    lab = canonical_counts_labelled(gs, qs, backend="host")
    assert lab.shape == (3020, 784)
    unl = canonical_counts(gs, queries, backend="host")
    nm = lambda a, b: a["feat"] == b["feat"]                      # noqa: E731
    aut = lambda g, **kw: sum(1 for _ in nx.algorithms.isomorphism.GraphMatcher(g, g, **kw)   # noqa: E731
                              .subgraph_isomorphisms_iter())
    start = 0
    for col, qid in enumerate(ALL):
        q = graph_atlas_plus(qid)
        n = 2 ** len(q.nodes)
        sym_lab = torch.tensor([aut(g, node_match=nm) for g in qs[start:start + n]], dtype=torch.double)
        total = (lab[:, start:start + n] * sym_lab).sum(dim=1) / aut(q)
        assert torch.equal(total, unl[:, col].double()), qid
        start += n
    print(f"[labelled] syn identity: labelled total {int(lab.sum())}, unlabelled total {int(unl.sum())}")
    assert unl.sum() > 1000


# ---- C-ABI argument checks: every call differs from a valid one in exactly one way ---------------------------------------
class _Valid:
    """A valid call of each host entry point on one triangle-with-a-tail graph and two labelled queries."""

    def __init__(self):
        gs = GraphSet.from_edge_lists([(4, [(0, 1), (1, 2), (0, 2), (2, 3)])])
        self.graph_ptr, self.rowptr, self.col = gs.graph_ptr, gs.rowptr, gs.col
        self.labels = np.array([0, 1, 1, 0], dtype=np.int32)
        self.q_nodes = np.array([3, 2], dtype=np.int32)
        self.q_edge_ptr = np.array([0, 2, 3], dtype=np.int32)
        self.q_edges = np.array([0, 1, 1, 2, 0, 1], dtype=np.int32)
        self.q_labels = np.array([0, 1, 1, 1, 0], dtype=np.int32)
        self.coq = np.array([0, 1], dtype=np.int32)
        self.out = np.full((4, 2), -1, dtype=np.int64)
        self.table = np.zeros(2 * 4 + 8 * 8, dtype=np.int32)
        self.c, self.kmax = ctypes.c_int(0), ctypes.c_int(0)

    def p(self, name):
        return getattr(self, name).ctypes.data

    def classes(self, **over):
        a = dict(q_nodes=self.p("q_nodes"), q_edge_ptr=self.p("q_edge_ptr"), q_edges=self.p("q_edges"),
                 q_labels=self.p("q_labels"), num_queries=2, num_labels=2, coq=self.p("coq"),
                 c=ctypes.addressof(self.c), kmax=ctypes.addressof(self.kmax))
        a.update(over)
        return _lib.lib().desco_canonical_label_classes(*a.values())

    def table_(self, **over):
        a = dict(q_nodes=self.p("q_nodes"), q_edge_ptr=self.p("q_edge_ptr"), q_edges=self.p("q_edges"),
                 q_labels=self.p("q_labels"), num_queries=2, num_labels=2, coq=self.p("coq"), num_classes=2, kmax=3,
                 table=self.p("table"), entries=len(self.table))
        a.update(over)
        return _lib.lib().desco_canonical_label_table(*a.values())

    def counts(self, **over):
        a = dict(graph_ptr=self.p("graph_ptr"), num_graphs=1, rowptr=self.p("rowptr"), col=self.p("col"),
                 labels=self.p("labels"), num_labels=2, q_nodes=self.p("q_nodes"), q_edge_ptr=self.p("q_edge_ptr"),
                 q_edges=self.p("q_edges"), q_labels=self.p("q_labels"), num_queries=2, coq=self.p("coq"),
                 num_classes=2, num_threads=1, out=self.p("out"))
        a.update(over)
        return _lib.lib().desco_canonical_counts_labelled(*a.values())


def _arr(*v):
    return np.array(v, dtype=np.int32)


def test_host_entry_points_reject_bad_arguments():
    L = _lib.lib()
    v = _Valid()
    assert v.classes() == 0 and v.c.value == 2 and v.kmax.value == 3 and v.coq.tolist() == [0, 1]
    assert v.table_() == 0 and sorted(set(v.table.tolist())) == [-1, 0, 1]
    assert v.counts() == 0, L.desco_last_error()
    # by hand: the edges with labels {0, 1} are (0,1), (0,2), (2,3), keyed by their larger node; the only induced path
    # with labels 0 - 1 - 1 is 3 - 2 - 1 (0 - 2 - 1 closes into the triangle), keyed by node 3
    assert v.out.tolist() == [[0, 0], [0, 1], [0, 1], [1, 1]]
    keep = []                                    # arrays of the cases below stay alive until the calls are done

    def bad(**kw):
        out = {}
        for k, a in kw.items():
            keep.append(a)
            out[k] = a.ctypes.data if isinstance(a, np.ndarray) else a
        return out

    q_bad_edge = bad(q_edges=_arr(0, 1, 1, 3, 0, 1))
    q_loop = bad(q_edges=_arr(0, 1, 1, 1, 0, 1))
    cases = {
        "desco_canonical_label_classes": (v.classes, [
            dict(q_nodes=None), dict(q_edge_ptr=None), dict(q_edges=None), dict(q_labels=None), dict(coq=None),
            dict(c=None), dict(kmax=None), dict(num_queries=-1), dict(num_labels=0), dict(num_labels=257),
            bad(q_nodes=_arr(1, 2)), bad(q_nodes=_arr(7, 2)), bad(q_labels=_arr(0, 1, 2, 1, 0)),
            bad(q_labels=_arr(0, -1, 1, 1, 0)), q_bad_edge, q_loop]),
        "desco_canonical_label_table": (v.table_, [
            dict(q_nodes=None), dict(q_edge_ptr=None), dict(q_edges=None), dict(q_labels=None), dict(coq=None),
            dict(table=None), dict(num_queries=-1), dict(num_labels=0), dict(num_labels=17), dict(kmax=1), dict(kmax=6),
            dict(kmax=2), dict(entries=len(v.table) - 1), dict(num_classes=1), bad(coq=_arr(0, -1)),
            bad(q_nodes=_arr(6, 2)), bad(q_labels=_arr(0, 1, 2, 1, 0)), q_bad_edge, q_loop]),
        "desco_canonical_counts_labelled": (v.counts, [
            dict(graph_ptr=None), dict(rowptr=None), dict(col=None), dict(labels=None), dict(q_nodes=None),
            dict(q_edge_ptr=None), dict(q_edges=None), dict(q_labels=None), dict(coq=None), dict(out=None),
            dict(num_graphs=-1), dict(num_queries=-1), dict(num_labels=0), dict(num_labels=257), dict(num_classes=3),
            dict(num_classes=1), bad(labels=_arr(0, 1, 2, 0)), bad(labels=_arr(0, -1, 1, 0)), bad(coq=_arr(0, 2)),
            bad(q_nodes=_arr(7, 2)), bad(q_nodes=_arr(1, 2)), bad(q_labels=_arr(0, 1, 1, 1, 2)), q_bad_edge, q_loop]),
    }
    for name, (call, overs) in cases.items():
        for over in overs:
            L.desco_gemm_f32_multi(5, None, None)                # (another entry point's message in between)
            assert call(**over) == -1, (name, over)
            assert name.encode() in L.desco_last_error(), (name, over, L.desco_last_error())
    # isomorphic queries (0 - 1 and 1 - 0) in two classes
    iso = bad(q_nodes=_arr(2, 2), q_edge_ptr=_arr(0, 1, 2), q_edges=_arr(0, 1, 0, 1), q_labels=_arr(0, 1, 1, 0))
    assert v.counts(**iso) == -1 and b"desco_canonical_counts_labelled: class_of_query" in L.desco_last_error()
    assert v.table_(kmax=2, entries=8, **iso) == -1 and b"desco_canonical_label_table: class_of_query" in L.desco_last_error()
    same = bad(coq=_arr(0, 0))
    assert v.counts(num_classes=1, **iso, **same) == 0 and v.table_(kmax=2, entries=8, num_classes=1, **iso, **same) == 0
    assert L.desco_canonical_label_table_size(1, 2) == -1 and b"desco_canonical_label_table_size" in L.desco_last_error()
    assert L.desco_canonical_label_table_size(6, 2) == -1 and L.desco_canonical_label_table_size(5, 17) == -1
    assert L.desco_canonical_label_table_size(5, 0) == -1
    assert L.desco_canonical_label_table_size(5, 16) == 2 * 16 ** 2 + 8 * 16 ** 3 + 64 * 16 ** 4 + 1024 * 16 ** 5


def test_device_entry_point_rejects_bad_arguments_before_any_launch():
    """host memory stands in for device memory: every call must fail its argument check (no GPU here)"""
    L = _lib.lib()
    name = b"desco_canonical_counts_labelled_dev"
    buf = np.zeros(4096, np.int64)
    p = buf.ctypes.data
    entries = L.desco_canonical_label_table_size(3, 2)

    def call(**over):
        a = dict(graph_ptr=p, num_graphs=1, num_nodes=4, rowptr=p, num_entries=8, col=p, node_graph=p, bit_off=p,
                 bits=p, num_words=4, labels=p, num_labels=2, table=p, entries=entries, kmax=3, num_classes=2, out=p,
                 stream=None)
        a.update(over)
        return L.desco_canonical_counts_labelled_dev(*a.values())

    for over in (dict(graph_ptr=None), dict(rowptr=None), dict(col=None), dict(node_graph=None), dict(bit_off=None),
                 dict(bits=None), dict(labels=None), dict(table=None), dict(out=None), dict(num_graphs=-1),
                 dict(num_nodes=-1), dict(num_entries=-1), dict(num_words=-1), dict(num_classes=-1), dict(kmax=1),
                 dict(kmax=6), dict(num_labels=0), dict(num_labels=17), dict(entries=entries + 1), dict(entries=0)):
        L.desco_gemm_f32_multi(5, None, None)
        assert call(**over) == -1, over
        assert name in L.desco_last_error(), (over, L.desco_last_error())
    assert b"2..5 nodes" in (call(kmax=6), L.desco_last_error())[1]
    assert b"16 label" in (call(num_labels=17), L.desco_last_error())[1]
    # an empty input is a no-op
    assert call(num_nodes=0, graph_ptr=None, out=None) == 0
    assert call(num_classes=0, table=None, out=None) == 0


def test_empty_inputs_are_no_ops_on_the_host_entry_points():
    v = _Valid()
    zero = np.zeros(1, dtype=np.int64)
    assert v.counts(num_queries=0, num_classes=0, q_nodes=None, q_edge_ptr=None, q_edges=None, q_labels=None, coq=None,
                    out=None) == 0
    assert v.counts(graph_ptr=zero.ctypes.data, num_graphs=0, rowptr=None, col=None, labels=None, out=None) == 0
    assert v.classes(num_queries=0, q_nodes=None, q_edge_ptr=None, q_edges=None, q_labels=None, coq=None) == 0
    assert v.c.value == 0
