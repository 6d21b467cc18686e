"""Labelled canonical counts (--use_node_feature) on the device enumerator (csrc/groundtruth_label_dev.hip) vs the
reference's VF2 procedure (``backend="vf2"``) and vs the native host path, which tests/test_groundtruth_labelled_host.py
pins to VF2 -- integers, bit-exact (torch.equal)."""
import networkx as nx
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from desco_amd import groundtruth as GT  # noqa: E402
from desco_amd import synthetic  # noqa: E402
from desco_amd.data import graph_atlas_plus  # noqa: E402
from desco_amd.graphs import GraphSet  # noqa: E402
from desco_amd.groundtruth import (canonical_counts_device, canonical_counts_labelled,  # noqa: E402
                                   canonical_counts_labelled_device)
from helpers import golden_graphs, standard_queries  # noqa: E402
from test_groundtruth_labelled_host import (ALL, TABLE_CASES, _labelled, check_against_vf2, expand,  # noqa: E402
                                            table_case, with_labels)


@pytest.mark.parametrize("name", TABLE_CASES)
def test_device_path_equals_vf2(name):
    gs, qs, num_q, want_total, want_nonzero = table_case(name)
    assert len(qs) == num_q
    _, total, nonzero = check_against_vf2(name, gs, qs, lambda: canonical_counts_labelled(gs, qs, backend="device"))
    assert GT.last_labelled_backend == "device"
    assert total > 0 and total == want_total
    assert want_nonzero is None or nonzero == want_nonzero


def _shape(case):
    """the graph sets of tests/test_groundtruth_dev_gpu.py::test_device_counts_equal_host_enumerator"""
    if case == "golden":
        return golden_graphs()
    if case == "dense":            # dense random graphs, hubs, an isolated node, a single-node graph
        rng = np.random.default_rng(1)
        graphs = []
        for n, p in [(30, 0.4), (70, 0.15), (1, 0.0), (45, 0.25), (2, 1.0)]:
            e = [(a, b) for a in range(n) for b in range(a + 1, n) if rng.random() < p and b != n - 1]
            graphs.append((n, e))
        return graphs
    if case == "syn":
        return synthetic.WORKLOADS["syn_1827"]().subset(300, 420)
    if case == "cox2":
        return synthetic.WORKLOADS["cox2"]()
    assert case == "cox2_100"
    return synthetic.WORKLOADS["cox2"]().subset(0, 100)


F3_IDS = [6, 7, 13, 14, 15, 16]
CASES = [(c, 2, None) for c in ("golden", "dense", "syn", "cox2")] + \
        [(c, 3, F3_IDS) for c in ("golden", "dense", "syn", "cox2")] + [("cox2_100", 7, [6, 7, 13, 14])]


@pytest.mark.parametrize("case,F,ids", CASES, ids=[f"{c}-F{f}" for c, f, _ in CASES])
def test_device_path_equals_host_path(case, F, ids):
    gs = with_labels(_shape(case), F)
    qs = expand(ALL if ids is None else ids, F)
    assert len(qs) == {2: 784, 3: 378, 7: 5488}[F]
    host = canonical_counts_labelled(gs, qs, backend="host")
    total, nonzero = int(host.sum().item()), int((host.sum(dim=0) > 0).sum())
    print(f"[labelled] {case} F={F}: {gs.num_nodes} nodes, {len(qs)} labelled queries, reference total {total}, "
          f"{nonzero} non-zero columns")
    assert total > 1000
    dev = canonical_counts_labelled_device(gs, qs)
    assert dev.dtype == torch.int64 and dev.is_cuda and dev.shape == host.shape
    assert torch.equal(dev.cpu().double(), host), (dev.cpu().double() - host).abs().max()
    del dev
    auto = canonical_counts_labelled(gs, qs)                      # auto -> device on this box
    assert GT.last_labelled_backend == "device" and torch.equal(auto, host)


@pytest.mark.parametrize("case", ["golden", "syn"])
def test_labelled_device_counts_sum_to_unlabelled_device_counts(case):
    gs = with_labels(_shape(case), 2)
    _, queries = standard_queries()
    qs = expand(ALL, 2)
    lab = canonical_counts_labelled_device(gs, qs).cpu().double()
    unl = canonical_counts_device(gs, queries).cpu()
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
    print(f"[labelled] {case}: labelled total {int(lab.sum())}, unlabelled total {int(unl.sum())}")
    assert unl.sum() > 1000


def test_node_chunks_and_repeated_runs_are_bit_identical(monkeypatch):
    gs = with_labels(_shape("syn"), 2)
    qs = expand(ALL, 2)
    one = canonical_counts_labelled_device(gs, qs)
    assert one.sum() > 1000
    assert torch.equal(one, canonical_counts_labelled_device(gs, qs))              # two runs in a row
    lab = GT._Labelled(gs, qs, "feat")
    lab.classes()
    per_node = 8 * (lab.num_classes + lab.num_queries)
    chunks = list(GT._labelled_device_chunks(gs, lab, torch.device("cuda"), chunk_bytes=per_node * 400))
    assert len(chunks) >= 7 and chunks[0][0] == 0 and chunks[-1][1] == gs.num_nodes
    assert all(a[1] == b[0] for a, b in zip(chunks, chunks[1:])) and all(n1 - n0 <= 400 for n0, n1, _ in chunks)
    assert torch.equal(torch.cat([c for _, _, c in chunks]), one)
    assert torch.equal(canonical_counts_labelled_device(gs, qs, chunk_bytes=per_node * 400), one)
    assert torch.equal(canonical_counts_labelled_device(gs, qs, chunk_bytes=1), one)   # one graph per chunk
    monkeypatch.setattr(GT, "_DEVICE_LABEL_CHUNK_BYTES", per_node * 1000)              # the CPU-returning path too
    assert torch.equal(canonical_counts_labelled(gs, qs, backend="device"), one.cpu().double())


def test_workload_ground_truth_runs_on_the_device():
    from desco_amd.workload import Workload
    from test_node_feature import QIDS, _featured_graphs
    _, _, gs = _featured_graphs()
    GT.last_labelled_backend = None
    truth = Workload(gs, root=None, node_feat_len=2).compute_groundtruth(QIDS)
    assert GT.last_labelled_backend == "device"
    ref = canonical_counts_labelled(gs, expand(QIDS, 2), backend="vf2")
    assert truth.shape == (gs.num_nodes, 80) and torch.equal(truth, ref) and ref.sum() == 712


def _one_hot_set(F):
    """four small graphs with F one-hot labels, and the features of the two ends of its first edge (so that a query
    built from them is certain to occur)"""
    gs = with_labels(golden_graphs(max_n=30)[:4], F)
    a, b = 0, int(gs.col[gs.rowptr[0]])
    return gs, [float(x) for x in gs.node_feat[a]], [float(x) for x in gs.node_feat[b]]


def test_device_limits_and_fallback():
    # 6-node labelled queries
    gs, fa, fb = _one_hot_set(2)
    e0, e1 = [1.0, 0.0], [0.0, 1.0]
    six = [_labelled(6, [(i, i + 1) for i in range(5)], [e0, e1, e0, e0, e1, e0]), _labelled(2, [(0, 1)], [fa, fb])]
    # an alphabet above 16 labels (3-node queries: the table would be small)
    gs20, fa, fb = _one_hot_set(20)
    e = np.eye(20).tolist()
    assert len({tuple(r) for r in gs20.node_feat.tolist()}) > 16
    wide = [_labelled(3, [(0, 1), (1, 2)], [e[0], e[1], e[19]]), _labelled(2, [(0, 1)], [fa, fb]),
            _labelled(2, [(0, 1)], [fb, fa])]
    # a lookup table above its budget: 10 labels and a 5-node query = 1024 * 10^5 entries
    gs10, fa, fb = _one_hot_set(10)
    e10 = np.eye(10).tolist()
    assert len({tuple(r) for r in gs10.node_feat.tolist()}) == 10
    big = [_labelled(5, [(0, 1), (1, 2), (2, 3), (3, 4)], [e10[0], e10[1], e10[2], e10[1], e10[0]]),
           _labelled(2, [(0, 1)], [fa, fb])]
    for name, g, qs, match in (("six nodes", gs, six, "2..5 nodes"), ("alphabet", gs20, wide, "at most 16"),
                               ("table", gs10, big, "budget")):
        with pytest.raises(RuntimeError, match=match):
            canonical_counts_labelled(g, qs, backend="device")
        with pytest.raises(RuntimeError, match=match):
            canonical_counts_labelled_device(g, qs)
        auto = canonical_counts_labelled(g, qs)
        assert GT.last_labelled_backend == "host", name
        assert torch.equal(auto, canonical_counts_labelled(g, qs, backend="host")), name
        assert torch.equal(auto, canonical_counts_labelled(g, qs, backend="vf2")) and auto.sum() > 0, name
    # within the limits: 16 labels, duplicates, and more than 32 queries
    gs16, _, _ = _one_hot_set(16)
    e16 = np.eye(16).tolist()
    many = [_labelled(3, [(0, 1), (1, 2)], [e16[a], e16[b], e16[15 - a]]) for a in range(16) for b in range(4)] + \
           [_labelled(3, [(0, 1), (1, 2)], [e16[15], e16[0], e16[0]]), _labelled(2, [(0, 1)], [e16[15], e16[14]])]
    got = canonical_counts_labelled(gs16, many, backend="device")
    assert len(many) == 66 and torch.equal(got, canonical_counts_labelled(gs16, many, backend="vf2")) and got.sum() > 0
    assert torch.equal(got[:, 0], got[:, 64])                      # 0 - 0 - 15 and 15 - 0 - 0
    empty = GraphSet.from_edge_lists([(3, [])], node_feat=[np.eye(2, dtype=np.float32)[[0, 1, 0]]])
    assert canonical_counts_labelled_device(empty, expand([6, 7], 2)).sum() == 0
