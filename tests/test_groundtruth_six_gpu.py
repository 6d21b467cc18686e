"""The ESU walk at depth six on the GPU (csrc/groundtruth6_dev.hip, canonical_counts6_device): exact counts of queries
of 2..6 nodes, bit for bit against the host enumerator, the brute-force oracle and closed forms -- integers."""
import functools
import math

import networkx as nx
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import groundtruth_mono_vf2 as M  # noqa: E402
from desco_amd import groundtruth as GT  # noqa: E402
from desco_amd import synthetic  # noqa: E402
from desco_amd.graphs import GraphSet  # noqa: E402
from desco_amd.groundtruth import canonical_counts, canonical_counts6_device, census_classes  # noqa: E402
from oracle import partition as OP  # noqa: E402
from helpers import golden_graphs  # noqa: E402

ALL = [(k, list(e)) for kk in (2, 3, 4, 5, 6) for k, e in census_classes(kk)]       # 142 classes, the 112 of 6 nodes last
SIX0 = 30                                                                           # first 6-node column
PATH6, STAR6 = (6, [(i, i + 1) for i in range(5)]), (6, [(0, i) for i in range(1, 6)])
CYCLE6, K6 = (6, [(i, (i + 1) % 6) for i in range(6)]), (6, [(a, b) for a in range(6) for b in range(a + 1, 6)])


def column_of(query):
    """the column of ``query``'s class among ALL"""
    g = nx.Graph(query[1])
    hits = [i for i, (k, e) in enumerate(ALL) if k == query[0] and nx.is_isomorphic(g, nx.Graph(e))]
    assert len(hits) == 1
    return hits[0]


@functools.lru_cache(maxsize=None)
def graph_set(case):
    if case == "golden":
        return GraphSet.from_edge_lists(golden_graphs())
    if case == "dense":            # dense random graphs, hubs, an isolated node, a single-node graph
        rng = np.random.default_rng(1)
        graphs = []
        for n, p in [(30, 0.4), (70, 0.15), (1, 0.0), (45, 0.25), (2, 1.0)]:
            e = [(a, b) for a in range(n) for b in range(a + 1, n) if rng.random() < p and b != n - 1]
            graphs.append((n, e))
        return GraphSet.from_edge_lists(graphs)
    if case == "syn":
        return synthetic.WORKLOADS["syn_1827"]().subset(300, 340)
    return synthetic.WORKLOADS["cox2"]()


@functools.lru_cache(maxsize=None)
def host_counts(case):
    """the host enumerator on all 142 classes: computed once per process, never changed"""
    out = canonical_counts(graph_set(case), ALL, backend="host").long()
    out.numpy().flags.writeable = False
    return out


@functools.lru_cache(maxsize=None)
def device_counts(case):
    return canonical_counts6_device(graph_set(case), ALL).cpu()


@pytest.mark.parametrize("case", ["golden", "dense", "cox2", "syn"])
def test_all_142_classes_equal_the_host_enumerator(case):
    host, dev = host_counts(case), device_counts(case)
    six = host[:, SIX0:]
    print(case, "six-node subsets", int(six.sum()), "non-empty classes", int((six.sum(0) > 0).sum()),
          "largest cell", int(six.max()))
    assert dev.dtype == torch.int64 and dev.shape == host.shape == (graph_set(case).num_nodes, 142)
    if case == "syn":              # no 6-node column is compared as 0 == 0 only
        assert graph_set(case).num_nodes == 938 and int((six.sum(0) > 0).sum()) == 112
    if case == "dense":
        assert int(six.sum()) == 5464999 and int((six.sum(0) > 0).sum()) == 111 and int(six.max()) == 68846
    assert torch.equal(dev, host), (dev - host).abs().max()


def test_against_the_bruteforce_oracle():
    rng = np.random.default_rng(3)
    edges = sorted({(int(min(a, b)), int(max(a, b))) for a, b in rng.integers(0, 12, size=(30, 2)) if a != b})
    qs = [(2, [(0, 1)]), (3, [(0, 1), (1, 2)]), (4, [(0, 1), (0, 2), (0, 3)]), (5, [(i, (i + 1) % 5) for i in range(5)]),
          (4, [(0, 1), (1, 2), (2, 3), (3, 0), (0, 2)]), PATH6, STAR6, CYCLE6, K6,
          (6, [(0, 1), (1, 2), (2, 0), (2, 3), (3, 4), (4, 5), (5, 3)]),             # two triangles bridged
          (6, [(0, 1), (1, 2), (2, 3), (3, 0), (0, 4), (4, 5), (1, 4)]),             # a ring with a triangle and a tail
          (6, [(0, 1), (1, 2), (2, 3), (3, 4), (1, 5)])]                             # a spider
    got = canonical_counts6_device(GraphSet.from_edge_lists([(12, edges)]), qs).cpu()
    want = OP.canonical_counts_bruteforce(12, edges, qs)
    assert want[:, 5:].sum() > 0 and got.tolist() == want.tolist()


def test_closed_forms():
    six = ALL[SIX0:]
    k6, star, path = column_of(K6) - SIX0, column_of(STAR6) - SIX0, column_of(PATH6) - SIX0
    # K12: C(v, 5) six-cliques have v as their largest node; nothing else of 6 nodes is induced
    k12 = GraphSet.from_edge_lists([(12, [(a, b) for a in range(12) for b in range(a + 1, 12)])])
    got = canonical_counts6_device(k12, six).cpu()
    want = torch.zeros((12, 112), dtype=torch.int64)
    want[:, k6] = torch.tensor([math.comb(v, 5) for v in range(12)])
    assert torch.equal(got, want)
    # the star with 250 leaves, the hub the largest id: C(250, 5) > 2^32 six-stars at the hub
    hub_last = GraphSet.from_edge_lists([(251, [(v, 250) for v in range(250)])])
    got = canonical_counts6_device(hub_last, six).cpu()
    want = torch.zeros((251, 112), dtype=torch.int64)
    want[250, star] = math.comb(250, 5)
    assert math.comb(250, 5) == 7817031300 > 2 ** 32 and torch.equal(got, want)
    # the same star, the hub id 0: the six-stars whose largest node is leaf v choose 4 of the v - 1 smaller leaves
    hub_first = GraphSet.from_edge_lists([(251, [(0, v) for v in range(1, 251)])])
    got = canonical_counts6_device(hub_first, six).cpu()
    want = torch.zeros((251, 112), dtype=torch.int64)
    want[:, star] = torch.tensor([math.comb(v - 1, 4) if v else 0 for v in range(251)])
    assert torch.equal(got, want)
    # the path 0-1-...-19 and the 6-ring alone
    p20 = GraphSet.from_edge_lists([(20, [(i, i + 1) for i in range(19)]), CYCLE6])
    got = canonical_counts6_device(p20, six).cpu()
    want = torch.zeros((26, 112), dtype=torch.int64)
    want[5:20, path] = 1
    want[25, column_of(CYCLE6) - SIX0] = 1     # (the ring's one 6-subset induces the ring: no path)
    assert torch.equal(got, want)


def test_same_bits_from_the_same_inputs():
    gs, full = graph_set("dense"), device_counts("dense")
    assert torch.equal(canonical_counts6_device(gs, ALL).cpu(), full)                      # two identical calls
    for slice_entries in (1, 7):
        assert torch.equal(canonical_counts6_device(gs, ALL, slice_entries=slice_entries).cpu(), full), slice_entries
    lo, hi = int(gs.graph_ptr[1]), int(gs.graph_ptr[2])                                   # a graph alone: its rows
    assert torch.equal(canonical_counts6_device(gs.subset(1, 2), ALL).cpu(), full[lo:hi])
    some = [141, 3, SIX0, 77, 100]                                                         # a query subset: those columns
    assert torch.equal(canonical_counts6_device(gs, [ALL[i] for i in some]).cpu(), full[:, some])
    with pytest.raises(ValueError, match="slice_entries"):
        canonical_counts6_device(gs, ALL, slice_entries=0)


def test_noninduced_equals_host_and_matcher():
    twelve = M.twelve_six_node_queries()
    queries = twelve + [twelve[3], nx.path_graph(2), nx.path_graph(4), twelve[0]]          # duplicates, other sizes
    for case in ("golden", "syn"):
        gs = graph_set(case)
        got = canonical_counts6_device(gs, queries, induced=False).cpu()
        host = canonical_counts(gs, queries, backend="host", induced=False)
        assert got.dtype == torch.int64 and got.sum() > 0
        assert torch.equal(got.double(), host), case
    matcher = canonical_counts(graph_set("syn"), queries, backend="host", induced=False, method="matcher")
    assert torch.equal(canonical_counts6_device(graph_set("syn"), queries, induced=False).cpu().double(), matcher)


def test_auto_routing_and_last_esu_backend():
    gs = graph_set("golden")
    mixed = [(3, [(0, 1), (1, 2)]), (5, [(i, (i + 1) % 5) for i in range(5)]), PATH6, CYCLE6,
             (7, [(i, i + 1) for i in range(6)])]
    host = canonical_counts(gs, mixed, backend="host")
    assert GT.last_esu_backend == "host"
    GT.last_esu_backend = None
    assert torch.equal(canonical_counts(gs, mixed, backend="auto"), host)
    assert GT.last_esu_backend == ("device6" if GT.AUTO_USES_DEVICE6 else "host")
    host_mono = canonical_counts(gs, mixed, backend="host", induced=False)
    GT.last_esu_backend = None
    assert torch.equal(canonical_counts(gs, mixed, backend="auto", induced=False), host_mono)
    assert GT.last_esu_backend == ("device6" if GT.AUTO_USES_DEVICE6 else "host")
    assert torch.equal(canonical_counts(gs, mixed[:2], backend="auto"), host[:, :2])        # no 6-node column
    assert GT.last_esu_backend == "device"
    assert torch.equal(canonical_counts(gs, mixed[:2], backend="auto", induced=False),
                       canonical_counts(gs, mixed[:2], backend="host", induced=False))


def test_edge_cases_and_refusals():
    singles = GraphSet.from_edge_lists([(1, []), (1, []), (1, [])])
    assert canonical_counts6_device(singles, ALL).cpu().tolist() == [[0] * 142] * 3
    assert canonical_counts6_device(GraphSet.from_edge_lists([]), ALL).shape == (0, 142)
    no_edges = GraphSet.from_edge_lists([(7, [])])
    out = canonical_counts6_device(no_edges, ALL)
    assert out.shape == (7, 142) and out.is_cuda and int(out.sum()) == 0
    assert int(canonical_counts6_device(no_edges, [PATH6], induced=False).sum()) == 0
    gs = graph_set("golden")
    for induced in (True, False):
        none = canonical_counts6_device(gs, [], induced=induced)
        assert none.shape == (gs.num_nodes, 0) and none.dtype == torch.int64 and none.is_cuda
        with pytest.raises(RuntimeError, match="2..6 nodes"):
            canonical_counts6_device(gs, [PATH6, (7, [(i, i + 1) for i in range(6)])], induced=induced)
    with pytest.raises(RuntimeError, match="isomorphic"):
        canonical_counts6_device(gs, [PATH6, (6, [(5, 4), (4, 3), (3, 0), (0, 1), (1, 2)])])
    with pytest.raises(RuntimeError, match="2..5 nodes"):                                  # (stays refused, on purpose)
        GT.canonical_counts_device(gs, [PATH6])
