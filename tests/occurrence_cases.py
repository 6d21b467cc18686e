"""The cases of the occurrence-listing tests (host: test_occurrences_host.py, GPU: test_occurrences_gpu.py) and the
property check they share.  Each case is the smallest that reaches one path of the walk."""
import functools

import networkx as nx
import numpy as np

import occurrence_reference as R
from desco_amd.graphs import GraphSet
from desco_amd.groundtruth import canonical_counts_match, match_plan
from helpers import golden_graphs

EDGE = (2, [(0, 1)])
P3 = (3, [(0, 1), (1, 2)])
TRIANGLE = (3, [(0, 1), (1, 2), (0, 2)])
C4 = (4, [(0, 1), (1, 2), (2, 3), (3, 0)])
TAILED = (4, [(0, 1), (1, 2), (0, 2), (2, 3)])
DIAMOND = (4, [(0, 1), (1, 2), (2, 3), (3, 0), (0, 2)])
STAR5 = (5, [(0, 1), (0, 2), (0, 3), (0, 4)])
HOUSE = (5, [(0, 1), (1, 2), (2, 3), (3, 0), (0, 4), (1, 4)])
P16 = (16, [(i, i + 1) for i in range(15)])


def _nx_set(graphs):
    return GraphSet.from_edge_lists([(g.number_of_nodes(), sorted(tuple(sorted(e)) for e in g.edges())) for g in graphs])


@functools.lru_cache(maxsize=None)
def small_set() -> GraphSet:
    """The five golden graphs of at most 9 nodes (the brute force's limit), K5 minus an edge for the diamond and the
    3-rung ladder for induced 4-cycles."""
    k5 = nx.complete_graph(5)
    k5.remove_edge(0, 4)
    few = golden_graphs(max_n=9)
    assert len(few) == 5
    return GraphSet.from_edge_lists(few + [(5, sorted(k5.edges())), (6, sorted(nx.ladder_graph(3).edges()))])


@functools.lru_cache(maxsize=None)
def stars_set() -> GraphSet:
    """K1,70 twice: hub = the largest id (one anchor, the hub's record, with all C(70, 4) rows and 70 position-2
    candidates) and hub = the smallest id (the leaf record at 70 anchors)."""
    return GraphSet.from_edge_lists([(71, [(u, 70) for u in range(70)]), (71, [(0, u) for u in range(1, 71)])])


@functools.lru_cache(maxsize=None)
def paths_set() -> GraphSet:
    return _nx_set([nx.path_graph(16), nx.cycle_graph(17)])


@functools.lru_cache(maxsize=None)
def three_set() -> GraphSet:
    """5, 70 and 130 nodes (1, 2 and 3 bitset words per row; sparse random graphs with triangles and 4-cycles), an
    edgeless graph and a tree (no occurrence of any cyclic query)."""
    gs = [nx.complete_graph(5)] + [nx.gnm_random_graph(n, 2 * n + n // 2, seed=n) for n in (70, 130)]
    return _nx_set([gs[0], nx.empty_graph(7), gs[1], nx.path_graph(6), gs[2]])


@functools.lru_cache(maxsize=None)
def k6_set() -> GraphSet:
    return _nx_set([nx.complete_graph(6)])


# name -> (graph set, query, modes, yardstick: "vf2" | "brute+vf2" | "star")
CASES = {
    "edge": (small_set, EDGE, (True, False), "brute+vf2"),
    "p3": (small_set, P3, (True, False), "brute+vf2"),
    "triangle": (small_set, TRIANGLE, (True, False), "brute+vf2"),
    "c4": (small_set, C4, (True, False), "brute+vf2"),
    "tailed": (small_set, TAILED, (True, False), "brute+vf2"),
    "diamond": (small_set, DIAMOND, (True, False), "brute+vf2"),
    "star5-in-k1,70": (stars_set, STAR5, (True, False), "star"),
    "p16": (paths_set, P16, (True, False), "vf2"),
    "three-triangle": (three_set, TRIANGLE, (True, False), "vf2"),
    "three-c4": (three_set, C4, (True, False), "vf2"),
    "three-tailed": (three_set, TAILED, (True, False), "vf2"),
    "k6-triangle": (k6_set, TRIANGLE, (True, False), "vf2"),
    "k6-p3": (k6_set, P3, (False,), "vf2"),
    "k6-c4": (k6_set, C4, (False,), "vf2"),
}
CASE_MODES = [(name, induced) for name, c in CASES.items() for induced in c[2]]


@functools.lru_cache(maxsize=None)
def host_counts(name, induced):
    graphs, query = CASES[name][0](), CASES[name][1]
    return canonical_counts_match(graphs, [query], backend="host", induced=induced)[:, 0].long().numpy()


@functools.lru_cache(maxsize=None)
def yardstick(name, induced):
    make, query, _, kind = CASES[name]
    if kind == "star":
        return R.star_total(make(), query[0] - 1)
    groups = R.vf2_groups(make(), query, induced)
    if kind == "brute+vf2":
        assert groups == R.brute_force_groups(make(), query, induced)
    return groups


def anchors_of(query):
    plan = match_plan([query])
    return sorted({int(plan[2 + a * 84 + 2]) for a in range(int(plan[1]))})


def check_listing(name, induced, occ):
    """Every property of the definition (include/desco_hip.h, OCCURRENCE LISTING) on a CPU ``Occurrences``."""
    graphs, query = CASES[name][0](), CASES[name][1]
    k, edges = query
    rows, ptr = occ.rows, occ.ptr
    N = graphs.num_nodes
    assert rows.dtype == np.int32 and rows.shape == (int(ptr[-1]), k) and ptr.dtype == np.int64 and len(ptr) == N + 1
    # ptr: the scan of the canonical counts
    assert ptr[0] == 0 and np.array_equal(np.diff(ptr), host_counts(name, induced))
    M = len(rows)
    want = yardstick(name, induced)
    if M == 0:
        assert not want
        return
    # valid maps: injective, inside one graph, edges to edges (induced: non-edges to non-edges)
    A = R.adjacency(graphs)
    assert rows.min() >= 0 and rows.max() < N
    node_graph = graphs.node_graph_ids()
    assert (node_graph[rows] == node_graph[rows[:, :1]]).all()
    es = {tuple(sorted(e)) for e in edges}
    for a in range(k):
        for b in range(a + 1, k):
            assert (rows[:, a] != rows[:, b]).all()
            adj = A[rows[:, a], rows[:, b]]
            if (a, b) in es:
                assert adj.all()
            elif induced:
                assert not adj.any()
    # anchor segments: the row's maximum is the segment's node and sits in an anchor column
    seg = np.repeat(np.arange(N), np.diff(ptr))
    assert np.array_equal(rows.max(axis=1), seg)
    assert (rows[:, anchors_of(query)] == seg[:, None]).any(axis=1).all()
    # strictly ascending lexicographic order inside every segment
    differ = rows[1:] != rows[:-1]
    first = differ.argmax(axis=1)
    idx = np.arange(M - 1)
    ascending = differ.any(axis=1) & (rows[:-1][idx, first] < rows[1:][idx, first])
    assert ascending[seg[1:] == seg[:-1]].all()
    # every occurrence exactly once, nothing else
    if isinstance(want, int):                      # stars: valid + pairwise different + the total (R.star_total)
        assert M == want and N ** k < 2 ** 62
        codes = (np.sort(rows, axis=1).astype(np.int64) * N ** np.arange(k, dtype=np.int64)).sum(axis=1)
        assert len(np.unique(codes)) == M
        return
    got = {}
    for row in rows:
        key = R.row_key(row, query, induced)
        v = int(row.max())
        assert key not in got.setdefault(v, set()), f"occurrence {key} listed twice"
        got[v].add(key)
    assert got == want
