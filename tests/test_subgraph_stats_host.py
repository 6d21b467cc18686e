"""Data-set statistics on the host (csrc/subgraph_stats.cpp, desco_amd.analysis): the seven raw quantities of a node
set against networkx on the component the definition picks, and against closed forms.  The six integers must be equal;
clustering_sum / n must be within 1e-12 of nx.average_clustering (both are float64 sums of at most 1024 correctly
rounded terms in [0, 1]: they differ by at most about n 2^-53 = 1.1e-13)."""
import csv
import os
import warnings
from math import comb

import networkx as nx
import numpy as np
import pytest

from desco_amd import _lib, analysis
from desco_amd.graphs import GraphSet
from helpers import golden_graphs, random_family_graphs
from oracle.partition import neighborhood_dataset

CLUSTERING_TOL = 1e-12


def nx_of(gs: GraphSet, g: int) -> nx.Graph:
    n, edges = gs.subset(g, g + 1).edge_lists()[0]
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from(edges)
    return G


def nx_reference(G: nx.Graph, members):
    """(six integers, average clustering) of the set ``members`` (graph-local ids) as the reference's script gets
    them: the largest component of the induced subgraph, nodes inserted in ascending order."""
    members = sorted(int(v) for v in members)
    if not members:
        return [0, 0, 0, 0, 0, 0], 0.0
    H = nx.Graph()
    H.add_nodes_from(members)
    H.add_edges_from((a, b) for a in members for b in G[a] if b in H and a < b)
    C = H.subgraph(max(nx.connected_components(H), key=len))
    n = C.number_of_nodes()
    lengths = dict(nx.all_pairs_shortest_path_length(C))
    dist_sum = sum(sum(d.values()) for d in lengths.values())
    if n > 1:
        assert abs(dist_sum / (n * (n - 1)) - nx.average_shortest_path_length(C)) < 1e-9
    return ([len(members), n, C.number_of_edges(), nx.diameter(C), dist_sum, sum(nx.triangles(C).values()) // 3],
            nx.average_clustering(C))


def flat_sets(gs: GraphSet, sets):
    """sets: [(graph id, local ids)] -> set_ptr, set_nodes (global ids, ascending)"""
    ptr, nodes = [0], []
    for g, mem in sets:
        nodes += [int(gs.graph_ptr[g]) + v for v in sorted(mem)]
        ptr.append(len(nodes))
    return np.array(ptr, dtype=np.int64), np.array(nodes, dtype=np.int32)


def ints_of(st, k):
    return [int(getattr(st, f)[k]) for f in analysis.STAT_FIELDS]


def check_against_networkx(gs, sets, st):
    nxg = {}
    worst = 0.0
    for k, (g, mem) in enumerate(sets):
        G = nxg.setdefault(g, nx_of(gs, g))
        want, clustering = nx_reference(G, mem)
        assert ints_of(st, k) == want, (k, g, sorted(mem))
        if want[1]:
            worst = max(worst, abs(st.clustering_sum[k] / want[1] - clustering))
    print(f"[parity] clustering_sum / n vs nx.average_clustering over {len(sets)} sets: max |d| = {worst:.2e} "
          f"(gate {CLUSTERING_TOL:.0e})")
    assert worst <= CLUSTERING_TOL
    return worst


def test_golden_neighborhoods_match_networkx():
    graphs = golden_graphs()
    gs = GraphSet.from_edge_lists(graphs)
    index, _, neighs = neighborhood_dataset(graphs, 4)
    sets = [(int(g), nodes) for (g, _), (nodes, _) in zip(index, neighs)]
    assert len(sets) > 100
    st = analysis.subgraph_statistics(gs, *flat_sets(gs, sets), backend="host")
    assert analysis.last_stats_backend == "host"
    check_against_networkx(gs, sets, st)
    assert (st.n == st.members).all()                     # a canonical neighborhood is connected


def test_random_families_match_networkx():
    graphs = random_family_graphs(7, 44)
    gs = GraphSet.from_edge_lists(graphs)
    index, _, neighs = neighborhood_dataset(graphs, 4)
    sets = [(int(g), nodes) for (g, _), (nodes, _) in zip(index, neighs)]
    sets += [(g, range(n)) for g, (n, _) in enumerate(graphs)]          # whole graphs: several components, isolated nodes
    st = analysis.subgraph_statistics(gs, *flat_sets(gs, sets), backend="host")
    check_against_networkx(gs, sets, st)
    assert (st.n < st.members).any() and st.triangles.sum() > 0


def gnp_sets(seed=3, graphs=6, subsets=12):
    rng = np.random.default_rng(seed)
    el, sets = [], []
    for g in range(graphs):
        n = int(rng.integers(20, 201))
        p = (0.01, 0.03, 0.1)[g % 3]
        m = np.triu(rng.random((n, n)) < p, 1)
        el.append((n, [(int(a), int(b)) for a, b in zip(*np.nonzero(m))]))
        for _ in range(subsets):
            size = int(rng.integers(1, n + 1))
            sets.append((g, sorted(rng.choice(n, size=size, replace=False).tolist())))
    return el, sets


def test_random_subsets_of_gnp_match_networkx():
    el, sets = gnp_sets()
    gs = GraphSet.from_edge_lists(el)
    st = analysis.subgraph_statistics(gs, *flat_sets(gs, sets), backend="host")
    check_against_networkx(gs, sets, st)
    assert (st.n < st.members).sum() > 10                 # disconnected subsets are in


def closed_form_graphs():
    """name -> ((n, edges), members, expected six integers, expected clustering_sum)"""
    out = {}
    n = 130
    out["path130"] = ((n, [(v, v + 1) for v in range(n - 1)]), range(n),
                      [n, n, n - 1, n - 1, n * (n - 1) * (n + 1) // 3, 0], 0.0)
    n = 65                                                # odd cycle: every node sees 2 nodes at each distance 1..32
    out["cycle65"] = ((n, [(v, (v + 1) % n) for v in range(n)]), range(n),
                      [n, n, n, 32, n * 2 * (32 * 33 // 2), 0], 0.0)
    n = 65                                                # star K_{1,64}, the hub in the middle of the ids
    out["star64"] = ((n, [(30, v) for v in range(n) if v != 30]), range(n),
                     [n, n, 64, 2, 2 * 64 + 64 * 63 * 2, 0], 0.0)
    out["k65"] = ((n, [(a, b) for a in range(n) for b in range(a + 1, n)]), range(n),
                  [n, n, comb(65, 2), 1, 65 * 64, comb(65, 3)], 65.0)
    # two components of 4 nodes: a triangle with a tail on the LARGER ids, a path on the smaller ones; the tie goes
    # to the component holding the smallest id, the path
    out["tie"] = ((9, [(0, 2), (2, 4), (4, 6), (1, 3), (3, 5), (1, 5), (5, 7)]), range(9),
                  [9, 4, 3, 3, 2 * (1 + 2 + 3 + 1 + 2 + 1), 0], 0.0)
    out["isolated"] = ((12, [(0, 1), (2, 3), (4, 5)]), [2, 4, 7, 9], [4, 1, 0, 0, 0, 0], 0.0)
    out["single"] = ((3, [(0, 1)]), [2], [1, 1, 0, 0, 0, 0], 0.0)
    out["pair"] = ((3, [(0, 1)]), [0, 1], [2, 2, 1, 1, 2, 0], 0.0)
    out["empty"] = ((3, [(0, 1)]), [], [0, 0, 0, 0, 0, 0], 0.0)
    return out


def closed_form_problem():
    cases = closed_form_graphs()
    gs = GraphSet.from_edge_lists([c[0] for c in cases.values()])
    sets = [(g, c[1]) for g, c in enumerate(cases.values())]
    return cases, gs, sets


def test_closed_forms():
    cases, gs, sets = closed_form_problem()
    st = analysis.subgraph_statistics(gs, *flat_sets(gs, sets), backend="host")
    for k, (name, c) in enumerate(cases.items()):
        assert ints_of(st, k) == c[2], name
        assert st.clustering_sum[k] == c[3], name
    t = st.table()
    k = list(cases).index("k65")
    assert t["clustering"][k] == 1.0 and t["density"][k] == 1.0 and t["diameter"][k] == 1.0
    assert t["avg_degree"][k] == 64.0 and t["shortest_path_length"][k] == 1.0
    e = list(cases).index("empty")
    assert all(t[c][e] == 0.0 for c in analysis.TABLE_COLUMNS)
    one = list(cases).index("isolated")
    assert all(t[c][one] == 0.0 for c in analysis.TABLE_COLUMNS if c != "num_nodes") and t["num_nodes"][one] == 1.0
    # the closed forms hold on networkx too (so the expectations above are not this code's own output)
    for g, (name, c) in enumerate(cases.items()):
        assert nx_reference(nx_of(gs, g), c[1])[0] == c[2], name


def test_tie_and_isolated_pick_the_smallest_id():
    """Which component is C shows in the answer: the tie case's triangle component would report a triangle."""
    cases, gs, sets = closed_form_problem()
    k = list(cases).index("tie")
    st = analysis.subgraph_statistics(gs, *flat_sets(gs, sets[k:k + 1]), backend="host")
    assert st.triangles[0] == 0 and st.m[0] == 3 and st.diameter[0] == 3
    # the same graph with the triangle on the smaller ids: now it is C
    gs2 = GraphSet.from_edge_lists([(9, [(1, 3), (3, 5), (5, 7), (0, 2), (2, 4), (0, 4), (4, 6)])])
    st = analysis.subgraph_statistics(gs2, *flat_sets(gs2, [(0, range(9))]), backend="host")
    assert st.triangles[0] == 1 and st.m[0] == 4 and st.diameter[0] == 2
    assert ints_of(st, 0) == nx_reference(nx_of(gs2, 0), range(9))[0]


def test_no_sets():
    gs = GraphSet.from_edge_lists([(3, [(0, 1)])])
    st = analysis.subgraph_statistics(gs, np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), backend="host")
    assert len(st) == 0 and all(len(v) == 0 for v in st.table().values())
    # S = 0 is served before any pointer is looked at
    assert _lib.lib().desco_subgraph_stats(None, None, 0, None, None, 0, 1, None, None) == 0


def test_set_in_the_second_graph():
    """Global ids: a set of the second graph reads the second graph's rows."""
    a = (5, [(0, 1), (1, 2), (2, 3), (3, 4)])
    b = (6, [(0, 1), (0, 2), (1, 2), (2, 3), (3, 4), (4, 5)])
    gs = GraphSet.from_edge_lists([a, b])
    sets = [(1, [0, 1, 2, 3]), (0, [0, 1, 2, 3]), (1, range(6))]
    st = analysis.subgraph_statistics(gs, *flat_sets(gs, sets), backend="host")
    assert ints_of(st, 0) == [4, 4, 4, 2, 2 * (1 + 1 + 2 + 1 + 2 + 1), 1]
    assert ints_of(st, 1) == [4, 4, 3, 3, 20, 0]
    check_against_networkx(gs, sets, st)


def _raw_host(gs, set_ptr, set_nodes, rowptr=True, sp=True, sn=True, oi=True, of=True):
    S = len(set_ptr) - 1
    ints, cs = np.zeros((S, 6), dtype=np.int64), np.zeros(S)
    rc = _lib.lib().desco_subgraph_stats(
        gs.rowptr.ctypes.data if rowptr else None, gs.col.ctypes.data, gs.num_nodes,
        set_ptr.ctypes.data if sp else None, set_nodes.ctypes.data if sn else None, S, 1,
        ints.ctypes.data if oi else None, cs.ctypes.data if of else None)
    return rc, _lib.lib().desco_last_error().decode()


def test_bad_arguments_are_refused_by_name():
    gs = GraphSet.from_edge_lists([(5, [(0, 1), (1, 2), (2, 3), (3, 4)])])
    ptr, nodes = np.array([0, 3], dtype=np.int64), np.array([0, 1, 2], dtype=np.int32)
    assert _raw_host(gs, ptr, nodes)[0] == 0
    for kw, word in (("rowptr", "rowptr"), ("sp", "set_ptr"), ("sn", "set_nodes"), ("oi", "out_i64"), ("of", "out_f64")):
        rc, msg = _raw_host(gs, ptr, nodes, **{kw: False})
        assert rc != 0 and word in msg and "null" in msg, (kw, msg)
    rc, msg = _raw_host(gs, np.array([0, 3, 2], dtype=np.int64), nodes)
    assert rc != 0 and "set_ptr" in msg and "monotone" in msg
    for bad in ([0, 1, 5], [-1, 1, 2]):
        rc, msg = _raw_host(gs, ptr, np.array(bad, dtype=np.int32))
        assert rc != 0 and "outside the graph" in msg, msg
    for bad in ([0, 2, 1], [0, 1, 1]):
        rc, msg = _raw_host(gs, ptr, np.array(bad, dtype=np.int32))
        assert rc != 0 and "strictly ascending" in msg, msg
    with pytest.raises(RuntimeError, match="strictly ascending"):
        analysis.subgraph_statistics(gs, ptr, np.array([2, 1, 0]), backend="host")
    with pytest.raises(ValueError, match="backend"):
        analysis.subgraph_statistics(gs, ptr, nodes, backend="cpu")


def test_threads_do_not_change_the_result():
    el, sets = gnp_sets(seed=5, graphs=3, subsets=8)
    gs = GraphSet.from_edge_lists(el)
    ptr, nodes = flat_sets(gs, sets)
    one = analysis.subgraph_statistics(gs, ptr, nodes, backend="host", num_threads=1)
    four = analysis.subgraph_statistics(gs, ptr, nodes, backend="host", num_threads=4)
    assert all((getattr(one, f) == getattr(four, f)).all() for f in analysis.STAT_FIELDS)
    assert one.clustering_sum.tobytes() == four.clustering_sum.tobytes()


def test_a_set_above_the_inner_threshold():
    """More than 4096 members: the OpenMP loop runs over the sources of the set.  A path and a clique on a path."""
    n = 4200
    edges = [(v, v + 1) for v in range(n - 1)] + [(a, b) for a in range(6) for b in range(a + 2, 6)]
    gs = GraphSet.from_edge_lists([(n, edges)])
    st = analysis.subgraph_statistics(gs, np.array([0, n], dtype=np.int64), np.arange(n, dtype=np.int32),
                                      backend="host", num_threads=4)
    G = nx_of(gs, 0)
    assert int(st.n[0]) == n and int(st.m[0]) == G.number_of_edges()
    assert int(st.triangles[0]) == sum(nx.triangles(G).values()) // 3 == comb(6, 3)
    assert int(st.diameter[0]) == n - 6 + 1
    assert abs(st.clustering_sum[0] / n - nx.average_clustering(G)) <= CLUSTERING_TOL
    # K6 on nodes 0..5 with a path of L nodes hanging off node 5: clique pairs, node 5 - path, the five others - path,
    # path - path
    L = n - 6
    pairs = 15 + L * (L + 1) // 2 + 5 * (L * (L + 1) // 2 + L) + (L - 1) * L * (L + 1) // 6
    assert int(st.dist_sum[0]) == 2 * pairs
    one = analysis.subgraph_statistics(gs, np.array([0, n], dtype=np.int64), np.arange(n, dtype=np.int32),
                                       backend="host", num_threads=1)
    assert ints_of(one, 0) == ints_of(st, 0) and one.clustering_sum.tobytes() == st.clustering_sum.tobytes()


def _table_reference(gs, sets):
    rows = []
    nxg = {}
    for g, mem in sets:
        G = nxg.setdefault(g, nx_of(gs, g))
        H = G.subgraph(mem)
        C = H.subgraph(max(nx.connected_components(H), key=len))
        n, m = C.number_of_nodes(), C.number_of_edges()
        rows.append(dict(clustering=nx.average_clustering(C),
                         shortest_path_length=nx.average_shortest_path_length(C) if n > 1 else 0.0,
                         diameter=nx.diameter(C), density=nx.density(C), num_nodes=n, num_edges=m,
                         avg_degree=2.0 * m / n))
    return rows


def _check_table(table, rows):
    assert list(table) == list(analysis.TABLE_COLUMNS)
    for k, row in enumerate(rows):
        for c in analysis.TABLE_COLUMNS:
            tol = 0.0 if c in ("diameter", "num_nodes", "num_edges") else 1e-12
            assert abs(table[c][k] - row[c]) <= tol, (k, c, table[c][k], row[c])


def test_neighborhood_and_graph_statistics_tables():
    graphs = random_family_graphs(11, 12)
    gs = GraphSet.from_edge_lists(graphs)
    index, _, neighs = neighborhood_dataset(graphs, 3)
    st = analysis.neighborhood_statistics(gs, depth=3, backend="host")
    assert analysis.last_stats_backend == "host"
    assert st.neigh_index.tolist() == index.tolist()
    _check_table(st.table(), _table_reference(gs, [(int(g), nodes) for (g, _), (nodes, _) in zip(index, neighs)]))
    gt = analysis.graph_statistics(gs, backend="host")
    assert len(gt) == len(graphs) and gt.members.tolist() == [n for n, _ in graphs]
    _check_table(gt.table(), _table_reference(gs, [(g, range(n)) for g, (n, _) in enumerate(graphs)]))
    # the restricted neighborhoods are node sets like any other
    rs = analysis.neighborhood_statistics(gs, depth=2, restricted=True, backend="host")
    assert len(rs) == len(rs.neigh_index) and (rs.n == rs.members).all()


def test_degree_sorted_partition_is_sorted_back():
    from desco_amd.partition import build_partition
    gs = GraphSet.from_edge_lists(random_family_graphs(2, 8))
    part = build_partition(gs, 4)
    a = analysis.neighborhood_statistics(gs, backend="host", partition=part)
    b = analysis.neighborhood_statistics(gs, backend="host", partition=part.degree_sorted())
    assert all((getattr(a, f) == getattr(b, f)).all() for f in analysis.STAT_FIELDS)
    assert a.clustering_sum.tobytes() == b.clustering_sum.tobytes()


def test_driver_end_to_end(tmp_path):
    import dataset_statistics as D
    from desco_amd.data import load_data
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = D.main(["--datasets", "MUTAG", "--depth", "2", "--graphs", "--backend", "host",
                      "--output_dir", str(tmp_path), "--data_root", str(tmp_path / "none")])
        gs = load_data("MUTAG", root_folder=str(tmp_path / "none"))
    st = analysis.neighborhood_statistics(gs, depth=2, backend="host")
    assert os.path.basename(out["neighborhood"]) == "neighborhood-features_0.csv"
    assert os.path.basename(out["graph"]) == "graph-features_0.csv"
    with open(out["neighborhood"], newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["", "dataset", "clustering", "shortest_path_length", "diameter", "density", "num_nodes",
                       "num_edges", "avg_degree"]
    assert len(rows) == 1 + len(st) and len(st) > 0
    assert [r[0] for r in rows[1:]] == [str(k) for k in range(len(st))] and {r[1] for r in rows[1:]} == {"MUTAG"}
    t = st.table()
    for k in (0, len(st) // 2, len(st) - 1):
        assert [float(x) for x in rows[1 + k][2:]] == [float(t[c][k]) for c in analysis.TABLE_COLUMNS]
    with open(out["graph"], newline="") as f:
        assert len(list(csv.reader(f))) == 1 + gs.num_graphs
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        again = D.main(["--datasets", "MUTAG", "--depth", "2", "--backend", "host", "--output_dir", str(tmp_path),
                        "--data_root", str(tmp_path / "none")])
    assert os.path.basename(again["neighborhood"]) == "neighborhood-features_1.csv" and "graph" not in again
    assert sorted(os.listdir(tmp_path)) == ["graph-features_0.csv", "neighborhood-features_0.csv",
                                            "neighborhood-features_1.csv"]
