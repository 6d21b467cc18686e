"""k-core / k-truss decomposition on the host (csrc/core_truss.cpp, desco_amd/decomposition.py): the plain-Python peels
of decomposition_reference.py against networkx, the host twin against those peels bit for bit, support against the edge
orbit counts, independence of threads / neighbours / labelling, the k-core and k-truss graph sets against networkx, the
refusals of the entry point, and the driver."""
import csv
import os
import warnings

import networkx as nx
import numpy as np
import pytest

import decomposition_reference as R
from helpers import random_family_graphs
from desco_amd import _lib, decomposition as D, synthetic
from desco_amd.graphs import GraphSet
from desco_amd.groundtruth import edge_orbit_counts, edge_orbit_rows

TRIANGLE = (3, ((0, 1), (0, 2), (1, 2)))


def nx_graph(n, edges):
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_edges_from(edges)
    return g


def edge_set(g):
    return {(min(a, b), max(a, b)) for a, b in g.edges()}


def check_reference_against_networkx(n, edges):
    g = nx_graph(n, edges)
    assert R.core_numbers(n, edges) == [nx.core_number(g)[v] for v in range(n)]
    st = R.truss_numbers(n, edges)
    assert set(st) == edge_set(g)
    top = max([t for _, t in st.values()], default=2)
    for k in range(2, top + 2):
        assert edge_set(nx.k_truss(g, k)) == {e for e, (_, t) in st.items() if t >= k}, k
    assert all(s == len(set(g[a]) & set(g[b])) for (a, b), (s, _) in st.items())


def test_reference_equals_networkx_on_the_families():
    for name, n, edges in R.family_graphs():
        check_reference_against_networkx(n, edges)


def test_reference_equals_networkx_on_random_graphs():
    for seed in range(30):
        rng = np.random.default_rng(seed)
        g = nx.gnp_random_graph(int(rng.integers(5, 41)), float(rng.uniform(0.1, 0.7)), seed=seed)
        check_reference_against_networkx(g.number_of_nodes(), list(g.edges()))


@pytest.fixture(scope="module")
def sets():
    syn = synthetic.WORKLOADS["syn_1827"]()
    assert D._device_fit(syn).all()                              # every graph of the benchmark shape fits the device
    out = {"families": R.families(), "dense": R.dense_random(),
           "random_families": GraphSet.from_edge_lists(random_family_graphs(43, 90)), "syn": syn.subset(300, 420)}
    return {name: (g, R.decompose(g)) for name, g in out.items()}


NAMES = ["families", "dense", "random_families", "syn"]


@pytest.mark.parametrize("name", NAMES)
def test_host_twin_equals_the_reference(sets, name):
    g, (core, truss, support) = sets[name]
    res = D.decompose(g, backend="host")
    assert D.last_backend == res.last_backend == "host"
    assert truss.max() >= 4, "a constant answer must not pass"
    for got, want in ((res.core, core), (res.truss, truss), (res.support, support)):
        assert got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(res.node_truss, D._node_truss_host(g.num_nodes, res.rows, truss))
    assert (res.core >= res.node_truss - 1).all()                 # an edge of a k-truss has both ends in the (k-1)-core
    if name == "syn":
        assert truss.min() == 2 and truss.max() == 24 and core.max() == 23
    if name == "families":
        by_name = {nm: i for i, (nm, _, _) in enumerate(R.family_graphs())}
        table = res.graph_table()
        for k in range(2, 7):                                    # K_k: (k-1)-core, k-truss, C(k, 3) triangles
            i = by_name[f"K{k}"]
            assert (table["degeneracy"][i], table["max_truss"][i], table["triangles"][i]) == (k - 1, k, k * (k - 1) * (k - 2) // 6)
            assert (table["nodes_in_top_core"][i], table["edges_in_top_truss"][i]) == (k, k * (k - 1) // 2)
        i = by_name["windmill 150"]
        assert (table["degeneracy"][i], table["max_truss"][i], table["triangles"][i]) == (2, 3, 150)
        i = by_name["star 300"]
        assert (table["degeneracy"][i], table["max_truss"][i], table["triangles"][i]) == (1, 2, 0)
        i = by_name["empty 5"]
        assert (table["degeneracy"][i], table["max_truss"][i], table["edges_in_top_truss"][i]) == (0, 0, 0)


@pytest.mark.parametrize("name", NAMES)
def test_support_is_the_triangle_column_and_rows_are_the_edge_orbit_rows(sets, name):
    g, _ = sets[name]
    res = D.decompose(g, backend="host")
    counts = edge_orbit_counts(g, [TRIANGLE], backend="host", induced=False)
    assert counts.shape == (len(res.support), 1) and np.array_equal(counts[:, 0].numpy(), res.support.astype(np.float64))
    assert res.rows.dtype == np.int64 and np.array_equal(res.rows, edge_orbit_rows(g).numpy())


def test_results_do_not_depend_on_threads_neighbours_or_labels(sets):
    g, _ = sets["random_families"]
    one, four = D.decompose(g, backend="host", num_threads=1), D.decompose(g, backend="host", num_threads=4)
    for f in ("core", "truss", "support", "node_truss"):
        assert np.array_equal(getattr(one, f), getattr(four, f)), f
    for i in (0, 4, 17, 89):                                     # a graph alone
        alone = D.decompose(g.subset(i, i + 1), backend="host")
        n0, n1 = int(g.graph_ptr[i]), int(g.graph_ptr[i + 1])
        r0, r1 = int(g.rowptr[n0]) // 2, int(g.rowptr[n1]) // 2
        assert np.array_equal(alone.core, one.core[n0:n1]) and np.array_equal(alone.truss, one.truss[r0:r1])
        assert np.array_equal(alone.support, one.support[r0:r1])
    rng = np.random.default_rng(5)
    for n, edges in [R.gnp(40, 0.3, 3), R.family_graphs()[12][1:], R.family_graphs()[14][1:]]:
        perm = rng.permutation(n)
        a = D.decompose(GraphSet.from_edge_lists([(n, edges)]), backend="host")
        b = D.decompose(GraphSet.from_edge_lists([(n, [(perm[x], perm[y]) for x, y in edges])]), backend="host")
        assert np.array_equal(b.core[perm], a.core)
        of = lambda r: {(int(u), int(v)): (int(s), int(t)) for (u, v), s, t in zip(r.rows, r.support, r.truss)}  # noqa: E731
        mapped = {(min(perm[u], perm[v]), max(perm[u], perm[v])): st for (u, v), st in of(a).items()}
        assert mapped == of(b)


@pytest.mark.parametrize("name", ["families", "dense"])
def test_k_core_and_k_truss_equal_networkx(sets, name):
    g, (core, truss, _) = sets[name]
    res = D.decompose(g, backend="host")
    lists = g.edge_lists()
    for k in range(0, int(truss.max()) + 2):
        kc, kt = res.k_core(k), res.k_truss(k)
        assert np.array_equal(kc.graph_ptr, g.graph_ptr) and np.array_equal(kt.graph_ptr, g.graph_ptr)
        for (n, edges), (_, ce), (_, te) in zip(lists, kc.edge_lists(), kt.edge_lists()):
            ng = nx_graph(n, edges)
            assert set(ce) == edge_set(nx.k_core(ng, k)), k
            if k >= 2:
                assert set(te) == edge_set(nx.k_truss(ng, k)), k
            else:
                assert set(te) == set(edges)
    again = D.decompose(res.k_truss(4), backend="host")           # fed straight back: the 4-truss is its own 4-truss
    assert (again.truss >= 4).all() and len(again.truss) == int((truss >= 4).sum())


def test_thin_wrappers_halves_and_empty_sets(sets):
    g, (core, truss, _) = sets["dense"]
    assert np.array_equal(D.core_numbers(g, backend="host"), core)
    assert np.array_equal(D.truss_numbers(g, backend="host"), truss)
    half = D.decompose(g, backend="host", truss=False)
    assert half.truss is None and half.support is None and half.node_truss is None and np.array_equal(half.core, core)
    assert set(half.graph_table()) == {"graph", "degeneracy", "nodes_in_top_core"}
    with pytest.raises(ValueError, match="k_truss needs"):
        half.k_truss(3)
    with pytest.raises(ValueError, match="unknown backend.*auto.*host.*device"):
        D.decompose(g, backend="gpu")
    empty = GraphSet.from_edge_lists([])
    res = D.decompose(empty, backend="host")
    assert res.core.shape == (0,) and res.truss.shape == (0,) and res.rows.shape == (0, 2)
    assert res.graph_table()["degeneracy"].shape == (0,) and res.k_core(1).num_graphs == 0
    bare = D.decompose(GraphSet.from_edge_lists([(5, []), (1, [])]), backend="host")
    assert bare.core.tolist() == [0] * 6 and bare.truss.shape == (0,) and bare.node_truss.tolist() == [0] * 6
    assert bare.graph_table()["max_truss"].tolist() == [0, 0] and bare.k_truss(2).num_directed_edges == 0


def test_workspace_formula_mirrors_the_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "desco_hip.h")).read()
    assert "#define DESCO_CORE_TRUSS_DEV_MAX_WORDS 40960" in hdr and D.DEVICE_MAX_WORDS == 40960
    assert f"#define DESCO_CORE_TRUSS_WAVE_WORDS {D.WAVE_WORDS}\n" in hdr and D.WAVE_WORDS in D._BUCKETS
    src = open(os.path.join(root, "desco_amd", "csrc", "core_truss.hpp")).read()
    assert "return n + 4 + 3 * m + (3 * m > n ? 3 * m : n);" in src
    assert D.workspace_words(10, 2) == 10 + 4 + 6 + 10 and D.workspace_words(10, 20) == 10 + 4 + 60 + 60
    assert D._device_fit(synthetic.cox2_shaped(64)).all()


def test_entry_point_refuses_bad_arguments_by_name():
    L = _lib.lib()
    g = GraphSet.from_edge_lists([(4, [(0, 1), (1, 2), (2, 3)])])
    N, E = 4, 6
    core, truss, sup = np.full(N, -7, np.int32), np.full(E // 2, -7, np.int32), np.full(E // 2, -7, np.int32)

    def call(graph_ptr=g.graph_ptr, rowptr=g.rowptr, col=g.col, G=1, c=core, t=truss, s=sup):
        ptr = lambda a: None if a is None else a.ctypes.data                              # noqa: E731
        keep = [np.ascontiguousarray(a) if a is not None else None for a in (graph_ptr, rowptr, col)]
        return L.desco_core_truss(ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), G, 1, ptr(c), ptr(t), ptr(s))

    def rejects(rc, word):
        assert rc == -1
        msg = L.desco_last_error()
        assert b"desco_core_truss:" in msg and word in msg, msg
        assert L.desco_rng_next(None, None, None) == -1          # (resets the message for the next case)
        assert (core == -7).all() and (truss == -7).all() and (sup == -7).all()    # nothing was written

    rejects(call(G=-1), b"negative")
    rejects(call(graph_ptr=None), b"graph_ptr is null")
    rejects(call(rowptr=None), b"rowptr is null")
    rejects(call(col=None), b"col is null")
    rejects(call(graph_ptr=np.array([0, 5, 4], np.int64), G=2), b"graph_ptr is not monotone")
    rejects(call(rowptr=np.array([0, 2, 1, 5, 6], np.int64)), b"rowptr is not monotone")
    rejects(call(col=np.array([1, 2, 0, 1, 3, 2], np.int32)), b"unsorted")
    rejects(call(col=np.array([1, 0, 3, 1, 3, 2], np.int32)), b"asymmetric")
    rejects(call(col=np.array([1, 0, 2, 1, 3, 3], np.int32)), b"loop")
    rejects(call(col=np.array([1, 0, 2, 1, 4, 2], np.int32)), b"outside")
    assert call(G=0, graph_ptr=None, rowptr=None, col=None, c=None, t=None, s=None) == 0
    # NULL outputs are honoured: each output alone gives what the full call gives
    assert call() == 0
    full = (core.copy(), truss.copy(), sup.copy())
    assert full[0].tolist() == [1, 1, 1, 1] and full[1].tolist() == [2, 2, 2] and full[2].tolist() == [0, 0, 0]
    for keep in range(3):
        outs = [np.full(N, -7, np.int32), np.full(E // 2, -7, np.int32), np.full(E // 2, -7, np.int32)]
        args = [o if i == keep else None for i, o in enumerate(outs)]
        assert call(c=args[0], t=args[1], s=args[2]) == 0 and np.array_equal(outs[keep], full[keep])
    assert call(c=None, t=None, s=None) == 0
    with pytest.raises(RuntimeError, match="desco_core_truss.*asymmetric"):
        D.decompose(GraphSet(g.graph_ptr, g.rowptr, np.array([1, 0, 3, 1, 3, 2], np.int32)), backend="host")


def test_driver_writes_three_tables(tmp_path, capsys):
    import graph_decomposition as driver
    argv = ["--datasets", "MUTAG", "--backend", "host", "--output_dir", str(tmp_path),
            "--data_root", str(tmp_path / "none")]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = driver.main(argv)
        from desco_amd.data import load_data
        gs = load_data("MUTAG", root_folder=str(tmp_path / "none"))
    res = D.decompose(gs, backend="host")
    assert [os.path.basename(out[k]) for k in ("node", "edge", "graph")] == \
        ["node-core_0.csv", "edge-truss_0.csv", "graph-decomposition_0.csv"]
    read = lambda path: list(csv.reader(open(path, newline="")))                         # noqa: E731
    nodes, edges, graphs = read(out["node"]), read(out["edge"]), read(out["graph"])
    assert nodes[0] == ["", "dataset", "graph", "node", "degree", "core", "node_truss"]
    assert edges[0] == ["", "dataset", "graph", "u", "v", "support", "truss"]
    assert graphs[0] == ["", "dataset", "graph", "degeneracy", "max_truss", "nodes_in_top_core", "edges_in_top_truss",
                         "triangles"]
    assert len(nodes) == 1 + gs.num_nodes and len(edges) == 1 + len(res.truss) and len(graphs) == 1 + gs.num_graphs
    assert [int(r[5]) for r in nodes[1:]] == res.core.tolist() and [int(r[6]) for r in edges[1:]] == res.truss.tolist()
    v = int(gs.graph_ptr[3]) + 2                                  # node 2 of graph 3
    assert nodes[1 + v][:5] == [str(v), "MUTAG", "3", "2", str(int(gs.rowptr[v + 1] - gs.rowptr[v]))]
    e = len(res.truss) // 2
    u, w = (int(x) for x in res.rows[e])
    gi = int(gs.node_graph_ids()[u])
    assert edges[1 + e][2:5] == [str(gi), str(u - int(gs.graph_ptr[gi])), str(w - int(gs.graph_ptr[gi]))]
    assert [int(r[3]) for r in graphs[1:]] == res.graph_table()["degeneracy"].tolist()
    assert "MUTAG: %d graphs" % gs.num_graphs in capsys.readouterr().out
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        again = driver.main(argv)
    assert os.path.basename(again["edge"]) == "edge-truss_1.csv"
    assert len(os.listdir(tmp_path)) == 6
