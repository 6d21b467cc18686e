"""Clique census on the host (csrc/clique_census.cpp, desco_amd/cliques.py): the twins against networkx's clique
enumeration and a plain restatement of the peel key, the closed forms of complete and complete multipartite graphs
(K70 wraps around 2^64), this project's own exact counters, independence of key and threads, the refusals of the entry
points, and the driver."""
import csv
import os
import re
import warnings
from math import comb

import numpy as np
import pytest

import clique_reference as R
from helpers import golden_graphs, random_family_graphs
from desco_amd import _lib, cliques as C, decomposition as D, synthetic
from desco_amd.graphs import GraphSet
from desco_amd.groundtruth import canonical_counts, canonical_counts_match, orbit_counts

FIELDS = ("graph_cliques", "node_cliques", "omega", "key")
KMAX = 8


def gnp_set(p):
    return GraphSet.from_edge_lists([R.gnp(n, p, 100 * n + seed) for seed, n in enumerate((28, 27, 21, 13, 6, 2))])


@pytest.fixture(scope="module")
def sets():
    out = {f"G(n, {p})": gnp_set(p) for p in (0.1, 0.3, 0.6, 0.85)}
    out["random_families"] = GraphSet.from_edge_lists(random_family_graphs(43, 60))
    out["golden"] = GraphSet.from_edge_lists(golden_graphs(max_n=40)[:40])
    out["small"] = GraphSet.from_edge_lists([(0, []), (1, []), (4, []), (2, [(0, 1)]), (5, [(1, 3)]), (3, R.clique(3))])
    return out


NAMES = ["G(n, 0.1)", "G(n, 0.3)", "G(n, 0.6)", "G(n, 0.85)", "random_families", "golden", "small"]


@pytest.mark.parametrize("name", NAMES)
def test_host_twin_equals_the_reference(sets, name):
    g = sets[name]
    want = R.census(g, KMAX)
    res = C.clique_census(g, kmax=KMAX, backend="host")
    assert C.last_backend == res.last_backend == "host" and res.status is None
    for f, w in zip(FIELDS, want):
        x = getattr(res, f)
        assert x.dtype == w.dtype and np.array_equal(x, w), f
    key, core = C.peel_order(g, backend="host")
    assert key.dtype == core.dtype == np.int32 and np.array_equal(key, want[3]) and np.array_equal(core, want[4])
    assert np.array_equal(core, D.core_numbers(g, backend="host"))
    assert (C.out_degrees(g, key) <= core).all()                  # what bounds the work
    assert (res.node_cliques[:, 0] == 1).all() and np.array_equal(res.node_cliques[:, 1], np.diff(g.rowptr))
    table = res.graph_table()
    assert list(table) == ["graph", "omega"] + [f"k{k}" for k in range(1, KMAX + 1)]
    assert all(v.dtype == np.int64 for v in table.values()) and np.array_equal(table["k3"], res.graph_cliques[:, 2])
    assert np.array_equal(table["k1"], np.diff(g.graph_ptr)) and np.array_equal(table["omega"], want[2])
    if name in ("G(n, 0.6)", "G(n, 0.85)", "random_families"):
        assert res.omega.max() >= 5, "a constant answer must not pass"
    none = C.clique_census(g, kmax=KMAX, nodes=False, backend="host")
    assert none.node_cliques is None and np.array_equal(none.graph_cliques, want[0])


@pytest.mark.parametrize("n", [33, 65, 70])
def test_complete_graphs_against_the_closed_form(n):
    g = GraphSet.from_edge_lists([(n, R.clique(n))])
    res = C.clique_census(g, kmax=64, backend="host")
    totals, row, omega = R.complete_closed_form(n, 64)
    assert res.graph_cliques[0].tolist() == totals and res.omega.tolist() == [omega]
    assert (res.node_cliques == np.array(row, np.int64)).all()
    assert C.out_degrees(g, res.key).tolist() == list(range(n - 1, -1, -1))     # no limit on the out-degree
    if n == 70:                                                   # the one place the wrap-around is exercised
        assert comb(70, 35) >= 1 << 64
        assert res.graph_cliques[0, 34] == R.as_i64(comb(70, 35))
        assert int(res.graph_cliques[0, 34]) % (1 << 64) == comb(70, 35) % (1 << 64)
    else:
        assert (res.graph_cliques >= 0).all()


@pytest.mark.parametrize("parts", [[3] * 7, [2] * 12, [1, 2, 3, 4]])
def test_complete_multipartite_graphs_against_the_closed_form(parts):
    n, edges = R.multipartite(parts)
    res = C.clique_census(GraphSet.from_edge_lists([(n, edges)]), kmax=14, backend="host")
    totals, rows, omega = R.multipartite_closed_form(parts, 14)
    assert res.graph_cliques[0].tolist() == totals and res.omega.tolist() == [omega] == [len(parts)]
    part = [i for i, s in enumerate(parts) for _ in range(s)]
    assert res.node_cliques.tolist() == [rows[part[v]] for v in range(n)]


def clique_query(k):
    return (k, R.clique(k))


def test_cross_checks_against_the_projects_own_counters():
    g = synthetic.WORKLOADS["syn_1827"]().subset(300, 340)
    res = C.clique_census(g, kmax=7, backend="host")
    owner = g.node_graph_ids()

    def per_graph(per_node):
        out = np.zeros(g.num_graphs, dtype=np.int64)
        np.add.at(out, owner, per_node)
        return out

    assert np.array_equal(res.graph_cliques[:, 2], D.decompose(g, backend="host").graph_table()["triangles"])
    assert res.graph_cliques[:, 4].max() >= 1
    queries = [clique_query(k) for k in (3, 4, 5)]
    canon = canonical_counts(g, queries, backend="host").numpy()
    orbits = orbit_counts(g, queries, backend="host", per_query=True).numpy()
    for j, k in enumerate((3, 4, 5)):
        assert np.array_equal(per_graph(canon[:, j].astype(np.int64)), res.graph_cliques[:, k - 1]), k
        assert np.array_equal(orbits[:, j].astype(np.int64), res.node_cliques[:, k - 1]), k
    k7 = canonical_counts_match(g, [clique_query(7)], backend="host").numpy()[:, 0]
    assert np.array_equal(per_graph(k7.astype(np.int64)), res.graph_cliques[:, 6]) and k7.sum() >= 1


def test_omega_is_exact_whatever_kmax_is(sets):
    for name in ("G(n, 0.85)", "random_families", "small"):
        g = sets[name]
        full = C.clique_census(g, kmax=KMAX, backend="host")
        one = C.clique_census(g, kmax=1, backend="host")
        assert np.array_equal(one.omega, R.census(g, 1)[2]) and np.array_equal(one.omega, full.omega)
        assert one.graph_cliques.shape == (g.num_graphs, 1) and np.array_equal(one.graph_cliques[:, 0], np.diff(g.graph_ptr))
    assert full.omega.tolist() == [0, 1, 1, 2, 2, 3]


def test_results_do_not_depend_on_key_or_threads(sets):
    g = sets["G(n, 0.6)"]
    one = C.clique_census(g, kmax=KMAX, backend="host", num_threads=1)
    four = C.clique_census(g, kmax=KMAX, backend="host", num_threads=4)
    rng = np.random.default_rng(9)
    for key in (rng.permutation(g.num_nodes), np.zeros(g.num_nodes), rng.integers(0, 3, g.num_nodes)):
        other = C.clique_census(g, kmax=KMAX, backend="host", key=key.astype(np.int32))
        assert np.array_equal(other.key, key)
        for f in FIELDS[:3]:
            assert np.array_equal(getattr(one, f), getattr(four, f)) and np.array_equal(getattr(one, f), getattr(other, f)), f
    k1, c1 = C.peel_order(g, backend="host", num_threads=1)
    k4, c4 = C.peel_order(g, backend="host", num_threads=4)
    assert np.array_equal(k1, k4) and np.array_equal(c1, c4) and np.array_equal(k1, one.key)
    for i in (0, 3):                                              # a graph alone: the key starts again at 0 per graph
        alone = C.clique_census(g.subset(i, i + 1), kmax=KMAX, backend="host")
        n0, n1 = int(g.graph_ptr[i]), int(g.graph_ptr[i + 1])
        assert np.array_equal(alone.key, one.key[n0:n1]) and alone.key.min() == 0
        assert np.array_equal(alone.node_cliques, one.node_cliques[n0:n1])


def test_python_refuses_bad_arguments(sets):
    g = sets["small"]
    with pytest.raises(ValueError, match="unknown backend.*auto.*host.*device"):
        C.clique_census(g, backend="gpu")
    with pytest.raises(ValueError, match="unknown backend"):
        C.peel_order(g, backend="gpu")
    for kmax in (0, 65):
        with pytest.raises(ValueError, match="DESCO_CLIQUE_MAX_K"):
            C.clique_census(g, kmax=kmax, backend="host")
    with pytest.raises(ValueError, match="one entry per node"):
        C.clique_census(g, backend="host", key=np.zeros(3, np.int32))
    with pytest.raises(RuntimeError, match="desco_clique_census.*negative"):
        C.clique_census(g, backend="host", key=np.full(g.num_nodes, -1, np.int32))
    empty = C.clique_census(GraphSet.from_edge_lists([]), kmax=3, backend="host")
    assert empty.graph_cliques.shape == (0, 3) and empty.node_cliques.shape == (0, 3) and empty.omega.shape == (0,)
    assert empty.graph_table()["k2"].shape == (0,)


def test_limits_and_formulas_mirror_the_headers():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "desco_hip.h")).read()
    assert f"#define DESCO_CLIQUE_MAX_K {C.MAX_K}\n" in hdr and C.MAX_K == 64
    assert f"#define DESCO_CLIQUE_DEV_MAX_OUT {C.DEVICE_MAX_OUT}\n" in hdr and C.DEVICE_MAX_OUT == C._OUT_BUCKETS[-1] == 64
    assert "#define DESCO_PEEL_DEV_MAX_WORDS 40960" in hdr and C.DEVICE_MAX_WORDS == C._PEEL_BUCKETS[-1] == 40960
    assert f"#define DESCO_PEEL_WAVE_WORDS {C.WAVE_WORDS}\n" in hdr and C.WAVE_WORDS in C._PEEL_BUCKETS
    src = open(os.path.join(root, "desco_amd", "csrc", "clique_census.hpp")).read()
    assert "return 2 * n + 2 * m + 8;" in src and C.peel_words(10, 20) == 68
    assert "return 8 * max_out + ((4 * max_out + 7) & ~(int64_t)7) + 16 * 64 * max_out + 8 * (max_out + 1) * kmax;" in src
    assert C.wave_bytes(64, 64) == 512 + 256 + 65536 + 33280 <= 160 * 1024 and 4 * C.wave_bytes(16, 64) <= 160 * 1024
    assert C._peel_fit(synthetic.cox2_shaped(64)).all()


def test_new_symbols_are_exported_and_signed():
    L = _lib.lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "desco_hip.h")).read(), flags=re.S)
    for name in ("desco_peel_order", "desco_clique_census", "desco_peel_order_dev", "desco_clique_census_dev"):
        assert hasattr(L, name) and name in _lib.SIGNATURES and re.search(rf"\b{name}\s*\(", hdr), name
    assert L.desco_abi_version() == 6


def test_entry_points_refuse_bad_arguments_by_name():
    L = _lib.lib()
    g = GraphSet.from_edge_lists([(4, [(0, 1), (1, 2), (2, 3)])])
    N, K = 4, 3
    key, core = np.full(N, -7, np.int32), np.full(N, -7, np.int32)
    gc, nc, om = np.full((1, K), -7, np.int64), np.full((N, K), -7, np.int64), np.full(1, -7, np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data                                  # noqa: E731

    def peel(graph_ptr=g.graph_ptr, rowptr=g.rowptr, col=g.col, G=1, k=key, c=core):
        keep = [np.ascontiguousarray(a) if a is not None else None for a in (graph_ptr, rowptr, col)]
        return L.desco_peel_order(ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), G, 1, ptr(k), ptr(c))

    def census(graph_ptr=g.graph_ptr, rowptr=g.rowptr, col=g.col, G=1, k=None, kmax=K, a=gc, b=nc, c=om):
        keep = [np.ascontiguousarray(x) if x is not None else None for x in (graph_ptr, rowptr, col, k)]
        return L.desco_clique_census(ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), G, ptr(keep[3]), kmax, 1, ptr(a), ptr(b),
                                     ptr(c))

    def rejects(rc, name, word):
        assert rc == -1
        msg = L.desco_last_error()
        assert name + b":" in msg and word in msg, msg
        assert L.desco_rng_next(None, None, None) == -1          # (resets the message for the next case)
        for x in (key, core, gc, nc, om):
            assert (x == -7).all()                                # nothing was written

    cases = [(dict(G=-1), b"negative"), (dict(graph_ptr=None), b"graph_ptr is null"), (dict(rowptr=None), b"rowptr is null"),
             (dict(col=None), b"col is null"),
             (dict(graph_ptr=np.array([0, 5, 4], np.int64), G=2), b"graph_ptr is not monotone"),
             (dict(rowptr=np.array([0, 2, 1, 5, 6], np.int64)), b"rowptr is not monotone"),
             (dict(col=np.array([1, 2, 0, 1, 3, 2], np.int32)), b"unsorted"),
             (dict(col=np.array([1, 0, 3, 1, 3, 2], np.int32)), b"asymmetric"),
             (dict(col=np.array([1, 0, 2, 1, 3, 3], np.int32)), b"loop"),
             (dict(col=np.array([1, 0, 2, 1, 4, 2], np.int32)), b"outside")]
    for kwargs, word in cases:
        rejects(peel(**kwargs), b"desco_peel_order", word)
        rejects(census(**kwargs), b"desco_clique_census", word)
    rejects(peel(k=None), b"desco_peel_order", b"key_out is null")
    rejects(census(kmax=0), b"desco_clique_census", b"DESCO_CLIQUE_MAX_K")
    rejects(census(kmax=65), b"desco_clique_census", b"DESCO_CLIQUE_MAX_K")
    rejects(census(k=np.array([0, 1, -1, 2], np.int32)), b"desco_clique_census", b"negative")
    assert peel(G=0, graph_ptr=None, rowptr=None, col=None, k=None, c=None) == 0
    assert census(G=0, graph_ptr=None, rowptr=None, col=None, a=None, b=None, c=None) == 0
    # NULL outputs are honoured: each output alone gives what the full call gives
    assert peel() == 0 and key.tolist() == [0, 1, 1, 0] and core.tolist() == [1, 1, 1, 1]
    only = np.full(N, -7, np.int32)
    assert peel(k=only, c=None) == 0 and only.tolist() == [0, 1, 1, 0]
    assert census() == 0
    assert gc.tolist() == [[4, 3, 0]] and om.tolist() == [2] and nc.tolist() == [[1, 1, 0], [1, 2, 0], [1, 2, 0], [1, 1, 0]]
    for keep in range(3):
        outs = [np.full((1, K), -7, np.int64), np.full((N, K), -7, np.int64), np.full(1, -7, np.int32)]
        args = [o if i == keep else None for i, o in enumerate(outs)]
        assert census(a=args[0], b=args[1], c=args[2]) == 0 and np.array_equal(outs[keep], (gc, nc, om)[keep])
    assert census(a=None, b=None, c=None) == 0
    with pytest.raises(RuntimeError, match="desco_peel_order.*asymmetric"):
        C.peel_order(GraphSet(g.graph_ptr, g.rowptr, np.array([1, 0, 3, 1, 3, 2], np.int32)), backend="host")


def test_driver_writes_its_tables(tmp_path, capsys):
    import clique_census as driver
    argv = ["--datasets", "MUTAG", "--kmax", "4", "--nodes", "--backend", "host", "--output_dir", str(tmp_path),
            "--data_root", str(tmp_path / "none")]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = driver.main(argv)
        from desco_amd.data import load_data
        gs = load_data("MUTAG", root_folder=str(tmp_path / "none"))
    res = C.clique_census(gs, kmax=4, backend="host")
    assert [os.path.basename(out[k]) for k in ("graph", "node")] == ["graph-cliques_0.csv", "node-cliques_0.csv"]
    read = lambda path: list(csv.reader(open(path, newline="")))                         # noqa: E731
    graphs, nodes = read(out["graph"]), read(out["node"])
    assert graphs[0] == ["", "dataset", "graph", "omega", "k1", "k2", "k3", "k4"]
    assert nodes[0] == ["", "dataset", "graph", "node", "core", "k1", "k2", "k3", "k4"]
    assert len(graphs) == 1 + gs.num_graphs and len(nodes) == 1 + gs.num_nodes
    assert [int(r[3]) for r in graphs[1:]] == res.omega.tolist()
    assert [[int(x) for x in r[4:]] for r in graphs[1:]] == res.graph_cliques.tolist()
    assert [[int(x) for x in r[5:]] for r in nodes[1:]] == res.node_cliques.tolist()
    v = int(gs.graph_ptr[3]) + 2                                  # node 2 of graph 3
    assert nodes[1 + v][:4] == [str(v), "MUTAG", "3", "2"]
    assert [int(r[4]) for r in nodes[1:]] == C.peel_order(gs, backend="host")[1].tolist()
    printed = capsys.readouterr().out
    assert "MUTAG: %d graphs" % gs.num_graphs in printed and "omega" in printed and "k4" in printed
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        again = driver.main(argv[:4] + argv[5:])                  # without --nodes: one table
    assert os.path.basename(again["graph"]) == "graph-cliques_1.csv" and "node" not in again
    assert len(os.listdir(tmp_path)) == 3
