"""Degree-preserving null model on the host (csrc/null_model.cpp, desco_amd/motifs.py): the draw and the chain against
the plain-Python chain of null_model_reference.py bit for bit, the invariants of a rewired graph set, the moments of
the result class against numpy, motif_significance against the VF2 counts, refusals, and the driver."""
import csv
import os
import warnings

import numpy as np
import pytest

import null_model_reference as R
from desco_amd import _lib, motifs, synthetic
from desco_amd.graphs import GraphSet
from desco_amd.groundtruth import canonical_counts, census_classes


def host(graphs, replicas, spe, seed, graph_base=0, replica_base=0, num_threads=0):
    return motifs._rewire_host(graphs, replicas, spe, seed, graph_base, replica_base, num_threads)


def test_draw_equals_the_python_draw():
    L = _lib.lib()
    out = np.zeros(3, np.int64)
    for seed in (0, 1, 0xDEADBEEFCAFEF00D):
        for graph, replica in ((0, 0), (5, 2), (2 ** 31 + 3, 77)):
            for t in (0, 1, 63, 64, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5, 2 ** 40 + 123, 2 ** 63 - 1):
                for m in (1, 2, 3, 43, 1000, 2 ** 20, 2 ** 32 - 1):
                    assert L.desco_null_model_draw(seed, graph, replica, t, m, out.ctypes.data) == 0
                    assert tuple(out) == R.draw(seed, graph, replica, t, m), (seed, graph, replica, t, m)
                    assert 0 <= out[0] < m and 0 <= out[1] < m and out[2] in (0, 1)
    assert L.desco_null_model_draw(0, 0, 0, 0, 0, out.ctypes.data) == -1
    assert b"desco_null_model_draw" in L.desco_last_error()
    assert L.desco_null_model_draw(0, 0, 0, 0, 2 ** 32, out.ctypes.data) == -1
    assert L.desco_null_model_draw(0, 0, 0, 0, 5, None) == -1
    # the generator is the Random123 one (known-answer vector of Philox4x32-10, counter and key all ones)
    from oracle.dropout import philox4x32_10
    w = philox4x32_10([0xFFFFFFFF] * 4, (0xFFFFFFFF, 0xFFFFFFFF))
    assert [int(x) for x in w] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


@pytest.fixture(scope="module")
def ladder():
    return R.ladder()


@pytest.mark.parametrize("name", ["edges0123", "fixed", "small", "classes", "gnm40", "hub"])
@pytest.mark.parametrize("spe", [1, 20])
def test_twin_equals_the_python_chain(ladder, name, spe):
    g = ladder[name]
    col, acc = host(g, 3, spe, seed=1234 + spe, graph_base=3, replica_base=1)
    ref_col, ref_acc = R.rewire(g, 3, spe, seed=1234 + spe, graph_base=3, replica_base=1)
    assert np.array_equal(acc, ref_acc) and np.array_equal(col, ref_col)
    if name == "fixed":
        assert not acc.any() and all(np.array_equal(c, g.col) for c in col)
    if name == "edges0123":
        assert not acc[:, :2].any()                       # m = 0 and m = 1 come back unchanged
        e = int(g.rowptr[g.graph_ptr[2]])
        assert all(np.array_equal(c[:e], g.col[:e]) for c in col)
    if name in ("gnm40", "hub") and spe == 20:
        assert (acc > 0).all() and not np.array_equal(col[0], g.col)


def check_invariants(g: GraphSet, col: np.ndarray):
    rows = np.repeat(np.arange(g.num_nodes, dtype=np.int64), np.diff(g.rowptr))
    graph_of = g.node_graph_ids()
    for c in col:
        c = c.astype(np.int64)
        assert (c != rows).all()                                            # loop-free
        assert (graph_of[c] == graph_of[rows]).all()                        # inside the node's graph
        inner = np.ones(len(c), dtype=bool)
        inner[g.rowptr[:-1][np.diff(g.rowptr) > 0]] = False
        assert (np.diff(c)[inner[1:]] > 0).all()                            # rows strictly ascending: sorted, no duplicate
        key = rows * g.num_nodes + c
        assert np.array_equal(np.sort(key), np.sort(c * g.num_nodes + rows))  # symmetric
        # degrees: the rows are those of the unchanged rowptr, so the sequence is preserved when every row is full
        assert len(c) == g.num_directed_edges


@pytest.fixture(scope="module", params=["cox2", "syn"])
def dataset(request):
    if request.param == "cox2":
        return synthetic.cox2_shaped(32)
    return synthetic.syn_1827_shaped(1827).subset(700, 730)


def test_invariants_and_reproducibility(dataset):
    g = dataset
    sets, acc = motifs.rewire(g, replicas=4, swaps_per_edge=10, seed=5, backend="host", num_threads=8)
    assert motifs.last_backend == "host" and len(sets) == 4 and acc.shape == (4, g.num_graphs) and acc.dtype == np.int32
    col = np.stack([s.col for s in sets])
    for s in sets:
        assert np.array_equal(s.rowptr, g.rowptr) and np.array_equal(s.graph_ptr, g.graph_ptr)
    check_invariants(g, col)
    assert (acc > 0).all()
    assert all(not np.array_equal(col[a], col[b]) for a in range(4) for b in range(a))
    assert all(not np.array_equal(c, g.col) for c in col)
    # the same seed gives the same bits, another seed does not; 1 thread equals 8 threads
    col1, acc1 = host(g, 4, 10, 5, num_threads=1)
    assert np.array_equal(col1, col) and np.array_equal(acc1, acc)
    assert not np.array_equal(host(g, 4, 10, 6)[0], col)
    # a slice of the graphs with graph_base reproduces the whole call's rows
    g0, g1 = 5, 17
    e0, e1 = int(g.rowptr[g.graph_ptr[g0]]), int(g.rowptr[g.graph_ptr[g1]])
    cs, as_ = host(g.subset(g0, g1), 4, 10, 5, graph_base=g0)
    assert np.array_equal(cs + np.int32(g.graph_ptr[g0]), col[:, e0:e1]) and np.array_equal(as_, acc[:, g0:g1])
    # replicas 2..3 with replica_base
    cr, ar = host(g, 2, 10, 5, replica_base=2)
    assert np.array_equal(cr, col[2:]) and np.array_equal(ar, acc[2:])


def test_moments_and_p_values_against_numpy():
    rng = np.random.default_rng(3)
    R_, G, Q = 7, 3, 5
    null = rng.integers(0, 50, (R_, G, Q)).astype(np.int64)
    real = rng.integers(0, 50, (G, Q)).astype(np.int64)
    null[:, 1, 2] = 9                                                    # a zero-variance column: z is NaN
    null[:, 2, :] = real[2] = np.arange(Q)                               # a graph with no variance at all
    res = motifs.MotifSignificance([(3, ((0, 1), (1, 2)))] * Q, real, null)
    x = null.astype(np.float64)
    mean, std = x.mean(0), x.std(0, ddof=1)
    assert np.array_equal(res.mean, mean) and np.array_equal(res.std, std)
    assert std[1, 2] == 0 and np.isnan(res.z[1, 2]) and np.isnan(res.z[2]).all()
    ok = std > 0
    assert np.array_equal(res.z[ok], ((real - mean) / np.where(ok, std, 1))[ok]) and np.isnan(res.z[~ok]).all()
    z0 = np.where(ok, res.z, 0.0)
    norm = np.sqrt((z0 ** 2).sum(1, keepdims=True))
    assert np.allclose(res.profile[:2], (z0 / np.where(norm > 0, norm, 1))[:2], rtol=1e-15, atol=0)
    assert res.profile[1, 2] == 0 and (res.profile[2] == 0).all()        # NaN taken as 0; an all-zero row stays zero
    assert np.allclose(np.sqrt((res.profile[:2] ** 2).sum(1)), 1.0, rtol=1e-14)
    assert np.array_equal(res.p_over, (1 + (null >= real).sum(0)) / (R_ + 1))
    assert np.array_equal(res.p_under, (1 + (null <= real).sum(0)) / (R_ + 1))
    assert (res.p_over[2] == 1).all() and (res.p_under[2] == 1).all()
    tot, tot_null = real.sum(0), null.sum(1)
    assert np.array_equal(res.dataset_real, tot) and np.array_equal(res.dataset_null, tot_null)
    tm, ts = tot_null.astype(np.float64).mean(0), tot_null.astype(np.float64).std(0, ddof=1)
    assert np.array_equal(res.dataset_mean, tm) and np.array_equal(res.dataset_std, ts)
    assert np.array_equal(res.dataset_z, (tot - tm) / ts)
    assert np.array_equal(res.dataset_p_over, (1 + (tot_null >= tot).sum(0)) / (R_ + 1))
    assert np.array_equal(res.dataset_p_under, (1 + (tot_null <= tot).sum(0)) / (R_ + 1))
    t = res.table()
    assert list(t) == ["graph", "query", "real", "mean", "std", "z", "profile", "p_over", "p_under"]
    assert len(t["graph"]) == G * Q and t["graph"][Q] == 1 and t["query"][Q + 2] == 2 and t["real"][Q + 2] == real[1, 2]
    d = res.dataset_table()
    assert list(d) == ["query", "real", "mean", "std", "z", "profile", "p_over", "p_under"] and len(d["query"]) == Q
    with pytest.raises(ValueError, match="replicas >= 2"):
        motifs.MotifSignificance([], real, null[:1])


@pytest.mark.parametrize("induced", [True, False])
def test_motif_significance_host_against_vf2(induced):
    rng = np.random.default_rng(11)
    graphs = GraphSet.from_edge_lists([R._gnm(int(n), int(m), int(rng.integers(1 << 30)))
                                       for n, m in ((8, 12), (9, 14), (10, 13), (7, 10), (12, 18), (6, 9))])
    queries = [(3, ((0, 1), (1, 2))), (3, ((0, 1), (1, 2), (0, 2))), (4, ((0, 1), (1, 2), (2, 3))),
               (4, ((0, 1), (1, 2), (2, 3), (3, 0))), (2, ((0, 1),)), (3, ((1, 0), (0, 2))),            # a duplicate class
               (5, ((0, 1), (1, 2), (2, 3), (3, 4))), (5, ((0, 1), (0, 2), (0, 3), (0, 4)))]
    res = motifs.motif_significance(graphs, queries, replicas=3, swaps_per_edge=5, seed=2, induced=induced,
                                    backend="host", keep_null=True, replica_chunk=2)
    assert res.last_backend == motifs.last_backend == "host"

    def sums(gs):
        c = canonical_counts(gs, [(n, list(e)) for n, e in queries], backend="vf2", induced=induced).numpy()
        return np.stack([c[gs.graph_ptr[g]:gs.graph_ptr[g + 1]].sum(0) for g in range(gs.num_graphs)]).astype(np.int64)

    assert res.real.dtype == np.int64 and np.array_equal(res.real, sums(graphs))
    sets, acc = motifs.rewire(graphs, replicas=3, swaps_per_edge=5, seed=2, backend="host")
    assert np.array_equal(res.accepted, acc)
    for r in range(3):
        assert np.array_equal(res.null[r], sums(sets[r])), r
    assert np.array_equal(res.real[:, 5], res.real[:, 0]) and res.real[:, 4].tolist() == [12, 14, 13, 10, 18, 9]
    assert motifs.motif_significance(graphs, queries, replicas=3, swaps_per_edge=5, seed=2, induced=induced,
                                     backend="host").null is None


def test_default_queries_are_the_29_classes():
    flat = motifs._queries(None)
    assert len(flat) == 29 and [k for k, _ in flat] == [3] * 2 + [4] * 6 + [5] * 21
    assert [tuple(e) for _, e in flat] == [tuple(e) for k in (3, 4, 5) for _, e in census_classes(k)]


def test_c_level_refusals_name_the_entry_point():
    L = _lib.lib()
    g = GraphSet.from_edge_lists([(4, [(0, 1), (1, 2), (2, 3)])])
    col_out, acc = np.zeros((1, 6), np.int32), np.zeros((1, 1), np.int32)

    def call(graph_ptr=g.graph_ptr, rowptr=g.rowptr, col=g.col, G=1, gb=0, reps=1, rb=0, spe=1, out=col_out, a=acc):
        p = lambda x: None if x is None else x.ctypes.data
        return L.desco_null_model_rewire(p(graph_ptr), p(rowptr), p(col), G, gb, reps, rb, spe, 0, 1, p(out), p(a))

    def rejects(rc, word):
        assert rc == -1
        msg = L.desco_last_error()
        assert b"desco_null_model_rewire" in msg and word in msg, msg
        assert L.desco_rng_next(None, None, None) == -1          # (resets the message for the next case)

    assert call() == 0 and call(G=0, graph_ptr=None, rowptr=None, col=None, out=None, a=None) == 0
    rejects(call(G=-1), b"negative")
    rejects(call(reps=-1), b"negative")
    rejects(call(gb=-1), b"negative")
    rejects(call(spe=-1), b"swaps_per_edge")
    rejects(call(graph_ptr=None), b"graph_ptr is null")
    rejects(call(rowptr=None), b"rowptr is null")
    rejects(call(col=None), b"col is null")
    rejects(call(out=None), b"col_out is null")
    rejects(call(a=None), b"accepted is null")
    rejects(call(col=np.array([1, 2, 0, 1, 3, 2], np.int32)), b"unsorted")
    rejects(call(col=np.array([1, 0, 3, 1, 3, 2], np.int32)), b"asymmetric")
    rejects(call(col=np.array([1, 0, 2, 1, 3, 3], np.int32)), b"loop")
    rejects(call(col=np.array([1, 0, 2, 1, 4, 2], np.int32)), b"outside")
    rejects(call(spe=2 ** 62), b"2^63")


def test_device_entry_point_refuses_before_any_launch():
    """desco_null_model_rewire_dev checks its arguments on the host: none of these calls reaches the GPU."""
    L = _lib.lib()
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data

    def call(graph_ptr=p, rowptr=p, col=p, G=1, E=6, ids=None, num_ids=0, max_words=7, gb=0, reps=1, rb=0, spe=1,
             out=p, acc=p):
        return L.desco_null_model_rewire_dev(graph_ptr, rowptr, col, G, E, ids, num_ids, max_words, gb, reps, rb, spe,
                                             0, out, acc, None)

    def rejects(rc, word):
        assert rc == -1
        msg = L.desco_last_error()
        assert b"desco_null_model_rewire_dev" in msg and word in msg, msg
        assert L.desco_rng_next(None, None, None) == -1          # (resets the message for the next case)

    assert call(G=0) == 0 and call(reps=0) == 0                   # nothing to do
    rejects(call(G=-1), b"negative")
    rejects(call(spe=-1), b"swaps_per_edge")
    rejects(call(rb=-1), b"negative")
    rejects(call(max_words=-1), b"negative")
    rejects(call(max_words=40961), b"DESCO_NULL_MODEL_DEV_MAX_WORDS")
    rejects(call(max_words=int(motifs.workspace_words(1200, 1200))), b"DESCO_NULL_MODEL_DEV_MAX_WORDS")
    rejects(call(spe=2 ** 62), b"2^63")
    rejects(call(graph_ptr=None), b"graph_ptr is null")
    rejects(call(rowptr=None), b"rowptr is null")
    rejects(call(col=None), b"col is null")
    rejects(call(out=None), b"col_out is null")
    rejects(call(acc=None), b"accepted is null")
    rejects(call(rowptr=p + 4), b"aligned")
    assert motifs.DEVICE_MAX_WORDS == 40960
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "desco_hip.h")).read()
    assert "#define DESCO_NULL_MODEL_DEV_MAX_WORDS 40960" in hdr


def test_python_refusals():
    g = GraphSet.from_edge_lists([(4, [(0, 1), (1, 2), (2, 3)])])
    six = (6, [(i, i + 1) for i in range(5)])
    with pytest.raises(ValueError, match="queries of 2..5 nodes"):
        motifs.motif_significance(g, [six], replicas=2, backend="host")
    with pytest.raises(ValueError, match="replicas >= 2"):
        motifs.motif_significance(g, replicas=1, backend="host")
    with pytest.raises(ValueError, match="unknown backend"):
        motifs.motif_significance(g, replicas=2, backend="gpu")
    with pytest.raises(ValueError, match="unknown backend"):
        motifs.rewire(g, backend="vf2")
    with pytest.raises(ValueError, match="negative"):
        motifs.rewire(g, replicas=-1, backend="host")
    with pytest.raises(RuntimeError, match="connected"):                # a disconnected query: the plan names the reason
        motifs.motif_significance(g, [(4, [(0, 1), (2, 3)])], replicas=2, backend="host")
    sets, acc = motifs.rewire(g, replicas=0, backend="host")
    assert sets == [] and acc.shape == (0, 1)


def test_driver_writes_both_tables(tmp_path, capsys):
    import motif_significance as D
    argv = ["--datasets", "MUTAG", "--replicas", "3", "--swaps_per_edge", "2", "--seed", "4", "--query_size", "3", "4",
            "--backend", "host", "--output_dir", str(tmp_path), "--data_root", str(tmp_path / "none")]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = D.main(argv)
        from desco_amd.data import load_data
        gs = load_data("MUTAG", root_folder=str(tmp_path / "none"))
    assert os.path.basename(out["graphs"]) == "motif-zscores_0.csv"
    assert os.path.basename(out["dataset"]) == "motif-zscores-dataset_0.csv"
    queries = [(k, tuple(e)) for k in (3, 4) for _, e in census_classes(k)]
    res = motifs.motif_significance(gs, queries, replicas=3, swaps_per_edge=2, seed=4, backend="host")
    with open(out["graphs"], newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["", "dataset", "graph", "query", "query_nodes", "query_edges", "real", "mean", "std", "z",
                       "profile", "p_over", "p_under"]
    assert len(rows) == 1 + gs.num_graphs * 8 and {r[1] for r in rows[1:]} == {"MUTAG"}
    k = 8 * 5 + 3                                                         # graph 5, query 3
    assert rows[1 + k][:5] == [str(k), "MUTAG", "5", "3", "4"] and int(rows[1 + k][6]) == res.real[5, 3]
    assert float(rows[1 + k][7]) == res.mean[5, 3] and float(rows[1 + k][11]) == res.p_over[5, 3]
    with open(out["dataset"], newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["", "dataset", "query", "query_nodes", "query_edges", "real", "mean", "std", "z", "profile",
                       "p_over", "p_under"]
    assert len(rows) == 9 and [int(r[5]) for r in rows[1:]] == res.dataset_real.tolist()
    assert [float(r[8]) for r in rows[1:]] == pytest.approx(res.dataset_z.tolist(), nan_ok=True)
    assert "MUTAG: %d graphs" % gs.num_graphs in capsys.readouterr().out
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        again = D.main(argv + ["--noninduced"])
    assert os.path.basename(again["graphs"]) == "motif-zscores_1.csv"
    assert sorted(os.listdir(tmp_path)) == ["motif-zscores-dataset_0.csv", "motif-zscores-dataset_1.csv",
                                            "motif-zscores_0.csv", "motif-zscores_1.csv"]
