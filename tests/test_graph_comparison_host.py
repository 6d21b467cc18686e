"""Graphlet correlation matrices and distances, the host twin (csrc/graphlet_correlation.cpp) and desco_amd.comparison,
against the numpy / scipy restatement in graph_comparison_reference.py.  No GPU."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph_comparison_reference as ref  # noqa: E402
from helpers import golden_graphs  # noqa: E402

from desco_amd import _lib  # noqa: E402
from desco_amd import comparison as cmp  # noqa: E402
from desco_amd import groundtruth as gt  # noqa: E402
from desco_amd.graphs import GraphSet  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _twin(X, dummy_row=True, seg=None, columns=None, threads=0):
    X = np.ascontiguousarray(X, dtype=np.int64)
    seg = np.array([0, X.shape[0]], dtype=np.int64) if seg is None else np.asarray(seg, dtype=np.int64)
    columns = np.arange(X.shape[1], dtype=np.int32) if columns is None else np.asarray(columns, dtype=np.int32)
    return cmp._gcm_host(X, seg, columns, dummy_row, threads)


@pytest.fixture(scope="module")
def golden():
    return GraphSet.from_edge_lists(golden_graphs(max_n=40)[:10])


@pytest.fixture(scope="module")
def golden_gcm(golden):
    return cmp.graphlet_correlation(golden, "all4", backend="host")


@pytest.mark.parametrize("n", [1, 2, 3, 5, 17, 64, 100])
def test_doubled_ranks_are_twice_rankdata(n):
    """d itself, through the ABI: an indicator column e_i has d = n' e_i - 1, and every column of D sums to 0, so
    S[a][e_i] = n' d[i][a].  (No dummy row: the indicators are the table's last n columns.)"""
    rng = np.random.default_rng(n)
    X = ref.random_table(rng, n, 10)
    S, _ = _twin(np.hstack([X, np.eye(n, dtype=np.int64)]), dummy_row=False)
    D = ref.doubled_ranks(X)
    assert (D.sum(axis=0) == 0).all()
    got = S[0][:10, 10:].T
    if n == 1:
        assert (S[0] == 0).all()                       # one row: every column is constant, d = 0
    else:
        assert (got % n == 0).all()
        assert np.array_equal(got // n, D)


@pytest.mark.parametrize("dummy_row", [True, False])
@pytest.mark.parametrize("n", [2, 3, 31, 32, 33, 200, 801])
def test_matrix_is_the_int64_product_and_rho_is_spearman(n, dummy_row):
    rng = np.random.default_rng(100 + n)
    X = ref.random_table(rng, n, 15)
    S, rho = _twin(X, dummy_row, threads=3)
    D, S_ref, rho_ref = ref.segment(X, dummy_row)
    assert S.dtype == np.int64 and np.array_equal(S[0], S_ref)
    assert np.array_equal(rho[0], rho_ref)             # the definition's operations, bit for bit
    if n + dummy_row < 3:                              # scipy's matrix starts at three rows
        return
    sp = ref.spearman(X, dummy_row)
    both = ~np.isnan(sp)
    err = np.abs(rho[0] - sp)[both].max()
    print(f"[gcm] n' = {n + dummy_row}: worst |rho - scipy| = {err:.3e} over {int(both.sum())} entries")
    assert both.sum() > 15 and err <= 1e-12
    varies = np.diag(S_ref) != 0
    assert np.array_equal(both, varies[:, None] & varies[None, :])    # scipy's NaNs are exactly the constant columns


@pytest.mark.parametrize("dummy_row", [True, False])
def test_constant_columns(dummy_row):
    rng = np.random.default_rng(5)
    X = ref.random_table(rng, 20, 6)
    X[:, 0], X[:, 1], X[:, 2] = 0, 1, 9                # zeros: varies only with the dummy row; ones: constant always
    _, rho = _twin(X, dummy_row)
    const = [1] if dummy_row else [0, 1, 2]
    for c in range(6):
        assert rho[0][c, c] == 1.0
    for c in const:
        off = np.delete(rho[0][c], c)
        assert (off == 0.0).all() and (np.delete(rho[0][:, c], c) == 0.0).all()
    assert not np.isnan(rho).any()
    if dummy_row:
        assert rho[0][0, 2] == -1.0                    # zeros below the dummy row against nines above it


def test_tiny_segments_and_thread_counts():
    rng = np.random.default_rng(9)
    X = ref.random_table(rng, 40, 11)
    seg = np.array([0, 1, 3, 3, 10, 40], dtype=np.int64)          # 1 row, 2 rows, none, 7, 30
    for dummy_row in (True, False):
        S, rho = _twin(X, dummy_row, seg, threads=1)
        S8, rho8 = _twin(X, dummy_row, seg, threads=8)
        assert np.array_equal(S, S8) and np.array_equal(rho, rho8)
        for s in range(5):
            _, S_ref, rho_ref = ref.segment(X[seg[s]:seg[s + 1]], dummy_row)
            assert np.array_equal(S[s], S_ref) and np.array_equal(rho[s], rho_ref)
        if not dummy_row:
            assert (S[0] == 0).all() and (S[2] == 0).all() and np.array_equal(rho[2], np.eye(11))


def test_edgeless_graph_and_empty_set():
    g = GraphSet.from_edge_lists([(5, []), (1, []), (4, [(0, 1), (1, 2), (2, 3)])])
    r = cmp.graphlet_correlation(g, "gcd11", backend="host")
    assert cmp.last_backend == "host" and r.S.shape == (3, 11, 11) and r.vector().shape == (3, 55)
    # all counts 0 under a dummy row of ones: every column has the same two-level ranks, every rho is 1
    assert (r.S[0] == 30).all() and (r.S[1] == 2).all() and (r.rho[0] == 1.0).all() and (r.rho[1] == 1.0).all()
    bare = cmp.graphlet_correlation(g, "gcd11", backend="host", dummy_row=False)
    assert (bare.S[0] == 0).all() and np.array_equal(bare.rho[0], np.eye(11))           # without it: all constant
    d = cmp.gcd(r, backend="host")
    assert d[0, 1] == 0.0 and d[0, 2] > 0.0
    empty = GraphSet.from_edge_lists([])
    e = cmp.graphlet_correlation(empty, "gcd11", backend="host")
    assert e.S.shape == (0, 11, 11) and e.vector().shape == (0, 55)
    assert cmp.gcd(e, r, backend="host").shape == (0, 3) and cmp.gcd(r, e, backend="host").shape == (3, 0)


def test_relabelling_changes_nothing(golden):
    rng = np.random.default_rng(3)
    lists = golden.edge_lists()
    shuffled = []
    for n, edges in lists:
        p = rng.permutation(n)
        shuffled.append((n, [(int(p[a]), int(p[b])) for a, b in edges]))
    a = cmp.graphlet_correlation(golden, "all5", backend="host")
    b = cmp.graphlet_correlation(GraphSet.from_edge_lists(shuffled), "all5", backend="host")
    assert np.array_equal(a.S, b.S) and np.array_equal(a.rho.view(np.int64), b.rho.view(np.int64))
    d = cmp.gcd(a, b, backend="host")
    assert (np.diag(d) == 0.0).all() and (d[~np.eye(len(lists), dtype=bool)] > 0).any()


def test_gcd_is_the_fma_chain_and_symmetric(golden_gcm):
    x = golden_gcm.vector()
    rng = np.random.default_rng(4)
    y = rng.uniform(-1, 1, (7, x.shape[1]))
    d = cmp.gcd(x, y, backend="host", num_threads=3)
    assert cmp.last_backend == "host" and d.shape == (len(x), 7)
    assert np.array_equal(d.view(np.int64), cmp.gcd(y, x, backend="host").T.copy().view(np.int64))
    assert np.array_equal(d.view(np.int64), ref.gcd_matrix(x, y).view(np.int64))
    self_d = cmp.gcd(golden_gcm, backend="host")
    assert np.array_equal(self_d, self_d.T) and (np.diag(self_d) == 0).all()
    assert np.array_equal(self_d.view(np.int64), ref.gcd_matrix(x, x).view(np.int64))
    # a strided view: only its elements are written
    parent = np.full((len(x) + 2, 12), np.nan)
    cmp._gcd_host(x, y, out=parent[1:-1, 2:9])
    assert np.array_equal(parent[1:-1, 2:9].view(np.int64), d.view(np.int64))
    keep = np.ones(parent.shape, dtype=bool)
    keep[1:-1, 2:9] = False
    assert np.isnan(parent[keep]).all()


def test_column_sets_are_structural():
    flat, cols = gt._orbit_queries(None), gt.orbit_columns()
    assert len(cols) == 73
    all5, all4, gcd11 = cmp.orbit_set("all5"), cmp.orbit_set("all4"), cmp.orbit_set("gcd11")
    assert np.array_equal(all5, np.arange(73)) and np.array_equal(all4, np.arange(15))
    dropped = sorted(set(all4.tolist()) - set(gcd11.tolist()))
    shapes = [(flat[cols[c][0]][0], len(flat[cols[c][0]][1])) for c in dropped]
    assert shapes == [(3, 3), (4, 5), (4, 5), (4, 6)]           # the triangle, the diamond's two orbits, K4
    assert len(gcd11) == 11 and set(gcd11.tolist()) <= set(all4.tolist())
    assert np.array_equal(cmp.orbit_set([5, 3, 70]), np.array([5, 3, 70], dtype=np.int32))
    with pytest.raises(ValueError):
        cmp.orbit_set("gcd12")
    with pytest.raises(ValueError):
        cmp.orbit_set([73])


def test_api_matches_the_reference_on_graphs(golden, golden_gcm):
    table = gt.orbit_counts(golden, backend="host").numpy().astype(np.int64)
    assert np.array_equal(golden_gcm.columns, np.arange(15))
    for g in range(golden.num_graphs):
        a, b = golden.graph_ptr[g], golden.graph_ptr[g + 1]
        _, S_ref, rho_ref = ref.segment(table[a:b, :15], True)
        assert np.array_equal(golden_gcm.S[g], S_ref) and np.array_equal(golden_gcm.rho[g], rho_ref)
        assert np.array_equal(golden_gcm.vector()[g], ref.upper(rho_ref))
    sub = cmp.graphlet_correlation(golden, [14, 0, 40], backend="host", dummy_row=False)
    _, S_ref, _ = ref.segment(table[:golden.graph_ptr[1]][:, [14, 0, 40]], False)
    assert np.array_equal(sub.S[0], S_ref)
    non = cmp.graphlet_correlation(golden, "all4", induced=False, backend="host")
    tab_non = gt.orbit_counts(golden, backend="host", induced=False).numpy().astype(np.int64)
    assert np.array_equal(non.S[1], ref.segment(tab_non[golden.graph_ptr[1]:golden.graph_ptr[2], :15], True)[1])
    assert not np.array_equal(non.S, golden_gcm.S)


def test_explicit_segments_and_datasets(golden, golden_gcm):
    again = cmp.graphlet_correlation(golden, "all4", segments=golden.graph_ptr, backend="host")
    assert np.array_equal(again.S, golden_gcm.S)
    pairs = np.array([0, golden.graph_ptr[2], golden.graph_ptr[5], golden.num_nodes], dtype=np.int64)
    merged = cmp.graphlet_correlation(golden, "all4", segments=pairs, backend="host")
    whole = cmp.graphlet_correlation(golden.subset(2, 5), "all4", backend="host",
                                     segments=np.array([0, golden.subset(2, 5).num_nodes]))
    assert np.array_equal(merged.S[1], whole.S[0])
    sets = [golden.subset(0, 4), golden.subset(4, 10)]
    d = cmp.dataset_gcd(sets, backend="host", orbits="all4")
    assert d.shape == (2, 2) and d[0, 0] == 0 and d[0, 1] == d[1, 0] > 0
    one = cmp.graphlet_correlation(sets[1], "all4", backend="host", segments=[0, sets[1].num_nodes])
    zero = cmp.graphlet_correlation(sets[0], "all4", backend="host", segments=[0, sets[0].num_nodes])
    assert d[0, 1] == ref.gcd_chain(zero.vector()[0], one.vector()[0])
    with pytest.raises(ValueError):
        cmp.graphlet_correlation(golden, "all4", segments=[0, golden.num_nodes + 1], backend="host")


def test_nearest(golden_gcm):
    x = golden_gcm.vector()
    d = cmp.gcd(x, backend="host")
    for chunk in (3, 1000):
        idx, dist = cmp.nearest(x, x[:7], k=3, backend="host", chunk_rows=chunk)
        assert idx.shape == dist.shape == (7, 3)
        assert (dist[:, 0] == 0).all() and (idx[:, 0] <= np.arange(7)).all()       # itself, or an equal one before it
        order = np.argsort(d[:7], axis=1, kind="stable")[:, :3]
        assert np.array_equal(idx, order) and np.array_equal(dist, np.take_along_axis(d[:7], order, axis=1))
    with pytest.raises(ValueError):
        cmp.nearest(x, x, k=len(x) + 1, backend="host")
    with pytest.raises(ValueError):
        cmp.gcd(x, backend="hots")


def test_bad_arguments_are_refused_by_name():
    L = _lib.lib()
    X = np.arange(12, dtype=np.int64).reshape(4, 3)
    seg = np.array([0, 4], dtype=np.int64)
    cols = np.array([0, 2], dtype=np.int32)
    S = np.zeros((1, 2, 2), dtype=np.int64)
    rho = np.zeros((1, 2, 2), dtype=np.float64)
    p = lambda a: a.ctypes.data                                                          # noqa: E731

    def rejects(name, rc, word):
        msg = L.desco_last_error()
        assert rc == -1 and msg.startswith(name.encode() + b":") and word.encode() in msg, (name, rc, msg)
        assert L.desco_rng_next(None, None, None) == -1          # (another entry point's message in between)

    def host(seg=seg, nseg=1, X=p(X), ld=3, cols=p(cols), C=2, dummy=1, S=p(S), rho=p(rho)):
        return L.desco_graphlet_correlation(p(seg) if seg is not None else None, nseg, X, ld, cols, C, dummy, S, rho, 1)

    name = "desco_graphlet_correlation"
    assert host() == 0 and S[0, 0, 0] != 0
    before = S.copy()
    rejects(name, host(nseg=-1), "negative")
    rejects(name, host(ld=-3), "negative")
    rejects(name, host(C=-1), "DESCO_GCM_MAX_COLUMNS")
    rejects(name, host(C=129), "DESCO_GCM_MAX_COLUMNS")
    rejects(name, host(dummy=2), "dummy_row")
    rejects(name, host(seg=None), "seg_ptr is null")
    rejects(name, host(cols=None), "columns is null")
    rejects(name, host(X=None), "counts is null")
    rejects(name, host(cols=p(np.array([0, 3], dtype=np.int32))), "column index")
    rejects(name, host(cols=p(np.array([-1, 1], dtype=np.int32))), "column index")
    rejects(name, host(seg=np.array([-1, 4], dtype=np.int64)), "negative")
    rejects(name, host(seg=np.array([0, 3, 2], dtype=np.int64), nseg=2), "monotone")
    rejects(name, host(seg=np.array([0, 2097151], dtype=np.int64)), "2097151")       # n' = 2097152 with the dummy row
    assert np.array_equal(S, before)                                                 # refused before any write
    assert host(nseg=0) == 0 and host(C=0) == 0 and host(S=None, rho=None) == 0     # nothing to do
    assert host(S=None) == 0 and host(rho=None) == 0

    x = np.zeros((2, 3))
    out = np.zeros((2, 2))
    name = "desco_gcd_matrix"
    assert L.desco_gcd_matrix(p(x), 2, p(x), 2, 3, p(out), 2, 1) == 0
    rejects(name, L.desco_gcd_matrix(p(x), -1, p(x), 2, 3, p(out), 2, 1), "negative")
    rejects(name, L.desco_gcd_matrix(p(x), 2, p(x), 2, -3, p(out), 2, 1), "negative")
    rejects(name, L.desco_gcd_matrix(p(x), 2, p(x), 2, 3, p(out), 1, 1), "ldo")
    rejects(name, L.desco_gcd_matrix(p(x), 2, p(x), 2, 3, None, 2, 1), "out is null")
    rejects(name, L.desco_gcd_matrix(None, 2, p(x), 2, 3, p(out), 2, 1), "x or y is null")
    rejects(name, L.desco_gcd_matrix(p(x), 2, None, 2, 3, p(out), 2, 1), "x or y is null")
    assert L.desco_gcd_matrix(None, 0, None, 2, 3, None, 2, 1) == 0
    assert L.desco_gcd_matrix(None, 2, None, 2, 0, p(out), 2, 1) == 0 and (out == 0).all()   # P = 0: all distances 0


def test_device_entry_points_refuse_bad_arguments_before_any_launch():
    """The host-side checks of the two _dev entry points: each call is wrong in one way and comes back as DESCO_EINVAL
    naming the entry point, before any HIP call (fake aligned pointers, never dereferenced)."""
    L = _lib.lib()
    buf = np.zeros(64, dtype=np.int64)
    q = buf.ctypes.data
    cols = np.array([0, 2], dtype=np.int32)

    def rejects(name, rc, word):
        msg = L.desco_last_error()
        assert rc == -1 and msg.startswith(name.encode() + b":") and word.encode() in msg, (name, rc, msg)
        assert L.desco_rng_next(None, None, None) == -1

    def gcm(seg=q, nseg=1, rows=4, X=q, ld=3, cols=cols.ctypes.data, C=2, dummy=1, ids=None, nids=0, bound=5, work=q,
            S=q, rho=q, vec=q, status=q):
        return L.desco_graphlet_correlation_dev(seg, nseg, rows, X, ld, cols, C, dummy, ids, nids, bound, work, S, rho,
                                                vec, status, None)

    name = "desco_graphlet_correlation_dev"
    rejects(name, gcm(nseg=-1), "negative")
    rejects(name, gcm(rows=-1), "negative")
    rejects(name, gcm(bound=-1), "negative")
    rejects(name, gcm(C=129), "DESCO_GCM_MAX_COLUMNS")
    rejects(name, gcm(dummy=-1), "dummy_row")
    rejects(name, gcm(bound=20481), "DESCO_GCM_DEV_MAX_ROWS (20480)")
    rejects(name, gcm(seg=None), "seg_ptr is null")
    rejects(name, gcm(cols=None), "columns is null")
    rejects(name, gcm(work=None), "work is null")
    rejects(name, gcm(status=None), "status is null")
    rejects(name, gcm(X=None), "counts is null")
    rejects(name, gcm(S=q + 4), "8-byte aligned")
    rejects(name, gcm(cols=np.array([0, 3], dtype=np.int32).ctypes.data), "column index")
    assert gcm(nseg=0) == 0 and gcm(C=0) == 0 and gcm(ids=q, nids=0) == 0            # nothing to do

    name = "desco_gcd_matrix_dev"
    rejects(name, L.desco_gcd_matrix_dev(q, -1, q, 2, 3, q, 2, None), "negative")
    rejects(name, L.desco_gcd_matrix_dev(q, 2, q, 2, 3, q, 1, None), "ldo")
    rejects(name, L.desco_gcd_matrix_dev(q, 2, q, 2, 3, None, 2, None), "out is null")
    rejects(name, L.desco_gcd_matrix_dev(None, 2, q, 2, 3, q, 2, None), "x or y is null")
    rejects(name, L.desco_gcd_matrix_dev(q + 4, 2, q, 2, 3, q, 2, None), "8-byte aligned")
    rejects(name, L.desco_gcd_matrix_dev(q, 32 * 65536, q, 2, 3, q, 2, None), "rows of x")
    assert L.desco_gcd_matrix_dev(None, 0, None, 2, 3, None, 2, None) == 0


def test_ops_refuse_cpu_tables():
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cmp.graphlet_correlation_device(table=torch.zeros((4, 15), dtype=torch.int64), segments=[0, 4])


def test_selftest_program_under_the_host_sanitizers(tmp_path):
    """tools/graph_comparison_selftest.cpp with the twin, built with AddressSanitizer and UBSan, as its own program."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "graph_comparison_selftest")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fopenmp", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", os.path.join(ROOT, "tools", "graph_comparison_selftest.cpp"),
                            os.path.join(ROOT, "desco_amd", "csrc", "graphlet_correlation.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr


def test_driver_writes_both_tables(tmp_path):
    import csv
    import warnings
    import dataset_comparison
    argv = ["--train", "MUTAG_train", "--targets", "MUTAG_test", "MUTAG_val", "--k", "2", "--backend", "host",
            "--output_dir", str(tmp_path), "--data_root", str(tmp_path / "none")]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                     # (the stand-in data set announces itself)
        first = dataset_comparison.main(argv)
        second = dataset_comparison.main(argv + ["--orbits", "all4"])
    assert first["nearest_csv"].endswith("gcd-nearest_0.csv") and second["nearest_csv"].endswith("gcd-nearest_1.csv")
    assert second["datasets_csv"].endswith("gcd-datasets_1.csv")
    rows = list(csv.reader(open(first["nearest_csv"])))
    assert rows[0] == ["target_set", "target_graph", "rank", "train_graph", "distance"]
    assert len(rows) == 1 + 2 * (94 + 47) and rows[1][0] == "MUTAG_test" and rows[2][2] == "1"
    assert float(rows[1][4]) <= float(rows[2][4])
    sets = list(csv.reader(open(first["datasets_csv"])))
    assert sets[0] == ["set", "MUTAG_train", "MUTAG_test", "MUTAG_val"] and float(sets[1][1]) == 0.0
    assert float(sets[1][2]) == float(sets[2][1]) > 0.0
    assert first["targets"]["MUTAG_test"]["count"] == 94 and first["dataset_distances"].shape == (3, 3)
