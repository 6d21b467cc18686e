"""Graphlet degree distributions and their agreement, the host twin (csrc/graphlet_distribution.cpp) and
desco_amd.comparison, against the plain-Python restatement in gdd_reference.py.  No GPU."""
import itertools
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gdd_reference as ref  # noqa: E402
from helpers import golden_graphs  # noqa: E402

from desco_amd import _lib  # noqa: E402
from desco_amd import comparison as cmp  # noqa: E402
from desco_amd import groundtruth as gt  # noqa: E402
from desco_amd.graphs import GraphSet  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIQUE_ORBITS = [0, 3, 14, 72]                         # the edge's, the triangle's, K4's and K5's orbit among the 73


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def _twin(X, seg=None, columns=None, threads=0):
    X = np.ascontiguousarray(X, dtype=np.int64)
    seg = np.array([0, X.shape[0]], dtype=np.int64) if seg is None else np.asarray(seg, dtype=np.int64)
    columns = np.arange(X.shape[1], dtype=np.int32) if columns is None else np.asarray(columns, dtype=np.int32)
    return cmp.GraphletDistribution(*cmp._gdd_host(X, seg, columns, threads), seg, columns, None, "host")


def _check_lists(d, X):
    """Every list of ``d`` against the reference, and the slots behind it zero."""
    C = len(d.columns)
    for s in range(len(d)):
        a, n = int(d.seg[s]), int(d.seg[s + 1] - d.seg[s])
        got = d.lists(s)
        for c in range(C):
            keys, vals = ref.distribution(X[a:a + n, d.columns[c]])
            assert same(got[c][0], keys) and same(got[c][1], vals), (s, c)
            at = a * C + c * n
            assert (d.key[at + len(keys):at + n] == 0).all() and (d.val[at + len(keys):at + n] == 0).all()


@pytest.fixture(scope="module")
def golden():
    return GraphSet.from_edge_lists(golden_graphs(max_n=40)[:10])


@pytest.fixture(scope="module")
def golden_gdd(golden):
    return cmp.graphlet_distribution(golden, "all4", backend="host")


@pytest.mark.parametrize("n", [1, 2, 3, 31, 32, 33, 200, 801])
def test_lists_are_the_definition(n):
    X = ref.random_table(np.random.default_rng(100 + n), n, 12)
    d = _twin(X, threads=3)
    _check_lists(d, X)
    assert d.len[0, 0] == 0 and d.len[0, 1] == 1 and d.len[0, 3] == n        # empty, one entry, all distinct
    assert same(d.lists(0)[1][1], np.array([1.0]))


@pytest.mark.parametrize("kind", ["zeros", "constant", "ties", "distinct", "huge"])
def test_column_kinds(kind):
    rng = np.random.default_rng(7)
    sizes = [1, 2, 3, 40, 0, 64]
    seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    X = np.concatenate([ref.random_table(rng, n, 3, kind) for n in sizes])
    d = _twin(X, seg)
    _check_lists(d, X)
    if kind == "huge":                                  # above 2^53 the conversion rounds: (double)k is not k
        k = d.lists(3)[0][0]
        assert (k > (1 << 53)).all() and any(int(float(int(v))) != int(v) for v in k)


@pytest.mark.parametrize("C", [1, 15, 73, 128])
def test_column_counts_and_agreement_against_the_definition(C):
    rng = np.random.default_rng(C)
    sizes = [5, 0, 12, 1, 30, 12, 7]
    seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    X = np.concatenate([ref.random_table(rng, n, C) for n in sizes])
    X[seg[5]:seg[6]] = X[seg[2]:seg[3]][::-1]           # segment 5 = segment 2, rows reversed
    cols = rng.permutation(C).astype(np.int32)
    d = _twin(X, seg, cols)
    _check_lists(d, X)
    agree, per = cmp.gdd_agreement(d, per_orbit=True, backend="host", num_threads=3)
    assert cmp.last_backend == "host" and agree.shape == (7, 7) and per.shape == (7, 7, C)
    assert same(agree, agree.T.copy()) and same(per, per.transpose(1, 0, 2).copy())
    assert (np.diag(agree) == 1.0).all() and agree[2, 5] == 1.0 and (per[2, 5] == 1.0).all()
    lists = [d.lists(s) for s in range(7)]
    pairs = [(0, 2), (2, 4), (1, 3), (1, 4), (3, 0), (6, 4), (5, 6)] if C > 15 else list(itertools.product(range(7), range(7)))
    for i, j in pairs:
        want, want_per = ref.pair(lists[i], lists[j])
        assert agree[i, j] == want and per[i, j].tolist() == want_per, (i, j)
    plain = cmp.gdd_agreement(d, backend="host")
    assert same(plain, agree)


def test_thread_counts_give_the_same_bits():
    rng = np.random.default_rng(9)
    sizes = rng.integers(0, 40, 30)
    seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    X = np.concatenate([ref.random_table(rng, n, 15) for n in sizes])
    one = _twin(X, seg, threads=1)
    a1, p1 = cmp._gdda_host(one, one, True, 1)
    for t in (3, 16):
        d = _twin(X, seg, threads=t)
        assert same(d.len, one.len) and same(d.key, one.key) and same(d.val, one.val)
        a, p = cmp._gdda_host(d, d, True, t)
        assert same(a, a1) and same(p, p1)
    # a strided view: only its elements are written
    parent = np.full((34, 40), np.nan)
    cmp._gdda_host(one.rows(0, 30), one.rows(3, 20), False, 3, out=parent[2:32, 5:22])
    assert same(parent[2:32, 5:22], a1[:, 3:20])
    keep = np.ones(parent.shape, dtype=bool)
    keep[2:32, 5:22] = False
    assert np.isnan(parent[keep]).all()


def test_relabelling_changes_nothing(golden):
    rng = np.random.default_rng(3)
    shuffled = []
    for n, edges in golden.edge_lists():
        p = rng.permutation(n)
        shuffled.append((n, [(int(p[a]), int(p[b])) for a, b in edges]))
    a = cmp.graphlet_distribution(golden, "all5", backend="host")
    b = cmp.graphlet_distribution(GraphSet.from_edge_lists(shuffled), "all5", backend="host")
    assert same(a.len, b.len) and same(a.key, b.key) and same(a.val, b.val) and (a.len > 1).any()
    agree = cmp.gdd_agreement(a, b, backend="host")
    assert (np.diag(agree) == 1.0).all() and (agree < 1.0).any() and same(agree, cmp.gdd_agreement(a, backend="host"))


def test_disjoint_key_sets_have_a_closed_form():
    x, y = np.array([2, 2, 4, 6, 6, 6, 0]), np.array([1, 3, 3, 5, 7, 0, 0])
    X = np.concatenate([x, y]).reshape(-1, 1)
    d = _twin(X, np.array([0, 7, 14]))
    (kx, nx), (ky, ny) = d.lists(0)[0], d.lists(1)[0]
    assert kx.tolist() == [2, 4, 6] and ky.tolist() == [1, 3, 5, 7]
    acc = 0.0
    for _, v in sorted(list(zip(kx, nx)) + list(zip(ky, ny))):                # sum N_x^2 + sum N_y^2 in chain order
        acc = ref.fma(float(v), float(v), acc)
    agree, per = cmp.gdd_agreement(d, per_orbit=True, backend="host")
    assert per[0, 1, 0] == 1.0 - math.sqrt(0.5 * acc) == agree[0, 1] == agree[1, 0]


def _complete(n):
    return (n, list(itertools.combinations(range(n), 2)))


@pytest.mark.parametrize("a,b", [(20, 32), (5, 9), (6, 9)])
def test_complete_graphs_of_different_sizes(a, b):
    """What the feature is for: the correlation distance of K_a and K_b is 0, their agreement is not 1."""
    g = GraphSet.from_edge_lists([_complete(a), _complete(b)])
    d = cmp.graphlet_distribution(g, "all5", backend="host")
    for s, n in enumerate((a, b)):
        for c, (k, v) in enumerate(d.lists(s)):
            if c in CLIQUE_ORBITS:                       # every node lies in C(n - 1, j - 1) cliques of j nodes
                j = CLIQUE_ORBITS.index(c) + 2
                assert k.tolist() == [math.comb(n - 1, j - 1)] and v.tolist() == [1.0]
            else:
                assert len(k) == 0
    agree, per = cmp.gdd_agreement(d, per_orbit=True, backend="host")
    want = np.ones(73)
    want[CLIQUE_ORBITS] = 0.0
    assert same(per[0, 1], want)
    total = 0.0
    for _ in range(69):
        total = total + 1.0
    assert agree[0, 1] == total / 73.0 == agree[1, 0] and agree[0, 0] == 1.0
    non = cmp.graphlet_distribution(g, "all5", induced=False, backend="host")
    assert (non.len == 1).all()
    agree_non, per_non = cmp.gdd_agreement(non, per_orbit=True, backend="host")
    assert (per_non[0, 1] == 0.0).all() and agree_non[0, 1] == 0.0 and agree_non[1, 1] == 1.0
    assert cmp.gdd_agreement(d, mean="geometric", backend="host")[0, 1] == 0.0
    bare = cmp.gcd(cmp.graphlet_correlation(g, "all5", dummy_row=False, backend="host"), backend="host")
    gcd = cmp.gcd(cmp.graphlet_correlation(g, "all5", backend="host"), backend="host")
    assert bare[0, 1] == 0.0
    # under the dummy row of ones too, from six nodes on: every node of K5 lies in ONE 5-clique, the dummy row's value,
    # so that column of K5 is constant where K_b's is not
    assert (gcd[0, 1] == 0.0) == (a > 5)


def test_edgeless_graph_empty_set_and_segments(golden, golden_gdd):
    g = GraphSet.from_edge_lists([(5, []), (1, []), (4, [(0, 1), (1, 2), (2, 3)])])
    d = cmp.graphlet_distribution(g, "all4", backend="host")
    assert cmp.last_backend == "host" and d.len.shape == (3, 15) and d.key.shape == (150,)
    assert (d.len[:2] == 0).all() and (d.key[:90] == 0).all() and d.len[2, 0] == 2
    agree = cmp.gdd_agreement(d, backend="host")
    assert agree[0, 1] == 1.0 and agree[0, 2] < 1.0                               # two empty distributions agree
    empty = cmp.graphlet_distribution(GraphSet.from_edge_lists([]), "all4", backend="host")
    assert empty.len.shape == (0, 15) and len(empty) == 0
    assert cmp.gdd_agreement(empty, d, backend="host").shape == (0, 3)
    assert cmp.gdd_agreement(d, empty, backend="host").shape == (3, 0)
    again = cmp.graphlet_distribution(golden, "all4", segments=golden.graph_ptr, backend="host")
    assert same(again.len, golden_gdd.len) and same(again.val, golden_gdd.val)
    pairs = np.array([0, golden.graph_ptr[2], golden.graph_ptr[5], golden.num_nodes], dtype=np.int64)
    merged = cmp.graphlet_distribution(golden, "all4", segments=pairs, backend="host")
    sub = golden.subset(2, 5)
    whole = cmp.graphlet_distribution(sub, "all4", backend="host", segments=np.array([0, sub.num_nodes]))
    for (k, v), (k2, v2) in zip(merged.lists(1), whole.lists(0)):
        assert same(k, k2) and same(v, v2)
    sets = [golden.subset(0, 4), golden.subset(4, 10)]
    a = cmp.dataset_gdda(sets, backend="host", orbits="all4")
    assert a.shape == (2, 2) and a[0, 0] == 1.0 and a[1, 1] == 1.0 and 0.0 < a[0, 1] == a[1, 0] < 1.0
    zero = cmp.graphlet_distribution(sets[0], "all4", backend="host", segments=[0, sets[0].num_nodes])
    one = cmp.graphlet_distribution(sets[1], "all4", backend="host", segments=[0, sets[1].num_nodes])
    assert a[0, 1] == ref.pair(zero.lists(0), one.lists(0))[0]
    with pytest.raises(ValueError):
        cmp.graphlet_distribution(golden, "all4", segments=[0, golden.num_nodes + 1], backend="host")
    with pytest.raises(ValueError):
        cmp.graphlet_distribution(golden, [], backend="host")
    with pytest.raises(ValueError):
        cmp.gdd_agreement(golden_gdd, cmp.graphlet_distribution(golden, "all5", backend="host"), backend="host")


def test_api_matches_the_reference_on_graphs(golden, golden_gdd):
    table = gt.orbit_counts(golden, backend="host").numpy().astype(np.int64)
    assert np.array_equal(golden_gdd.columns, np.arange(15)) and np.array_equal(golden_gdd.seg, golden.graph_ptr)
    _check_lists(golden_gdd, table)
    non = cmp.graphlet_distribution(golden, "all4", induced=False, backend="host")
    _check_lists(non, gt.orbit_counts(golden, backend="host", induced=False).numpy().astype(np.int64))
    assert not same(non.val, golden_gdd.val)


def test_geometric_mean(golden_gdd):
    """exp(mean(log A_c)): three operations of an ulp or so per term over at most 128 terms, 3e-14 at the most."""
    agree, per = cmp.gdd_agreement(golden_gdd, mean="geometric", per_orbit=True, backend="host", chunk_rows=3)
    arith, per2 = cmp.gdd_agreement(golden_gdd, per_orbit=True, backend="host")
    assert same(per, per2) and agree.shape == arith.shape
    worst = 0.0
    for i in range(len(golden_gdd)):
        for j in range(len(golden_gdd)):
            want = ref.geometric(per[i, j].tolist())
            worst = max(worst, abs(agree[i, j] - want) / want if want else abs(agree[i, j]))
    print(f"[gdd] geometric mean: worst relative difference to the reference {worst:.3e}")
    assert worst <= 1e-12
    assert (agree <= arith + 1e-15).all() and (np.diag(agree) == 1.0).all()
    assert same(cmp.gdd_agreement(golden_gdd, mean="geometric", backend="host"), agree)
    with pytest.raises(ValueError):
        cmp.gdd_agreement(golden_gdd, mean="harmonic", backend="host")


def test_nearest_order_and_ties(golden_gdd):
    a = cmp.gdd_agreement(golden_gdd, backend="host")
    for chunk in (3, 1000):
        idx, val = cmp.gdd_nearest(golden_gdd, golden_gdd.rows(0, 7), k=3, backend="host", chunk_rows=chunk)
        assert idx.shape == val.shape == (7, 3) and (val[:, 0] == 1.0).all()
        order = np.argsort(-a[:7], axis=1, kind="stable")[:, :3]
        assert np.array_equal(idx, order) and same(val, np.take_along_axis(a[:7], order, axis=1))
        assert (np.diff(val, axis=1) <= 0).all()
    # ties: three copies of one graph among the training segments come back in ascending index
    X = np.array([[1], [2], [2], [5], [1], [2], [2], [9], [9], [1], [2], [2]], dtype=np.int64)
    d = _twin(X, np.array([0, 3, 4, 7, 9, 12]))
    idx, val = cmp.gdd_nearest(d, d.rows(0, 1), k=4, backend="host")
    assert idx[0].tolist()[:3] == [0, 2, 4] and (val[0, :3] == 1.0).all() and val[0, 3] < 1.0
    with pytest.raises(ValueError):
        cmp.gdd_nearest(d, d, k=6, backend="host")
    with pytest.raises(ValueError):
        cmp.gdd_nearest(d, d, backend="hots")


def test_bad_arguments_are_refused_by_name():
    L = _lib.lib()
    X = np.arange(12, dtype=np.int64).reshape(4, 3)
    seg = np.array([0, 4], dtype=np.int64)
    cols = np.array([0, 2], dtype=np.int32)
    ln = np.full((1, 2), -7, dtype=np.int32)
    key = np.full(8, -7, dtype=np.int64)
    val = np.full(8, -7.0)
    p = lambda a: a.ctypes.data                                                          # noqa: E731

    def rejects(name, rc, word):
        msg = L.desco_last_error()
        assert rc == -1 and msg.startswith(name.encode() + b":") and word.encode() in msg, (name, rc, msg)
        assert L.desco_rng_next(None, None, None) == -1          # (another entry point's message in between)

    def build(seg=seg, nseg=1, X=p(X), ld=3, cols=p(cols), C=2, ln=p(ln), key=p(key), val=p(val)):
        return L.desco_gdd_build(p(seg) if seg is not None else None, nseg, X, ld, cols, C, ln, key, val, 1)

    name = "desco_gdd_build"
    rejects(name, build(nseg=-1), "negative")
    rejects(name, build(ld=-3), "negative")
    rejects(name, build(C=0), "DESCO_GCM_MAX_COLUMNS")
    rejects(name, build(C=129), "DESCO_GCM_MAX_COLUMNS")
    rejects(name, build(seg=None), "seg_ptr is null")
    rejects(name, build(cols=None), "columns is null")
    rejects(name, build(ln=None), "len is null")
    rejects(name, build(X=None), "counts is null")
    rejects(name, build(key=None), "key or val is null")
    rejects(name, build(val=None), "key or val is null")
    rejects(name, build(cols=p(np.array([0, 3], dtype=np.int32))), "column index")
    rejects(name, build(cols=p(np.array([-1, 1], dtype=np.int32))), "column index")
    rejects(name, build(seg=np.array([-1, 4], dtype=np.int64)), "negative")
    rejects(name, build(seg=np.array([0, 3, 2], dtype=np.int64), nseg=2), "monotone")
    assert (ln == -7).all() and (key == -7).all() and (val == -7.0).all()            # refused before any write
    assert build(nseg=0) == 0 and (ln == -7).all()
    assert build() == 0 and ln.tolist() == [[3, 4]] and key.tolist() == [3, 6, 9, 0, 2, 5, 8, 11]

    out = np.full((1, 1), -3.0)

    y_key, y_val = p(key), p(val)

    def agree(seg=seg, ln=p(ln), key=p(key), val=p(val), Gx=1, Gy=1, C=2, out=p(out), ldo=1, other=ln):
        seg = p(seg) if seg is not None else None          # x: the arguments; y: the same segment with the lens `other`
        return L.desco_gdd_agreement(seg, ln, key, val, Gx, seg, p(other), y_key, y_val, Gy, C, out, ldo, None, 1)

    name = "desco_gdd_agreement"
    rejects(name, agree(Gx=-1), "negative")
    rejects(name, agree(Gy=-1), "negative")
    rejects(name, agree(C=0), "DESCO_GCM_MAX_COLUMNS")
    rejects(name, agree(C=129), "DESCO_GCM_MAX_COLUMNS")
    rejects(name, agree(ldo=0), "ldo")
    rejects(name, agree(out=None), "agree is null")
    rejects(name, agree(seg=None), "seg_ptr is null")
    rejects(name, agree(ln=None), "len is null")
    rejects(name, agree(key=None), "key or val is null")
    rejects(name, agree(val=None), "key or val is null")
    rejects(name, agree(seg=np.array([-1, 4], dtype=np.int64)), "negative")
    rejects(name, agree(seg=np.array([4, 0], dtype=np.int64)), "monotone")
    rejects(name, agree(other=np.array([[5, 0]], dtype=np.int32)), "len is outside")
    rejects(name, agree(ln=p(np.array([[0, -1]], dtype=np.int32))), "len is outside")
    assert out[0, 0] == -3.0                                                          # refused before any write
    assert agree(Gx=0) == 0 and agree(Gy=0) == 0 and out[0, 0] == -3.0               # nothing to do
    assert agree() == 0 and out[0, 0] == 1.0


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

    def build(seg=q, nseg=1, rows=4, X=q, ld=3, cols=cols.ctypes.data, C=2, ids=None, nids=0, bound=5, ln=q, key=q,
              val=q, status=q):
        return L.desco_gdd_build_dev(seg, nseg, rows, X, ld, cols, C, ids, nids, bound, ln, key, val, status, None)

    name = "desco_gdd_build_dev"
    rejects(name, build(nseg=-1), "negative")
    rejects(name, build(rows=-1), "negative")
    rejects(name, build(bound=-1), "negative")
    rejects(name, build(ids=q, nids=-1), "negative")
    rejects(name, build(C=0), "DESCO_GCM_MAX_COLUMNS")
    rejects(name, build(C=129), "DESCO_GCM_MAX_COLUMNS")
    rejects(name, build(bound=20481), "DESCO_GCM_DEV_MAX_ROWS (20480)")
    rejects(name, build(seg=None), "seg_ptr is null")
    rejects(name, build(cols=None), "columns is null")
    rejects(name, build(ln=None), "len is null")
    rejects(name, build(status=None), "status is null")
    rejects(name, build(X=None), "counts is null")
    rejects(name, build(key=None), "key or val is null")
    rejects(name, build(val=None), "key or val is null")
    rejects(name, build(key=q + 4), "8-byte aligned")
    rejects(name, build(cols=np.array([0, 3], dtype=np.int32).ctypes.data), "column index")
    assert build(nseg=0) == 0 and build(ids=q, nids=0) == 0                          # nothing to do

    def agree(xs=q, xl=q, xk=q, xv=q, Gx=2, ys=q, yl=q, yk=q, yv=q, Gy=2, C=3, out=q, ldo=2, per=None):
        return L.desco_gdd_agreement_dev(xs, xl, xk, xv, Gx, ys, yl, yk, yv, Gy, C, out, ldo, per, None)

    name = "desco_gdd_agreement_dev"
    rejects(name, agree(Gx=-1), "negative")
    rejects(name, agree(Gy=-1), "negative")
    rejects(name, agree(C=0), "DESCO_GCM_MAX_COLUMNS")
    rejects(name, agree(C=129), "DESCO_GCM_MAX_COLUMNS")
    rejects(name, agree(ldo=1), "ldo")
    rejects(name, agree(out=None), "agree is null")
    rejects(name, agree(xs=None), "seg_ptr is null")
    rejects(name, agree(ys=None), "seg_ptr is null")
    rejects(name, agree(xl=None), "len is null")
    rejects(name, agree(yl=None), "len is null")
    rejects(name, agree(xk=q + 4), "8-byte aligned")
    rejects(name, agree(per=q + 4), "8-byte aligned")
    rejects(name, agree(Gx=32 * 65536), "segments of x")
    assert agree(Gx=0) == 0 and agree(Gy=0) == 0


def test_ops_refuse_cpu_tensors(golden_gdd):
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cmp.graphlet_distribution_device(table=torch.zeros((4, 15), dtype=torch.int64), orbits="all4", segments=[0, 4])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cmp.graphlet_distribution_device(table=np.zeros((4, 15), dtype=np.int64), orbits="all4", segments=[0, 4])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cmp.gdd_agreement_device(golden_gdd)
    assert cmp.AUTO_DEVICE.keys() >= {"gdd", "gdda"}


def test_selftest_program_under_the_host_sanitizers(tmp_path):
    """tools/gdd_selftest.cpp with the twin, built with AddressSanitizer and UBSan, as its own program."""
    cxx = shutil.which("g++")
    assert cxx is not None, "the selftest needs g++"
    exe = str(tmp_path / "gdd_selftest")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fopenmp", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", os.path.join(ROOT, "tools", "gdd_selftest.cpp"),
                            os.path.join(ROOT, "desco_amd", "csrc", "graphlet_distribution.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr


def test_driver_writes_four_tables_and_the_default_run_is_unchanged(tmp_path):
    import csv
    import warnings
    sys.path.insert(0, ROOT)
    import dataset_comparison
    argv = ["--train", "MUTAG_train", "--targets", "MUTAG_test", "MUTAG_val", "--k", "2", "--backend", "host",
            "--output_dir", str(tmp_path), "--data_root", str(tmp_path / "none")]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                     # (the stand-in data set announces itself)
        plain = dataset_comparison.main(argv)
        both = dataset_comparison.main(argv + ["--measure", "both"])
        only = dataset_comparison.main(argv + ["--measure", "gdda", "--orbits", "all4"])
    assert sorted(plain) == ["dataset_distances", "datasets_csv", "nearest_csv", "targets"]
    assert plain["nearest_csv"].endswith("gcd-nearest_0.csv") and plain["datasets_csv"].endswith("gcd-datasets_0.csv")
    # <i> is the first number free for every table a run writes: 1 for the four of "both", 0 again for the two of "gdda"
    assert sorted(os.listdir(tmp_path)) == ["gcd-datasets_0.csv", "gcd-datasets_1.csv", "gcd-nearest_0.csv",
                                            "gcd-nearest_1.csv", "gdda-datasets_0.csv", "gdda-datasets_1.csv",
                                            "gdda-nearest_0.csv", "gdda-nearest_1.csv"]
    assert open(plain["nearest_csv"]).read() == open(both["nearest_csv"]).read()       # the same GCD tables beside it
    assert open(plain["datasets_csv"]).read() == open(both["datasets_csv"]).read()
    assert both["gdda_nearest_csv"].endswith("gdda-nearest_1.csv") and only["gdda_datasets_csv"].endswith("_0.csv")
    assert sorted(only) == ["dataset_agreements", "gdda_datasets_csv", "gdda_nearest_csv", "gdda_targets"]
    rows = list(csv.reader(open(both["gdda_nearest_csv"])))
    assert rows[0] == ["target_set", "target_graph", "rank", "train_graph", "agreement"]
    assert len(rows) == 1 + 2 * (94 + 47) and rows[1][0] == "MUTAG_test" and rows[2][2] == "1"
    assert 1.0 >= float(rows[1][4]) >= float(rows[2][4]) >= 0.0
    sets = list(csv.reader(open(both["gdda_datasets_csv"])))
    assert sets[0] == ["set", "MUTAG_train", "MUTAG_test", "MUTAG_val"] and float(sets[1][1]) == 1.0
    assert 0.0 < float(sets[1][2]) == float(sets[2][1]) < 1.0
    assert both["gdda_targets"]["MUTAG_test"]["count"] == 94 and both["dataset_agreements"].shape == (3, 3)
