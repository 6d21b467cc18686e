"""Graphlet correlation on the MI355X (csrc/graphlet_correlation_dev.hip) against the host twin
(csrc/graphlet_correlation.cpp): the integer matrix S and the squared distances bit for bit; rho, the vectors and the
distances bit for bit as well (the definition's operations are single correctly rounded ones on both sides)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph_comparison_reference as ref  # noqa: E402
from helpers import golden_graphs  # noqa: E402

from desco_amd import comparison as cmp  # noqa: E402
from desco_amd import generators  # noqa: E402
from desco_amd.graphs import GraphSet  # noqa: E402

pytestmark = pytest.mark.gpu

MAX = cmp.DEVICE_MAX_ROWS
# n' of the synthetic segments (dummy row included): the smallest, around the matrix kernel's chunk of 32 rows, around
# the wave (64 rows a step of the rank kernel), around DESCO_GCM_WAVE_ROWS, around the 256-thread step
SIZES = [1, 2, 3, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 513, 801]


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int64) if a.dtype == np.float64 else a


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def _table(sizes, C, seed, dummy_row=True, kind="mixed"):
    rng = np.random.default_rng(seed)
    rows = [n - int(dummy_row) for n in sizes]
    seg = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    X = np.concatenate([ref.random_table(rng, n, C, kind) for n in rows]) if sum(rows) else np.zeros((0, C), np.int64)
    return X, seg


def _both(X, seg, columns, dummy_row=True, **kw):
    columns = np.asarray(columns, dtype=np.int32)
    S, rho = cmp._gcm_host(X, seg, columns, dummy_row, 0)
    dev = cmp._gcm_device(torch.from_numpy(X).cuda(), seg, columns, dummy_row, **kw)
    return S, rho, dev


@pytest.fixture(scope="module")
def graphs():
    lists = list(golden_graphs(max_n=40))[:12]
    fam = np.repeat(np.arange(6), 3)
    n = np.array([9, 20, 33] * 6)
    lists += generators.generate(fam, n, (n * np.array([1.2, 2.0, 3.0] * 6)).astype(np.int64), seed=5,
                                 backend="host").edge_lists()
    lists += [(1, []), (2, [(0, 1)]), (6, [])]
    return GraphSet.from_edge_lists(lists)


@pytest.mark.parametrize("orbits", ["gcd11", "all4", "all5"])
def test_graphs_device_equals_twin(graphs, orbits):
    host = cmp.graphlet_correlation(graphs, orbits, backend="host")
    dev = cmp.graphlet_correlation(graphs, orbits, backend="device")
    assert cmp.last_backend == "device" and dev.S.shape == host.S.shape
    assert same(dev.S, host.S) and (host.S != 0).any()
    assert same(dev.rho, host.rho) and same(dev.vector(), host.vector())
    assert (dev.status == 0).all()
    on_gpu = cmp.graphlet_correlation_device(graphs, orbits)
    assert on_gpu.S.is_cuda and same(on_gpu.S, host.S) and same(on_gpu.vector(), host.vector())
    d_host = cmp.gcd(host, backend="host")
    assert same(cmp.gcd(dev, backend="device"), d_host) and cmp.last_backend == "device"
    assert same(cmp.gcd_device(on_gpu), d_host)
    idx, dist = cmp.nearest(host, host, k=3, backend="host")
    idx_d, dist_d = cmp.nearest(on_gpu, on_gpu, k=3, backend="device", chunk_rows=7)
    assert np.array_equal(idx, idx_d) and same(dist, dist_d)
    non = cmp.graphlet_correlation(graphs, orbits, induced=False, backend="host")
    assert same(cmp.graphlet_correlation(graphs, orbits, induced=False, backend="device").S, non.S)


@pytest.mark.parametrize("dummy_row", [True, False])
@pytest.mark.parametrize("C", [11, 15, 73])
def test_segment_sizes(C, dummy_row):
    X, seg = _table(SIZES, C, seed=C, dummy_row=dummy_row)
    S, rho, dev = _both(X, seg, np.arange(C), dummy_row, keep_ranks=True)
    assert (dev.status == 0).all()
    assert same(dev.S, S) and same(dev.rho, rho) and same(dev.vector(), ref.upper(rho))
    ranks = dev.ranks.cpu().numpy()
    for s in (0, 1, 4, 8, 11):                                       # the ranks themselves against scipy's
        D = ref.doubled_ranks(ref.with_dummy(X[seg[s]:seg[s + 1]], dummy_row))
        assert np.array_equal(ranks[seg[s] + s:seg[s] + s + len(D)], D)
    # every segment through the four-wave rank kernel, one launch
    forced = cmp._gcm_device(torch.from_numpy(X).cuda(), seg, np.arange(C, dtype=np.int32), dummy_row, max_rows=1024)
    assert same(forced.S, S) and same(forced.rho, rho)


def test_row_bound():
    """n' = DESCO_GCM_DEV_MAX_ROWS is computed, one more is refused by the kernel and merged by the twin."""
    cols = np.array([10, 0, 3, 4, 7, 1, 2, 9, 5, 6, 8], dtype=np.int32)          # a permuted column list, C = 11
    X, seg = _table([MAX, 40, MAX + 1, 257], 11, seed=1)
    S, rho, dev = _both(X, seg, cols)
    status = dev.status.cpu().numpy()
    assert status.tolist() == [0, 0, -1, 0]
    keep = [0, 1, 3]
    assert same(dev.S[keep], S[keep]) and same(dev.rho[keep], rho[keep])
    assert (dev.S[2] == 0).all() and (dev.vector()[2] == 0).all()                 # refused: nothing written
    merged = cmp._merge_refused(dev, torch.from_numpy(X).cuda(), seg, True, 0)
    assert merged.last_backend == "device+host" and (merged.status == 0).all()
    assert same(merged.S, S) and same(merged.rho, rho) and same(merged.vector(), ref.upper(rho))


def test_auto_merges_refused_segments(graphs, monkeypatch):
    host = cmp.graphlet_correlation(graphs, "gcd11", backend="host")
    monkeypatch.setitem(cmp.AUTO_DEVICE, "gcm", True)
    monkeypatch.setattr(cmp, "WAVE_ROWS", 16)
    monkeypatch.setattr(cmp, "DEVICE_MAX_ROWS", 30)                  # the launch's bound: larger graphs are refused
    auto = cmp.graphlet_correlation(graphs, "gcd11", backend="auto")
    assert cmp.last_backend == "device+host"
    assert same(auto.S, host.S) and same(auto.rho, host.rho) and same(auto.vector(), host.vector())
    with pytest.raises(RuntimeError, match="DESCO_GCM_DEV_MAX_ROWS"):
        cmp.graphlet_correlation(graphs, "gcd11", backend="device")
    monkeypatch.undo()
    whole = [graphs.subset(0, 9), graphs.subset(9, 20)]
    assert same(cmp.dataset_gcd(whole, backend="auto"), cmp.dataset_gcd(whole, backend="host"))


@pytest.mark.parametrize("kind", ["constant", "ties"])
def test_all_tied_columns(kind):
    X, seg = _table([1, 2, 40, 64, 300], 15, seed=2, kind=kind)
    for dummy_row in (True, False):
        S, rho, dev = _both(X, seg, np.arange(15), dummy_row)
        assert same(dev.S, S) and same(dev.rho, rho)
    if kind == "constant":
        assert (S == 0).all() and same(rho, np.broadcast_to(np.eye(15), rho.shape))


def test_segment_slices_reproduce_the_full_call():
    X, seg = _table([5, 64, 300, 17, 2, 257, 90, 33], 15, seed=3)
    table = torch.from_numpy(X).cuda()
    full = cmp.graphlet_correlation_device(table=table, orbits="all4", segments=seg)
    ids = np.array([6, 2, 3], dtype=np.int64)
    part = cmp.graphlet_correlation_device(table=table, orbits="all4", segments=seg, segment_ids=ids)
    assert part.status.cpu().tolist() == [1, 1, 0, 0, 1, 1, 0, 1]                  # NOT_LAUNCHED outside the slice
    assert same(part.S[ids], full.S[ids]) and same(part.vector()[ids], full.vector()[ids])
    rest = np.setdiff1d(np.arange(8), ids)
    assert (part.S[rest] == 0).all() and (part.rho[rest] == 0).all()               # untouched
    again = cmp.graphlet_correlation_device(table=table, orbits="all4", segments=seg)
    assert same(again.S, full.S) and same(again.rho, full.rho)                     # the same from call to call
    # a slice of the row pointer on the same table: the segments 2 .. 5
    sub = cmp.graphlet_correlation_device(table=table, orbits="all4", segments=seg[2:7])
    assert same(sub.S, full.S[2:6]) and same(sub.rho, full.rho[2:6])


@pytest.fixture(scope="module")
def vectors():
    rng = np.random.default_rng(8)
    v = rng.uniform(-1, 1, (66, 2628))
    v[5] = v[4]                                                       # a distance of exactly 0
    v[:, 7] = 1.0                                                     # a coordinate that cancels
    return v


@pytest.mark.parametrize("P", [55, 105, 2628])
def test_distance_shapes(vectors, P):
    for Gx in (1, 15, 16, 17, 31, 32, 33):
        for Gy in (1, 15, 16, 17, 31, 32, 33):
            x, y = np.ascontiguousarray(vectors[:Gx, :P]), np.ascontiguousarray(vectors[33:33 + Gy, :P])
            got = cmp.gcd_device(x, y)
            assert got.shape == (Gx, Gy) and same(got, cmp._gcd_host(x, y))
    x = np.ascontiguousarray(vectors[:33, :P])
    self_d = cmp.gcd_device(x).cpu().numpy()
    assert same(self_d, self_d.T.copy()) and self_d[4, 5] == 0.0 and (np.diag(self_d) == 0).all()
    if P == 55:                                                       # and the chain of the definition itself
        assert same(self_d[:6, :9], ref.gcd_matrix(x[:6], x[:9]))
    # the squared distance: bit for bit whatever the root does
    acc = 0.0
    for t in x[0] - x[1]:
        acc = ref.fma(float(t), float(t), acc)
    assert self_d[0, 1] == np.sqrt(acc)


def test_strided_output(vectors):
    x, y = np.ascontiguousarray(vectors[:33, :105]), np.ascontiguousarray(vectors[33:50, :105])
    parent = torch.full((40, 64), float("nan"), dtype=torch.float64, device="cuda")
    cmp.gcd_device(x, y, out=parent[3:36, 5:22])
    got = parent.cpu().numpy()
    assert same(got[3:36, 5:22], cmp._gcd_host(x, y))
    outside = np.ones(got.shape, dtype=bool)
    outside[3:36, 5:22] = False
    assert np.isnan(got[outside]).all()
    with pytest.raises(RuntimeError, match="unit column stride"):
        cmp.gcd_device(x, y, out=parent[3:36, 5:39:2])
