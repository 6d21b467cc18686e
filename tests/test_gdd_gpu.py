"""Graphlet degree distributions and their agreement on the MI355X (csrc/graphlet_distribution_dev.hip) against the
host twin (csrc/graphlet_distribution.cpp), bit for bit: the lists (len, key, val, the unused slots zero) and the
agreements (the matrix and the per-orbit values); a subset of pairs also against the plain-Python definition in
gdd_reference.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gdd_reference as ref  # noqa: E402
from helpers import golden_graphs  # noqa: E402

from desco_amd import _lib  # noqa: E402
from desco_amd import comparison as cmp  # noqa: E402
from desco_amd import synthetic  # noqa: E402
from desco_amd.graphs import GraphSet  # noqa: E402

pytestmark = pytest.mark.gpu

MAX = cmp.DEVICE_MAX_ROWS


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int64) if a.dtype == np.float64 else a


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def same_lists(dev, host):
    return same(dev.len, host.len) and same(dev.key, host.key) and same(dev.val, host.val)


def _table(sizes, C, seed, kind="mixed"):
    rng = np.random.default_rng(seed)
    seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    X = np.concatenate([ref.random_table(rng, n, C, kind) for n in sizes]) if sum(sizes) else np.zeros((0, C), np.int64)
    return X, seg


def _host(X, seg, columns=None, threads=0):
    columns = np.arange(X.shape[1], dtype=np.int32) if columns is None else np.asarray(columns, dtype=np.int32)
    return cmp.GraphletDistribution(*cmp._gdd_host(X, seg, columns, threads), seg, columns, None, "host")


def _raw_build(X, seg, columns, bound, ids=None):
    """desco_gdd_build_dev into buffers filled with sentinels: what the launch did not write keeps them."""
    N, C, nseg = X.shape[0], len(columns), len(seg) - 1
    table, seg_d = torch.from_numpy(X).cuda(), torch.from_numpy(seg).cuda()
    ln = torch.full((nseg, C), -5, dtype=torch.int32, device="cuda")
    key = torch.full((N * C,), -5, dtype=torch.int64, device="cuda")
    val = torch.full((N * C,), float("nan"), dtype=torch.float64, device="cuda")
    status = torch.full((nseg,), cmp.NOT_LAUNCHED, dtype=torch.int32, device="cuda")
    ids_d = None if ids is None else torch.from_numpy(np.asarray(ids, dtype=np.int64)).cuda()
    columns = np.asarray(columns, dtype=np.int32)
    _lib.check(_lib.lib().desco_gdd_build_dev(seg_d.data_ptr(), nseg, N, table.data_ptr(), X.shape[1],
                                              columns.ctypes.data, C, None if ids is None else ids_d.data_ptr(),
                                              0 if ids is None else len(ids), bound, ln.data_ptr(), key.data_ptr(),
                                              val.data_ptr(), status.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream), "desco_gdd_build_dev")
    torch.cuda.synchronize()
    return ln.cpu().numpy(), key.cpu().numpy(), val.cpu().numpy(), status.cpu().numpy()


@pytest.fixture(scope="module")
def graphs():
    lists = list(golden_graphs(max_n=40))[:12]
    lists += synthetic.cox2_shaped(20).edge_lists() + synthetic.syn_1827_shaped(40).edge_lists()
    lists += [(1, []), (2, [(0, 1)]), (6, [])]
    return GraphSet.from_edge_lists(lists)


@pytest.mark.parametrize("orbits", ["all4", "all5"])
def test_graphs_device_equals_twin(graphs, orbits):
    host = cmp.graphlet_distribution(graphs, orbits, backend="host")
    dev = cmp.graphlet_distribution(graphs, orbits, backend="device")
    assert cmp.last_backend == "device" and (dev.status == 0).all()
    assert same_lists(dev, host) and (host.len != 0).any()
    on_gpu = cmp.graphlet_distribution_device(graphs, orbits)
    assert on_gpu.key.is_cuda and same_lists(on_gpu, host)
    non = cmp.graphlet_distribution(graphs, orbits, induced=False, backend="host")
    assert same_lists(cmp.graphlet_distribution(graphs, orbits, induced=False, backend="device"), non)
    a_host, p_host = cmp.gdd_agreement(host, per_orbit=True, backend="host")
    a_dev, p_dev = cmp.gdd_agreement_device(on_gpu, per_orbit=True)
    assert same(a_dev, a_host) and same(p_dev, p_host) and (np.diag(a_host) == 1.0).all()
    assert same(cmp.gdd_agreement(host, backend="device"), a_host) and cmp.last_backend == "device"
    idx, val = cmp.gdd_nearest(host, host, k=3, backend="host")
    idx_d, val_d = cmp.gdd_nearest(on_gpu, on_gpu, k=3, backend="device", chunk_rows=7)
    assert np.array_equal(idx, idx_d) and same(val, val_d)
    g_host = cmp.gdd_agreement(host, mean="geometric", backend="host")
    g_dev = cmp.gdd_agreement(host, mean="geometric", backend="device", chunk_rows=5)
    assert np.allclose(g_dev, g_host, rtol=1e-12, atol=0.0)


# one wave up to DESCO_GCM_WAVE_ROWS rows, four above; the bound itself
SIZES = [1, 2, 63, 64, 65, 255, 256, 0, 257, 1025, MAX]


def test_segment_sizes_and_unused_slots():
    X, seg = _table(SIZES, 6, seed=1)
    host = _host(X, seg)
    dev = cmp._gdd_device(torch.from_numpy(X).cuda(), seg, host.columns)
    assert (dev.status == 0).all() and same_lists(dev, host)
    # every segment through the four-wave kernel in one launch, into buffers of sentinels: the unused slots are written
    ln, key, val, status = _raw_build(X, seg, host.columns, MAX)
    assert (status == 0).all() and same(ln, host.len) and same(key, host.key) and same(val, host.val)
    # and the small ones through the one-wave kernel alone
    small = np.flatnonzero(np.diff(seg) <= cmp.WAVE_ROWS)
    ln, key, val, status = _raw_build(X, seg, host.columns, cmp.WAVE_ROWS, ids=small)
    for s in range(len(SIZES)):
        a, b = seg[s] * 6, seg[s + 1] * 6
        if s in small:
            assert status[s] == 0 and same(ln[s], host.len[s]) and same(key[a:b], host.key[a:b])
            assert same(val[a:b], host.val[a:b])
        else:
            assert status[s] == cmp.NOT_LAUNCHED and (ln[s] == -5).all() and (key[a:b] == -5).all()
            assert np.isnan(val[a:b]).all()


@pytest.mark.parametrize("kind", ["zeros", "constant", "ties", "distinct", "huge"])
def test_column_kinds(kind):
    X, seg = _table([1, 2, 40, 64, 300], 3, seed=2, kind=kind)
    host = _host(X, seg)
    dev = cmp._gdd_device(torch.from_numpy(X).cuda(), seg, host.columns)
    assert same_lists(dev, host)
    if kind == "zeros":
        assert (host.len == 0).all()
    if kind == "constant":
        assert (host.len == 1).all()
    if kind == "distinct":
        assert np.array_equal(host.len[:, 0], np.diff(seg))


def test_row_bound_is_refused_and_nothing_written():
    cols = np.array([2, 0, 1], dtype=np.int32)                                    # a permuted column list
    X, seg = _table([MAX + 1, 40], 3, seed=3, kind="ties")
    host = _host(X, seg, cols)
    ln, key, val, status = _raw_build(X, seg, cols, MAX)
    assert status.tolist() == [-1, 0]
    a = seg[1] * 3
    assert (ln[0] == -5).all() and (key[:a] == -5).all() and np.isnan(val[:a]).all()
    assert same(ln[1], host.len[1]) and same(key[a:], host.key[a:]) and same(val[a:], host.val[a:])
    dev = cmp._gdd_device(torch.from_numpy(X).cuda(), seg, cols)
    assert dev.status.cpu().tolist() == [-1, 0]
    merged = cmp._gdd_merge_refused(dev, torch.from_numpy(X).cuda(), 0)
    assert merged.last_backend == "device+host" and (merged.status == 0).all() and same_lists(merged, host)
    with pytest.raises(RuntimeError, match=r"DESCO_GCM_DEV_MAX_ROWS \(20480\)"):
        _raw_build(X, seg, cols, MAX + 1)


def test_auto_merges_refused_segments(graphs, monkeypatch):
    host = cmp.graphlet_distribution(graphs, "all4", backend="host")
    monkeypatch.setitem(cmp.AUTO_DEVICE, "gdd", True)
    monkeypatch.setitem(cmp.AUTO_DEVICE, "gdda", True)
    monkeypatch.setattr(cmp, "WAVE_ROWS", 16)
    monkeypatch.setattr(cmp, "DEVICE_MAX_ROWS", 30)                  # the launch's bound: larger graphs are refused
    auto = cmp.graphlet_distribution(graphs, "all4", backend="auto")
    assert cmp.last_backend == "device+host" and same_lists(auto, host)
    with pytest.raises(RuntimeError, match="DESCO_GCM_DEV_MAX_ROWS"):
        cmp.graphlet_distribution(graphs, "all4", backend="device")
    monkeypatch.setattr(cmp, "WAVE_ROWS", 256)
    monkeypatch.setattr(cmp, "DEVICE_MAX_ROWS", MAX)
    whole = [graphs.subset(0, 9), graphs.subset(9, 20)]
    assert same(cmp.dataset_gdda(whole, backend="auto"), cmp.dataset_gdda(whole, backend="host"))


def test_segment_slices_reproduce_the_full_call():
    X, seg = _table([5, 64, 300, 17, 2, 257, 90, 33], 15, seed=4)
    table = torch.from_numpy(X).cuda()
    full = cmp.graphlet_distribution_device(table=table, orbits="all4", segments=seg)
    assert same_lists(full, _host(X, seg))
    ids = np.array([6, 2, 3], dtype=np.int64)
    part = cmp.graphlet_distribution_device(table=table, orbits="all4", segments=seg, segment_ids=ids)
    assert part.status.cpu().tolist() == [1, 1, 0, 0, 1, 1, 0, 1]                  # NOT_LAUNCHED outside the slice
    for s in range(8):
        a, b = seg[s] * 15, seg[s + 1] * 15
        if s in ids:
            assert same(part.len[s], full.len[s]) and same(part.key[a:b], full.key[a:b])
            assert same(part.val[a:b], full.val[a:b])
        else:
            assert (part.len[s] == 0).all() and (part.key[a:b] == 0).all() and (part.val[a:b] == 0).all()
    # a slice of the row pointer on the same table: the segments 2 .. 5, at their places in the table
    sub = cmp.graphlet_distribution_device(table=table, orbits="all4", segments=seg[2:7])
    a, b = seg[2] * 15, seg[6] * 15
    assert same(sub.len, full.len[2:6]) and same(sub.key[a:b], full.key[a:b]) and same(sub.val[a:b], full.val[a:b])
    for s in range(4):
        for (k, v), (k2, v2) in zip(sub.lists(s), full.lists(s + 2)):
            assert same(k, k2) and same(v, v2)


@pytest.fixture(scope="module")
def many():
    """Host-built lists of 140 short segments per column count: empty, one-entry, tied, distinct and huge columns, two
    pairs of identical segments, segments of no rows."""
    out = {}
    for C in (1, 15, 73):
        rng = np.random.default_rng(C)
        sizes = rng.integers(0, 14, 140)
        sizes[3], sizes[40] = 9, 13
        sizes[71], sizes[139] = sizes[3], sizes[40]
        X, seg = _table(sizes, C, seed=10 + C, kind="ties" if C == 1 else "mixed")
        for s, t in ((3, 71), (40, 139)):                                         # two pairs of identical segments
            X[seg[t]:seg[t + 1]] = X[seg[s]:seg[s + 1]]
        out[C] = _host(X, seg)
    return out


@pytest.mark.parametrize("C", [1, 15, 73])
@pytest.mark.parametrize("shape", [(1, 1), (1, 65), (31, 33), (64, 64), (70, 3)])
def test_agreement_tile_edges(many, C, shape):
    Gx, Gy = shape
    host = many[C]
    dev = host.cuda()
    x, y, xd, yd = host.rows(0, Gx), host.rows(70, 70 + Gy), dev.rows(0, Gx), dev.rows(70, 70 + Gy)
    a_host, p_host = cmp._gdda_host(x, y, True)
    a_dev, p_dev = cmp.gdd_agreement_device(xd, yd, per_orbit=True)
    assert a_dev.shape == (Gx, Gy) and same(a_dev, a_host) and same(p_dev, p_host)
    assert same(cmp.gdd_agreement_device(xd, yd), a_host)                          # the same without the per-orbit output
    assert same(cmp.gdd_agreement_device(yd, xd), a_host.T.copy())
    assert (a_host >= 0).all() and (a_host <= 1).all()


def test_agreement_of_crafted_lists():
    """Empty, one-entry, identical, disjoint and interleaved lists, C = 1: segment by segment."""
    cols = [[0, 0, 0], [5, 5, 5], [1, 2, 3, 3], [3, 1, 3, 2], [10, 20, 30], [1, 10, 3, 30], [2, 4, 6, 8, 10, 12],
            [1, 3, 5, 7, 9, 11], []]
    seg = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
    X = np.concatenate([np.asarray(c, dtype=np.int64) for c in cols]).reshape(-1, 1)
    host = _host(X, seg)
    assert host.len[:, 0].tolist() == [0, 1, 3, 3, 3, 4, 6, 6, 0]
    dev = cmp._gdd_device(torch.from_numpy(X).cuda(), seg, host.columns)
    assert same_lists(dev, host)
    a_host, _ = cmp._gdda_host(host, host, False)
    a_dev = cmp.gdd_agreement_device(dev)
    assert same(a_dev, a_host) and same(a_host, a_host.T.copy()) and (np.diag(a_host) == 1.0).all()
    assert a_host[0, 8] == 1.0 and a_host[2, 3] == 1.0                              # empty x empty, the same multiset
    assert a_host[0, 1] == 1.0 - np.sqrt(0.5)                                       # empty against the one entry (k, 1)
    lists = [host.lists(s) for s in range(9)]
    for i in range(9):
        for j in range(9):
            assert a_host[i, j] == ref.pair(lists[i], lists[j])[0]


def test_long_lists_pass_the_staging_budget():
    """One list of 5000 entries and one of 600 (above what is staged) against lists of 3, on both sides of the pair."""
    sizes = [5000, 3, 3, 600, 3, 513, 512, 0]
    rng = np.random.default_rng(6)
    seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    X = np.zeros((seg[-1], 2), dtype=np.int64)
    for s, n in enumerate(sizes):
        X[seg[s]:seg[s + 1], 0] = rng.permutation(6000)[:n] + 1                    # all distinct: a list of n entries
        X[seg[s]:seg[s + 1], 1] = rng.integers(0, 3, n)
    host = _host(X, seg)
    assert host.len[:, 0].tolist() == sizes
    dev = cmp._gdd_device(torch.from_numpy(X).cuda(), seg, host.columns)
    assert same_lists(dev, host)
    a_host, p_host = cmp._gdda_host(host, host, True)
    for d in (dev, host.cuda()):                                                    # device-built and host-built lists
        a_dev, p_dev = cmp.gdd_agreement_device(d, per_orbit=True)
        assert same(a_dev, a_host) and same(p_dev, p_host)
    assert same(a_host, a_host.T.copy()) and (np.diag(a_host) == 1.0).all()


def test_strided_output(many):
    dev = many[15].cuda()
    x, y = dev.rows(0, 33), dev.rows(50, 67)
    want, _ = cmp._gdda_host(many[15].rows(0, 33), many[15].rows(50, 67), False)
    parent = torch.full((40, 64), float("nan"), dtype=torch.float64, device="cuda")
    cmp.gdd_agreement_device(x, y, out=parent[3:36, 5:22])
    got = parent.cpu().numpy()
    assert same(got[3:36, 5:22], want)
    outside = np.ones(got.shape, dtype=bool)
    outside[3:36, 5:22] = False
    assert np.isnan(got[outside]).all()
    with pytest.raises(RuntimeError, match="unit column stride"):
        cmp.gdd_agreement_device(x, y, out=parent[3:36, 5:39:2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cmp.gdd_agreement_device(many[15])


def test_forty_pairs_against_the_definition(many):
    host = many[15]
    dev = host.cuda()
    a_dev, p_dev = cmp.gdd_agreement_device(dev.rows(0, 8), dev.rows(100, 105), per_orbit=True)
    a_dev, p_dev = a_dev.cpu().numpy(), p_dev.cpu().numpy()
    for i in range(8):
        for j in range(5):
            agree, per = ref.pair(host.lists(i), host.lists(100 + j))
            assert a_dev[i, j] == agree and p_dev[i, j].tolist() == per
