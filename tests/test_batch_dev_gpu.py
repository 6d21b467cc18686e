"""Device batch set-up (csrc/batch_dev.hip) against the host routines it replaces: integer work, every comparison exact.
The reference is always the host path (NeighborhoodPartition.slice / degree_sorted, the numpy pool index, the numpy
expressions of InferencePipeline), never the code under test."""
import functools

import numpy as np
import pytest
import torch

from helpers import golden_graphs, make_models, standard_queries

pytestmark = pytest.mark.gpu

from desco_amd import ops, synthetic
from desco_amd.batch import NeighborhoodBatch
from desco_amd.graphs import GraphSet
from desco_amd.partition import NeighborhoodPartition, build_partition, build_partition_device
from desco_amd.pipeline import InferencePipeline

FIELDS = ("neigh_index", "indicator", "count_ptr", "count_orig", "vrowptr", "vcol")
INPUTS = ("golden", "syn40", "msrc_imdb", "random1500")


def _random1500():
    """one connected graph of 1500 nodes: the path 0-1-...-1499 plus 4500 random pairs"""
    pairs = np.random.default_rng(5).integers(1500, size=(4500, 2))
    edges = {(i, i + 1) for i in range(1499)}
    edges |= {(int(min(a, b)), int(max(a, b))) for a, b in pairs if a != b}
    return GraphSet.from_edge_lists([(1500, sorted(edges))])


@functools.lru_cache(maxsize=None)
def _input(name):
    """(graphs, host partition, device partition)"""
    gs = {"golden": lambda: GraphSet.from_edge_lists(golden_graphs()),
          "syn40": lambda: synthetic.syn_1827_shaped(40),
          "msrc_imdb": lambda: synthetic.msrc_imdb_mixed(6, 10),
          "random1500": _random1500}[name]()
    return gs, build_partition(gs, 4), build_partition_device(gs, 4)


def _same(a, b, fields=FIELDS):
    for f in fields:
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and x.shape == y.shape, (f, x.dtype, y.dtype, x.shape, y.shape)
        assert np.array_equal(x, y), f


def _coverage(part, neigh_key=True):
    """what the degree sort can get wrong, as facts about a HOST partition: neighborhoods per primary slot, per
    direction, with two rows of equal key, and the largest neighborhood"""
    cp = part.count_ptr.astype(np.int64)
    deg = np.diff(part.vrowptr.astype(np.int64))[:4 * part.num_count].reshape(-1, 4)
    seg = np.repeat(np.arange(part.num_neigh), np.diff(cp))
    tot0 = np.bincount(seg, weights=deg[:, 0], minlength=part.num_neigh)
    tot1 = np.bincount(seg, weights=deg[:, 1], minlength=part.num_neigh)
    ps = tot1 >= tot0
    key = part.neigh_index[:, 1] if neigh_key else np.arange(part.num_neigh)
    psr = ps[seg]
    k = (np.where(psr, deg[:, 1], deg[:, 0]) << 32) + np.where(psr, deg[:, 0], deg[:, 1])
    ties = 0
    for b in range(part.num_neigh):
        kb = k[cp[b]:cp[b + 1]]
        ties += len(np.unique(kb)) < len(kb)
    return {"ps1": int(ps.sum()), "ps0": int((~ps).sum()), "odd": int((key & 1).sum()),
            "even": int(((key & 1) == 0).sum()), "ties": ties, "max_rows": int(np.diff(cp).max())}


def _assert_covers(part, both_slots=True):
    c = _coverage(part)
    assert c["ps1"] > 0 and (c["ps0"] > 0 or not both_slots), c       # both primary slots
    assert c["odd"] > 0 and c["even"] > 0, c            # both directions
    assert c["ties"] > 0, c                             # stability matters
    return c


# ---------------------------------------------------------------------------------------------- degree sort
@pytest.mark.parametrize("name", INPUTS)
def test_degree_sorted_device_equals_host(name):
    _, host, dev = _input(name)
    _same(dev, host)
    # (the random graph is dense: every neighborhood's heavier slot is slot 1; the other three inputs have both)
    c = _assert_covers(host, both_slots=name != "random1500")
    if name == "random1500":
        cp = host.count_ptr.astype(np.int64)
        assert c["max_rows"] > 1024 and int((np.diff(cp) > 1024).sum()) >= 100, c      # the LDS pair sort
    if name == "syn40":
        assert c["max_rows"] > 256, c
    ref = host.degree_sorted()
    got = dev.degree_sorted_device()
    assert got.downloads == {f: 0 for f in FIELDS}
    _same(got, ref)
    for f in ("count_ptr", "neigh_index", "indicator"):            # untouched: the very same device tensors
        assert got.device_arrays[f].data_ptr() == dev.device_arrays[f].data_ptr(), f
    assert (got.num_neigh, got.num_count, got.num_edges) == (ref.num_neigh, ref.num_count, ref.num_edges)
    # idempotent, as the host routine is on its own output
    again = got.degree_sorted_device()
    _same(again, ref.degree_sorted())
    _same(again, ref, ("count_orig", "vrowptr", "vcol"))
    # the batch reads the sorted arrays without an upload
    b = NeighborhoodBatch(got, "cuda")
    assert b.vcol.data_ptr() == got.device_arrays["vcol"].data_ptr()
    assert b.vrowptr.data_ptr() == got.device_arrays["vrowptr"].data_ptr()


@pytest.mark.parametrize("name", INPUTS)
def test_degree_sort_without_neigh_key_and_any_launch_geometry(name):
    """neigh_key = NULL (direction by the index b), and the result does not depend on the number of workgroups"""
    from desco_amd import _lib
    _, host, dev = _input(name)
    B, Nc, E = host.num_neigh, host.num_count, host.num_edges
    cp, vr, vc, co = (np.ascontiguousarray(getattr(host, f), dtype=np.int32)
                      for f in ("count_ptr", "vrowptr", "vcol", "count_orig"))
    co2, vr2, vc2 = np.empty_like(co), np.empty_like(vr), np.empty_like(vc)
    _lib.check(_lib.lib().desco_partition_degree_sort(cp.ctypes.data, B, vr.ctypes.data, vc.ctypes.data, co.ctypes.data,
                                                      co2.ctypes.data, vr2.ctypes.data, vc2.ctypes.data, None, 0))
    c = _coverage(host, neigh_key=False)
    assert c["odd"] > 0 and c["even"] > 0
    da = dev.device_arrays
    for key, ref in ((None, (co2, vr2, vc2)),
                     (da["neigh_index"], tuple(getattr(host.degree_sorted(), f) for f in ("count_orig", "vrowptr", "vcol")))):
        for blocks in (0, 5, 1000):
            got = ops.partition_degree_sort_dev(da["count_ptr"], da["vrowptr"], da["vcol"], da["count_orig"], B, Nc, E,
                                                key, blocks)
            for g, r, f in zip(got, ref, ("count_orig", "vrowptr", "vcol")):
                assert np.array_equal(g.cpu().numpy(), r), (f, blocks, key is None)


def test_degree_sort_of_a_neighborhood_too_large_for_lds():
    """A hub joined to 5200 nodes: its depth-1 neighborhood has 5200 count rows, more than the workgroup keeps in LDS
    (and more than the device builder emits): the workspace path, same result.  Built on the host and uploaded."""
    n = 5201
    rng = np.random.default_rng(11)
    edges = {(i, n - 1) for i in range(n - 1)}
    edges |= {(int(min(a, b)), int(max(a, b))) for a, b in rng.integers(n - 1, size=(9000, 2)) if a != b}
    gs = GraphSet.from_edge_lists([(n, sorted(edges)), (4, [(0, 1), (1, 2), (2, 3), (0, 3)])])
    host = build_partition(gs, 1)
    assert int(np.diff(host.count_ptr).max()) == n - 1 > 4608
    _assert_covers(host)
    da = {"device": torch.device("cuda", torch.cuda.current_device())}
    for f in FIELDS:
        a = getattr(host, f)
        da[f] = torch.from_numpy(np.ascontiguousarray(a.astype(np.uint8) if f == "indicator" else a)).cuda()
    dev = NeighborhoodPartition.from_device_arrays(da, host.num_neigh, host.num_count, host.num_edges, 1)
    _same(dev.degree_sorted_device(), host.degree_sorted())
    B = host.num_neigh
    _same(dev.slice_device(B // 2, B).degree_sorted_device(), host.slice(B // 2, B).degree_sorted())


# ---------------------------------------------------------------------------------------------- slice
@pytest.mark.parametrize("name", INPUTS)
def test_slice_device_equals_host(name):
    _, host, dev = _input(name)
    B = host.num_neigh
    assert dev.slice_device(0, B) is dev                              # the whole range costs nothing
    assert dev.slice_device(-5, B + 9) is dev
    before = dict(dev.downloads)                 # (the cached input may have been read by another test)
    cuts = [(0, 0), (3, 3), (B, B), (0, 1), (B - 1, B), (B // 2, B // 2 + 1), (0, B // 3), (B // 3, B), (1, B - 1),
            (B // 4, 3 * B // 4), (-2, 5), (B - 4, B + 10)]
    for b0, b1 in cuts:
        ref, got = host.slice(b0, b1), dev.slice_device(b0, b1)
        assert got.downloads == {f: 0 for f in FIELDS}
        assert (got.num_neigh, got.num_count, got.num_rows, got.num_edges) == \
            (ref.num_neigh, ref.num_count, ref.num_rows, ref.num_edges), (b0, b1)
        _same(got, ref)
    assert dev.downloads == before               # slicing on the device reads no host view of its source
    for b0, b1 in ((0, 1), (B - 1, B), (B // 3, B), (1, B - 1), (B // 4, 3 * B // 4)):
        _same(dev.slice_device(b0, b1).degree_sorted_device(), host.slice(b0, b1).degree_sorted())
        # a slice of a slice
        mid = (b1 - b0) // 2
        _same(dev.slice_device(b0, b1).slice_device(mid, b1 - b0), host.slice(b0, b1).slice(mid, b1 - b0))


# ---------------------------------------------------------------------------------------------- pool index
def _stub_batch(cp, on_device):
    class _P:
        count_ptr = cp
    nb = NeighborhoodBatch.__new__(NeighborhoodBatch)
    nb.part, nb.device = _P, torch.device("cuda", torch.cuda.current_device())
    if on_device:
        nb.count_ptr = torch.from_numpy(cp).cuda()
        nb.num_count = int(cp[-1])
        nb.device_prologue = True
    return nb


def _assert_pool_equal(cp):
    ref, got = _stub_batch(cp, False), _stub_batch(cp, True)
    assert not ref._pool_on_device() and got._pool_on_device()
    (rb, rs, rn), (gb, gs, gn) = ref.pool_index(), got.pool_index()
    assert gn == rn and isinstance(gn, int)
    assert gb.dtype == rb.dtype == torch.int32 and gs.dtype == rs.dtype == torch.int32
    assert torch.equal(gb.cpu(), rb.cpu()) and torch.equal(gs.cpu(), rs.cpu())
    assert got.max_count_rows() == ref.max_count_rows()
    assert _stub_batch(cp, True).max_count_rows() == ref.max_count_rows()       # asked first, too


def test_pool_index_device_equals_numpy_on_segment_lists():
    rng = np.random.default_rng(3)
    for lens in ([1], [32], [33], [5, 1, 1, 90, 2, 31, 64, 1], list(rng.integers(1, 70, size=200)),
                 [1] * 100, [700, 3, 640], [16] * 40, [15, 1, 16, 17], list(rng.integers(1, 40, size=50_000))):
        _assert_pool_equal(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32))
    for lens in ([4, 0, 7], [0], [3, 5, 0], [16, 0, 16]):                       # a neighborhood without count rows
        cp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        msgs = []
        for on_device in (False, True):
            with pytest.raises(ValueError, match="at least one count row per neighborhood") as e:
                _stub_batch(cp, on_device).pool_index()
            msgs.append(str(e.value))
        assert msgs[0] == msgs[1]


@pytest.mark.parametrize("name", INPUTS)
def test_pool_index_device_equals_numpy_on_partitions(name):
    _, host, dev = _input(name)
    _assert_pool_equal(np.ascontiguousarray(host.count_ptr, dtype=np.int32))
    b = NeighborhoodBatch(dev.degree_sorted_device(), "cuda")
    ref = _stub_batch(np.ascontiguousarray(host.count_ptr, dtype=np.int32), False)
    assert b._pool_on_device()
    for g, r in zip(b.pool_index(), ref.pool_index()):
        assert (g == r) if isinstance(r, int) else torch.equal(g.cpu(), r.cpu())
    assert b.max_count_rows() == ref.max_count_rows()
    assert b.part.downloads == {f: 0 for f in FIELDS}


# ---------------------------------------------------------------------------------------------- neighborhood rows
def _assert_neigh_rows(gs):
    host, dev = build_partition(gs, 4), build_partition_device(gs, 4)
    G = gs.num_graphs
    per_graph = np.bincount(host.neigh_index[:, 0], minlength=G)
    ngp = np.concatenate([[0], np.cumsum(per_graph)]).astype(np.int64)
    rows = gs.graph_ptr[host.neigh_index[:, 0]] + host.neigh_index[:, 1]
    da = dev.device_arrays
    scatter, ngp_dev = ops.neigh_rows_dev(da["neigh_index"], da["graph_ptr"], G)
    assert scatter.dtype == ngp_dev.dtype == torch.int32
    assert np.array_equal(scatter.cpu().numpy(), rows.astype(np.int32))
    assert np.array_equal(ngp_dev.cpu().numpy(), ngp.astype(np.int32))
    return per_graph


@pytest.mark.parametrize("name", INPUTS)
def test_neigh_rows_device_equals_numpy(name):
    _assert_neigh_rows(_input(name)[0])


def test_neigh_rows_with_graphs_that_have_no_neighborhood():
    graphs = [(3, []), (2, [(0, 1)]), (1, []), (3, [(0, 1), (1, 2), (0, 2)]), (2, []), (2, []),
              (5, [(0, 1), (1, 2), (3, 4)]), (4, [])]
    per_graph = _assert_neigh_rows(GraphSet.from_edge_lists(graphs))
    assert (per_graph == 0).sum() >= 5 and per_graph[0] == 0 and per_graph[-1] == 0 and per_graph.sum() > 0
    per_graph = _assert_neigh_rows(GraphSet.from_edge_lists([(2, []), (3, [])]))          # no neighborhood at all
    assert per_graph.sum() == 0


# ---------------------------------------------------------------------------------------------- pipeline
@functools.lru_cache(maxsize=None)
def _models():
    nm, gm = make_models(seed=0)
    nm, gm = nm.to("cuda"), gm.to("cuda")
    nm.set_queries(standard_queries()[0])
    return nm, gm


def _pipeline_graphs(name):
    return GraphSet.from_edge_lists(golden_graphs()) if name == "golden" else synthetic.cox2_shaped(60)


OUT_KEYS = ("neigh_count", "graph_neigh_count", "x", "node_count", "graph_gossip_count")


@pytest.mark.parametrize("kw", [{}, {"max_neigh_rows": 4000}, {"chunks": 4}, {"degree_sort": False},
                                {"max_neigh_rows": 4000, "degree_sort": False}, {"max_neigh_rows": 4000, "chunks": 4}],
                         ids=["one_block", "small_blocks", "chunks4", "unsorted", "small_blocks_unsorted",
                              "small_blocks_chunks4"])
@pytest.mark.parametrize("name", ["golden", "cox2_60"])
def test_pipeline_device_prologue_equals_host_prologue(name, kw):
    nm, gm = _models()
    gs = _pipeline_graphs(name)
    dev = InferencePipeline(nm, gm, gs, depth=4, device="cuda", rank=0, world=1, device_prologue=True, **kw)
    host = InferencePipeline(nm, gm, gs, depth=4, device="cuda", rank=0, world=1, device_prologue=False, **kw)
    assert dev.device_prologue and not host.device_prologue
    assert dev.partition_backend == host.partition_backend == "device"
    if name == "golden":
        assert dev.partition.num_rows == 12402
        if "max_neigh_rows" in kw:
            assert len(dev.neigh_batches) >= 4
    if "chunks" in kw:
        assert len(dev.neigh_batches) >= 4
    assert len(dev.neigh_batches) == len(host.neigh_batches)
    for a, b in zip(dev.neigh_batches, host.neigh_batches):
        assert (a.num_graphs, a.num_count, a.num_rows) == (b.num_graphs, b.num_count, b.num_rows)
        for f in ("count_ptr", "vrowptr", "vcol"):
            assert getattr(a, f).dtype == getattr(b, f).dtype == torch.int32
            assert torch.equal(getattr(a, f), getattr(b, f)), f
        assert a._pool_on_device() and not b._pool_on_device()
        (ab, as_, an), (bb, bs, bn) = a.pool_index(), b.pool_index()
        assert an == bn and torch.equal(ab, bb) and torch.equal(as_, bs)
        assert a.max_count_rows() == b.max_count_rows()
    for f in ("scatter_index", "neigh_graph_ptr"):
        assert getattr(dev, f).dtype == getattr(host, f).dtype and torch.equal(getattr(dev, f), getattr(host, f)), f
    od = {k: v.clone() for k, v in dev.run().items()}
    oh = host.run()
    torch.cuda.synchronize()
    assert set(od) == set(oh) == set(OUT_KEYS)
    for k in OUT_KEYS:
        assert od[k].shape == oh[k].shape and torch.equal(od[k], oh[k]), k          # bit-identical
    # the large arrays never reached the host on the device path
    for p in [dev.partition] + [b.part for b in dev.neigh_batches]:
        assert p.downloads["count_orig"] == 0 and p.downloads["vrowptr"] == 0 and p.downloads["vcol"] == 0
    if not kw:
        assert dev.partition.downloads == {f: 0 for f in FIELDS}                  # one block: nothing at all


def test_pipeline_partition_host_views_answer_lazily():
    nm, gm = _models()
    gs = GraphSet.from_edge_lists(golden_graphs())
    pipe = InferencePipeline(nm, gm, gs, depth=4, device="cuda", rank=0, world=1, device_prologue=True)
    pipe.run()
    torch.cuda.synchronize()
    part, host = pipe.partition, build_partition(gs, 4)
    assert part.downloads == {f: 0 for f in FIELDS}
    assert np.array_equal(part.neigh_index, host.neigh_index) and part.downloads["neigh_index"] == 1
    assert part.indicator.dtype == np.bool_ and np.array_equal(part.indicator, host.indicator)
    assert part.downloads["vcol"] == 0 and part.downloads["vrowptr"] == 0 and part.downloads["count_orig"] == 0
    _same(part, host)


def test_switch_and_given_partition_keep_the_host_path(monkeypatch):
    nm, gm = _models()
    gs = GraphSet.from_edge_lists(golden_graphs(max_n=30))
    monkeypatch.setenv("DESCO_DEVICE_PROLOGUE", "0")
    assert not InferencePipeline(nm, gm, gs, depth=4, device="cuda", rank=0, world=1).device_prologue
    monkeypatch.setenv("DESCO_DEVICE_PROLOGUE", "1")
    assert InferencePipeline(nm, gm, gs, depth=4, device="cuda", rank=0, world=1).device_prologue
    monkeypatch.delenv("DESCO_DEVICE_PROLOGUE")
    assert InferencePipeline(nm, gm, gs, depth=4, device="cuda", rank=0, world=1).device_prologue
    given = InferencePipeline(nm, gm, gs, depth=4, device="cuda", rank=0, world=1, partition=build_partition(gs, 4))
    assert not given.device_prologue and given.partition_backend == "given"
    quirk = InferencePipeline(nm, gm, gs, depth=4, device="cuda", rank=0, world=1, quirk_batch=512)
    assert not quirk.device_prologue and quirk.partition_backend == "host"
