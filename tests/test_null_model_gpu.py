"""Degree-preserving null model on the GPU (csrc/null_model_dev.hip): the kernel against the host twin bit for bit --
on tiny graphs almost every speculative batch is cut short by a conflict, and on the 5-node classes an accepted lane
changes a pair that a later lane tests without sharing a slot with it --, repeatability and slicing, the size limit and
the merge with the host twin, and motif_significance on the device against the host route."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import null_model_reference as R  # noqa: E402
from desco_amd import motifs, synthetic  # noqa: E402
from desco_amd.graphs import GraphSet  # noqa: E402


def host(graphs, replicas, spe, seed, graph_base=0, replica_base=0):
    return motifs._rewire_host(graphs, replicas, spe, seed, graph_base, replica_base, 0)


def device(graphs, replicas, spe, seed, graph_base=0, replica_base=0):
    col, acc = motifs.rewire_device(graphs, replicas, spe, seed, "cuda", graph_base, replica_base)
    assert col.is_cuda and col.dtype == torch.int32 and acc.is_cuda and acc.dtype == torch.int32
    return col.cpu().numpy(), acc.cpu().numpy()


@pytest.fixture(scope="module")
def sets():
    out = R.ladder()
    out["cox2"] = synthetic.cox2_shaped(64)
    syn = synthetic.syn_1827_shaped(1827)
    n, m = motifs._graph_sizes(syn)
    density = m / np.maximum(n * (n - 1) / 2, 1)
    big, dense = int(np.argmax(n)), int(np.argmax(np.where(n >= 20, density, 0)))
    out["syn_largest"] = syn.subset(max(big - 5, 0), min(big + 3, 1827))       # the data set's largest graph
    out["syn_densest"] = syn.subset(max(dense - 5, 0), min(dense + 3, 1827))   # and its densest of 20 nodes or more
    assert motifs._device_fit(out["syn_largest"]).all()
    return out


NAMES = ["edges0123", "fixed", "small", "classes", "gnm40", "hub", "cox2", "syn_largest", "syn_densest"]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("replicas,spe", [(1, 1), (3, 1), (1, 10), (3, 10)])
def test_device_equals_host_twin(sets, name, replicas, spe):
    g = sets[name]
    col, acc = device(g, replicas, spe, seed=99 + spe, graph_base=2, replica_base=5)
    ref_col, ref_acc = host(g, replicas, spe, seed=99 + spe, graph_base=2, replica_base=5)
    assert (acc >= 0).all() and np.array_equal(acc, ref_acc)
    assert np.array_equal(col, ref_col)
    if name == "fixed":
        assert not acc.any() and all(np.array_equal(c, g.col) for c in col)
    if name in ("cox2", "gnm40", "hub", "syn_largest") and spe == 10:
        assert (acc > 0).all()


def test_repeatability_and_slicing(sets):
    g = sets["cox2"]
    col, acc = device(g, 4, 10, seed=8)
    again = device(g, 4, 10, seed=8)
    assert np.array_equal(again[0], col) and np.array_equal(again[1], acc)
    assert not np.array_equal(device(g, 4, 10, seed=9)[0], col)
    g0, g1 = 11, 40
    e0, e1 = int(g.rowptr[g.graph_ptr[g0]]), int(g.rowptr[g.graph_ptr[g1]])
    cs, as_ = device(g.subset(g0, g1), 4, 10, seed=8, graph_base=g0)
    assert np.array_equal(cs + np.int32(g.graph_ptr[g0]), col[:, e0:e1]) and np.array_equal(as_, acc[:, g0:g1])
    cr, ar = device(g, 2, 10, seed=8, replica_base=2)
    assert np.array_equal(cr, col[2:]) and np.array_equal(ar, acc[2:])
    sets_, acc2 = motifs.rewire(g, replicas=4, swaps_per_edge=10, seed=8, backend="device")
    assert motifs.last_backend == "device" and np.array_equal(acc2, acc)
    assert all(np.array_equal(s.col, c) for s, c in zip(sets_, col))


def ring(n):
    return n, [(i, (i + 1) % n) for i in range(n)]


def test_size_limit_and_merge_with_the_host(sets):
    big = 1200                                   # 1200 rows of 39 words: above the 40960 of the LDS workspace
    assert motifs.workspace_words(big, big) > motifs.DEVICE_MAX_WORDS >= motifs.workspace_words(1000, 2000)
    small = sets["small"].edge_lists()
    g = GraphSet.from_edge_lists(small[:2] + [ring(big)] + small[2:] + [R._gnm(40, 100, 5)])
    with pytest.raises(RuntimeError, match="desco_null_model_rewire_dev.*DESCO_NULL_MODEL_DEV_MAX_WORDS"):
        motifs.rewire_device(g, 2, 3, seed=1)
    with pytest.raises(RuntimeError, match="DESCO_NULL_MODEL_DEV_MAX_WORDS"):
        motifs.rewire(g, 2, 3, seed=1, backend="device")
    merged, acc = motifs.rewire(g, replicas=2, swaps_per_edge=3, seed=1, backend="auto")
    assert motifs.last_backend == "device+host"
    ref, ref_acc = motifs.rewire(g, replicas=2, swaps_per_edge=3, seed=1, backend="host")
    assert np.array_equal(acc, ref_acc) and (acc[:, 2] > 0).all()
    assert all(np.array_equal(a.col, b.col) for a, b in zip(merged, ref))
    motifs.rewire(sets["small"], replicas=2, swaps_per_edge=3, seed=1, backend="auto")
    assert motifs.last_backend == "device"
    queries = [(3, ((0, 1), (1, 2))), (4, ((0, 1), (1, 2), (2, 3)))]
    a = motifs.motif_significance(g, queries, replicas=2, swaps_per_edge=3, seed=1, backend="auto", keep_null=True)
    b = motifs.motif_significance(g, queries, replicas=2, swaps_per_edge=3, seed=1, backend="host", keep_null=True)
    assert a.last_backend == "device+host" and np.array_equal(a.null, b.null) and np.array_equal(a.real, b.real)
    assert np.array_equal(a.accepted, b.accepted)


@pytest.fixture(scope="module")
def significance_host():
    g = synthetic.cox2_shaped(12)
    return g, {ind: motifs.motif_significance(g, None, replicas=5, swaps_per_edge=10, seed=3, induced=ind,
                                              backend="host", keep_null=True) for ind in (True, False)}


@pytest.mark.parametrize("induced", [True, False])
@pytest.mark.parametrize("chunk", [1, 4, None])
def test_motif_significance_device_equals_host(significance_host, induced, chunk):
    g, ref = significance_host
    res = motifs.motif_significance(g, None, replicas=5, swaps_per_edge=10, seed=3, induced=induced,
                                    backend="device", replica_chunk=chunk, keep_null=True)
    want = ref[induced]
    assert res.last_backend == motifs.last_backend == "device"
    assert res.real.shape == (12, 29) and res.null.shape == (5, 12, 29) and res.real.any()
    for f in ("real", "null", "accepted", "dataset_real", "dataset_null"):
        assert np.array_equal(getattr(res, f), getattr(want, f)), f
    for f in motifs.MotifSignificance.FIELDS:
        for name in (f, "dataset_" + f):
            assert getattr(res, name).tobytes() == getattr(want, name).tobytes(), name


def test_duplicate_and_two_node_queries_on_the_device(sets):
    g = sets["gnm40"]
    queries = [(2, ((0, 1),)), (3, ((0, 1), (1, 2))), (3, ((1, 0), (0, 2))), (5, ((0, 1), (0, 2), (0, 3), (0, 4)))]
    for induced in (True, False):
        a = motifs.motif_significance(g, queries, replicas=3, seed=6, induced=induced, backend="device", keep_null=True)
        b = motifs.motif_significance(g, queries, replicas=3, seed=6, induced=induced, backend="host", keep_null=True)
        assert np.array_equal(a.real, b.real) and np.array_equal(a.null, b.null)
        assert a.real[0, 0] == 100 and (a.null[:, 0, 0] == 100).all() and np.array_equal(a.real[:, 1], a.real[:, 2])
