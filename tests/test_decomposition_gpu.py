"""k-core / k-truss decomposition on the GPU (csrc/core_truss_dev.hip): the kernel against the host twin bit for bit on
the named families (one round that removes a whole clique, a hub above the workgroup's lanes, several passes per edge
loop), slices of a graph set, routing above the LDS limit, the refusals of the entry point and the kernel's own guard."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import decomposition_reference as R  # noqa: E402
from helpers import random_family_graphs  # noqa: E402
from desco_amd import _lib, decomposition as D, synthetic  # noqa: E402
from desco_amd.graphs import GraphSet  # noqa: E402

FIELDS = ("core", "truss", "support", "node_truss")


@pytest.fixture(scope="module")
def sets():
    return {"families": R.families(), "dense": R.dense_random(),
            "random_families": GraphSet.from_edge_lists(random_family_graphs(43, 90)),
            "syn": synthetic.WORKLOADS["syn_1827"]().subset(300, 420), "cox2": synthetic.WORKLOADS["cox2"]()}


@pytest.mark.parametrize("name", ["families", "dense", "random_families", "syn", "cox2"])
def test_device_equals_host_twin(sets, name):
    g = sets[name]
    want = D.decompose(g, backend="host")
    got = D.decompose_device(g)
    for f in FIELDS + ("rows", "status"):
        x = getattr(got, f)
        assert x.is_cuda and x.dtype == (torch.int64 if f == "rows" else torch.int32), f
    assert (got.status == 0).all()
    got = got.cpu()
    for f in FIELDS + ("rows",):
        assert np.array_equal(getattr(got, f), getattr(want, f)), f
    if name != "cox2":
        assert want.truss.max() >= 4                              # a constant answer must not pass
    else:
        assert (want.truss == 2).all() and want.core.max() >= 2   # molecules: no triangles; the core peel is what counts
    res = D.decompose(g, backend="device")
    assert D.last_backend == res.last_backend == "device"
    assert all(np.array_equal(getattr(res, f), getattr(want, f)) for f in FIELDS)
    auto = D.decompose(g, backend="auto")
    assert D.last_backend == "device" and all(np.array_equal(getattr(auto, f), getattr(want, f)) for f in FIELDS)


def test_halves_and_empty_sets_on_the_device(sets):
    g = sets["dense"]
    want = D.decompose(g, backend="host")
    only_core, only_truss = D.decompose_device(g, truss=False).cpu(), D.decompose_device(g, core=False).cpu()
    assert only_core.truss is None and np.array_equal(only_core.core, want.core)
    assert only_truss.core is None and np.array_equal(only_truss.truss, want.truss)
    assert np.array_equal(only_truss.support, want.support) and (only_truss.status == 0).all()
    empty = D.decompose_device(GraphSet.from_edge_lists([])).cpu()
    assert empty.core.shape == (0,) and empty.truss.shape == (0,) and empty.status.shape == (0,)
    bare = D.decompose_device(GraphSet.from_edge_lists([(5, []), (1, [])])).cpu()
    assert bare.core.tolist() == [0] * 6 and bare.truss.shape == (0,) and bare.status.tolist() == [0, 0]


def test_a_slice_writes_exactly_its_graphs_rows(sets):
    g = sets["random_families"]
    whole = D.decompose_device(g).cpu()
    ids = np.arange(0, g.num_graphs, 3)
    part = D.decompose_device(g, graph_ids=ids, fill=-7).cpu()
    mine = np.zeros(g.num_graphs, dtype=bool)
    mine[ids] = True
    node_mine = mine[g.node_graph_ids()]
    edge_mine = node_mine[whole.rows[:, 0]]
    assert node_mine.any() and edge_mine.any() and not node_mine.all() and not edge_mine.all()
    assert np.array_equal(part.core[node_mine], whole.core[node_mine]) and (part.core[~node_mine] == -7).all()
    for f in ("truss", "support"):
        assert np.array_equal(getattr(part, f)[edge_mine], getattr(whole, f)[edge_mine]), f
        assert (getattr(part, f)[~edge_mine] == -7).all(), f
    assert (part.status[mine] == 0).all() and (part.status[~mine] == D.NOT_LAUNCHED).all()


def sparse_graph_of_words(words):
    """A sparse graph (a cycle with chords to the node 2 further on) whose workspace is just above ``words``."""
    n = 5000
    m = (words - n - 4) // 6 + 1
    assert n <= m <= 2 * n
    edges = [(i, (i + 1) % n) for i in range(n)] + [(i, (i + 2) % n) for i in range(m - n)]
    assert words < D.workspace_words(n, m) <= words + 6
    return n, edges


def test_graphs_above_the_limit_go_to_the_host(sets):
    small = sets["dense"].edge_lists()
    g = GraphSet.from_edge_lists(small[:2] + [sparse_graph_of_words(D.DEVICE_MAX_WORDS)] + small[2:])
    assert D._device_fit(g).tolist() == [True, True, False, True]
    with pytest.raises(RuntimeError, match="desco_core_truss_dev.*DESCO_CORE_TRUSS_DEV_MAX_WORDS"):
        D.decompose_device(g)
    with pytest.raises(RuntimeError, match="DESCO_CORE_TRUSS_DEV_MAX_WORDS"):
        D.decompose(g, backend="device")
    merged = D.decompose(g, backend="auto")
    assert D.last_backend == merged.last_backend == "device+host" and (merged.status == 0).all()
    want = D.decompose(g, backend="host")
    assert all(np.array_equal(getattr(merged, f), getattr(want, f)) for f in FIELDS)
    assert want.truss.max() >= 4 and want.truss[want.rows[:, 0] >= g.graph_ptr[2]].max() >= 3
    just_below = GraphSet.from_edge_lists([sparse_graph_of_words(D.DEVICE_MAX_WORDS - 6)])     # the largest that fits
    assert D._device_fit(just_below).all()
    got = D.decompose(just_below, backend="auto")
    assert D.last_backend == "device"
    want = D.decompose(just_below, backend="host")
    assert all(np.array_equal(getattr(got, f), getattr(want, f)) for f in FIELDS)


def test_entry_point_refuses_before_any_launch():
    """desco_core_truss_dev checks its arguments on the host: none of these calls reaches the GPU."""
    L = _lib.lib()
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data

    def call(graph_ptr=p, rowptr=p, col=p, G=1, M=3, entry_row=p, ids=None, num_ids=0, max_words=64, status=p):
        return L.desco_core_truss_dev(graph_ptr, rowptr, col, G, M, entry_row, ids, num_ids, max_words, p, p, p, status,
                                      None)

    def rejects(rc, word):
        assert rc == -1
        msg = L.desco_last_error()
        assert b"desco_core_truss_dev" in msg and word in msg, msg
        assert L.desco_rng_next(None, None, None) == -1          # (resets the message for the next case)

    assert call(G=0) == 0                                         # nothing to do
    rejects(call(G=-1), b"negative")
    rejects(call(M=-1), b"negative")
    rejects(call(ids=p, num_ids=-1), b"negative")
    rejects(call(max_words=-1), b"negative")
    rejects(call(max_words=40961), b"DESCO_CORE_TRUSS_DEV_MAX_WORDS")
    rejects(call(graph_ptr=None), b"graph_ptr is null")
    rejects(call(rowptr=None), b"rowptr is null")
    rejects(call(col=None), b"col is null")
    rejects(call(entry_row=None), b"entry_row is null")
    rejects(call(status=None), b"status is null")
    rejects(call(rowptr=p + 4), b"aligned")


def test_a_graph_over_the_launch_bound_is_guarded(sets):
    g = sets["dense"]
    words = D.workspace_words(*D._graph_sizes(g))
    bound = int(np.sort(words)[1])                                # the largest graph does not fit this launch
    over = words > bound
    assert over.sum() == 1
    ids = np.arange(g.num_graphs, dtype=np.int64)
    got = D._device(g, ids, torch.device("cuda"), True, True, fill=-7, max_words=bound).cpu()
    want = D.decompose(g, backend="host")
    assert got.status.tolist() == [-1 if o else 0 for o in over]
    node_over = over[g.node_graph_ids()]
    edge_over = node_over[want.rows[:, 0]]
    assert (got.core[node_over] == -7).all() and np.array_equal(got.core[~node_over], want.core[~node_over])
    for f in ("truss", "support"):
        assert (getattr(got, f)[edge_over] == -7).all() and \
            np.array_equal(getattr(got, f)[~edge_over], getattr(want, f)[~edge_over]), f
