"""Clique census on the GPU (csrc/clique_census_dev.hip): the kernels against the host twins bit for bit on the named
families (every out-degree at which the launch changes, a graph that branches at every level, a hub above a wave's
lanes, more roots than lanes), slices of a graph set, routing above the two device limits, the refusals of the entry
points and the kernels' own guards."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import clique_reference as R  # noqa: E402
from helpers import random_family_graphs  # noqa: E402
from desco_amd import _lib, cliques as C, decomposition as D, synthetic  # noqa: E402
from desco_amd.graphs import GraphSet  # noqa: E402

FIELDS = ("graph_cliques", "node_cliques", "omega", "key")


@pytest.fixture(scope="module")
def sets():
    return {"families": R.families(), "dense": R.dense_random(),
            "random_families": GraphSet.from_edge_lists(random_family_graphs(43, 90)),
            "syn": synthetic.WORKLOADS["syn_1827"]().subset(300, 420), "cox2": synthetic.WORKLOADS["cox2"]()}


@pytest.fixture(scope="module")
def twins(sets):
    return {name: C.clique_census(g, kmax=8, backend="host") for name, g in sets.items()}


def same(got, want, fields=FIELDS):
    for f in fields:
        assert np.array_equal(getattr(got, f), getattr(want, f)), f


@pytest.mark.parametrize("name", ["families", "dense", "random_families", "syn", "cox2"])
def test_device_equals_host_twin(sets, twins, name):
    g, want = sets[name], twins[name]
    key, core, status = C.peel_order_device(g)
    assert key.is_cuda and key.dtype == core.dtype == status.dtype == torch.int32 and (status == 0).all()
    want_key, want_core = C.peel_order(g, backend="host")
    assert np.array_equal(key.cpu().numpy(), want_key) and np.array_equal(core.cpu().numpy(), want_core)
    assert np.array_equal(want_core, D.decompose_device(g, truss=False).cpu().core)
    got = C.clique_census_device(g, kmax=8)
    for f in FIELDS + ("status",):
        x = getattr(got, f)
        assert x.is_cuda and x.dtype == (torch.int64 if f.endswith("cliques") else torch.int32), f
    assert (got.status == 0).all()
    same(got.cpu(), want)
    if name != "cox2":
        assert want.graph_cliques[:, 4].max() >= 1 and want.omega.max() >= 5      # a constant answer must not pass
    else:
        assert want.omega.max() == 2 and want.graph_cliques[:, 1].min() >= 1      # molecules: edges are their cliques
    assert (want.node_cliques[:, 0] == 1).all() and np.array_equal(want.node_cliques[:, 1], np.diff(g.rowptr))
    res = C.clique_census(g, kmax=8, backend="device")
    assert C.last_backend == res.last_backend == "device"
    same(res, want)
    auto = C.clique_census(g, kmax=8, backend="auto")
    assert C.last_backend == "device"
    same(auto, want)


def test_every_out_degree_bucket_edge_is_a_clique_of_the_families(sets, twins):
    g, want = sets["families"], twins["families"]
    names = [nm for nm, _, _ in R.family_graphs()]
    top = C._graph_max(g, C.out_degrees(g, want.key))
    for k in (9, 10, 17, 18, 33, 34, 64, 65):                    # out-degree 8, 9, 16, 17, 32, 33, 63, 64
        i = names.index(f"K{k}")
        assert top[i] == k - 1 and want.omega[i] == k
        assert want.graph_cliques[i].tolist() == R.complete_closed_form(k, 8)[0]
    i = names.index("star 200")
    assert top[i] == 1 and want.graph_cliques[i, :3].tolist() == [201, 200, 0]
    assert top[names.index("K3x7")] > 8 and int(np.diff(g.graph_ptr)[names.index("path 150")]) > 64
    dev_top = C._graph_max(g, C.out_degrees(g, C.peel_order_device(g)[0]).cpu().numpy())
    assert np.array_equal(dev_top, top)


@pytest.mark.parametrize("kmax", [1, 2, 64])
def test_kmax_1_2_and_64(sets, kmax):
    g = sets["families"]
    want = C.clique_census(g, kmax=kmax, backend="host")
    got = C.clique_census_device(g, kmax=kmax)
    assert (got.status == 0).all() and got.graph_cliques.shape == (g.num_graphs, kmax)
    same(got.cpu(), want)
    names = [nm for nm, _, _ in R.family_graphs()]
    assert want.omega[names.index("K65")] == 65 and want.omega[names.index("K3x7")] == 7      # exact whatever kmax is
    if kmax == 64:
        assert want.graph_cliques[names.index("K65")].tolist() == R.complete_closed_form(65, 64)[0]


def test_without_node_columns_and_empty_sets(sets, twins):
    g, want = sets["dense"], twins["dense"]
    got = C.clique_census_device(g, kmax=8, nodes=False)
    assert got.node_cliques is None and (got.status == 0).all()
    same(got.cpu(), want, ("graph_cliques", "omega", "key"))
    empty = C.clique_census_device(GraphSet.from_edge_lists([])).cpu()
    assert empty.graph_cliques.shape == (0, 8) and empty.node_cliques.shape == (0, 8) and empty.status.shape == (0,)
    bare = C.clique_census_device(GraphSet.from_edge_lists([(5, []), (0, []), (1, [])]), kmax=3).cpu()
    assert bare.graph_cliques.tolist() == [[5, 0, 0], [0, 0, 0], [1, 0, 0]] and bare.omega.tolist() == [1, 0, 1]
    assert bare.node_cliques.tolist() == [[1, 0, 0]] * 6 and bare.status.tolist() == [0, 0, 0]
    no_nodes = C.clique_census_device(GraphSet.from_edge_lists([(0, []), (0, [])]), kmax=2).cpu()
    assert no_nodes.graph_cliques.tolist() == [[0, 0], [0, 0]] and no_nodes.status.tolist() == [0, 0]


def test_the_counts_do_not_depend_on_the_key(sets, twins):
    g, want = sets["dense"], twins["dense"]
    key = np.random.default_rng(3).permutation(g.num_nodes).astype(np.int32)
    assert C._graph_max(g, C.out_degrees(g, key)).max() <= C.DEVICE_MAX_OUT
    got = C.clique_census_device(g, kmax=8, key=key).cpu()
    assert (got.status == 0).all() and np.array_equal(got.key, key)
    same(got, want, ("graph_cliques", "node_cliques", "omega"))


def test_a_slice_writes_exactly_its_graphs_rows(sets):
    g = sets["random_families"]
    whole = C.clique_census_device(g, kmax=5).cpu()
    ids = np.arange(0, g.num_graphs, 3)
    part = C.clique_census_device(g, kmax=5, graph_ids=ids, fill=-7).cpu()
    mine = np.zeros(g.num_graphs, dtype=bool)
    mine[ids] = True
    node_mine = mine[g.node_graph_ids()]
    assert node_mine.any() and not node_mine.all()
    for f in ("graph_cliques", "omega"):
        assert np.array_equal(getattr(part, f)[mine], getattr(whole, f)[mine]) and (getattr(part, f)[~mine] == -7).all(), f
    for f in ("node_cliques", "key"):
        assert np.array_equal(getattr(part, f)[node_mine], getattr(whole, f)[node_mine]), f
        assert (getattr(part, f)[~node_mine] == -7).all(), f
    assert (part.status[mine] == 0).all() and (part.status[~mine] == C.NOT_LAUNCHED).all()
    key, core, status = (x.cpu().numpy() for x in C.peel_order_device(g, graph_ids=ids, fill=-7))
    assert np.array_equal(key[node_mine], whole.key[node_mine]) and (key[~node_mine] == -7).all()
    assert (core[~node_mine] == -7).all() and (status[~mine] == C.NOT_LAUNCHED).all()


def sparse_graph_of_words(words):
    """A sparse graph (a cycle with chords to the node 2 further on) whose peel workspace is just above ``words``."""
    n = 6000
    m = (words - 8 - 2 * n) // 2 + 1
    assert 2 * n <= m <= 3 * n
    edges = [(i, (i + 1) % n) for i in range(n)] + [(i, (i + 2) % n) for i in range(min(m - n, n))] + \
        [(i, (i + 3) % n) for i in range(max(m - 2 * n, 0))]
    assert words < C.peel_words(n, len(edges)) <= words + 2
    return n, edges


def test_graphs_above_a_limit_go_to_the_host(sets):
    small = sets["dense"].edge_lists()
    k66 = (66, R.clique(66))
    g = GraphSet.from_edge_lists(small[:2] + [k66] + small[2:4])
    with pytest.raises(RuntimeError, match="desco_clique_census_dev.*DESCO_CLIQUE_DEV_MAX_OUT"):
        C.clique_census_device(g)
    with pytest.raises(RuntimeError, match="DESCO_CLIQUE_DEV_MAX_OUT"):
        C.clique_census(g, backend="device")
    want = C.clique_census(g, kmax=8, backend="host")
    merged = C.clique_census(g, kmax=8, backend="auto")
    assert C.last_backend == merged.last_backend == "device+host" and (merged.status == 0).all()
    same(merged, want)
    assert want.omega.tolist()[2] == 66 and want.graph_cliques[2].tolist() == R.complete_closed_form(66, 8)[0]

    g = GraphSet.from_edge_lists(small[:2] + [sparse_graph_of_words(C.DEVICE_MAX_WORDS)] + small[2:4])
    assert C._peel_fit(g).tolist() == [True, True, False, True, True]
    with pytest.raises(RuntimeError, match="desco_peel_order_dev.*DESCO_PEEL_DEV_MAX_WORDS"):
        C.clique_census_device(g)
    with pytest.raises(RuntimeError, match="DESCO_PEEL_DEV_MAX_WORDS"):
        C.peel_order(g, backend="device")
    want = C.clique_census(g, kmax=8, backend="host")
    merged = C.clique_census(g, kmax=8, backend="auto")
    assert C.last_backend == merged.last_backend == "device+host" and (merged.status == 0).all()
    same(merged, want)
    assert want.omega[2] >= 3 and want.omega.max() >= 5
    key, core = C.peel_order(g, backend="auto")
    assert C.last_backend == "device+host" and np.array_equal(key, want.key)
    just_below = GraphSet.from_edge_lists([sparse_graph_of_words(C.DEVICE_MAX_WORDS - 2)])      # the largest that fits
    assert C._peel_fit(just_below).all()
    got = C.clique_census(just_below, kmax=4, backend="auto")
    assert C.last_backend == "device"
    same(got, C.clique_census(just_below, kmax=4, backend="host"))


def test_entry_points_refuse_before_any_launch():
    """Both device entry points check their arguments on the host: none of these calls reaches the GPU."""
    L = _lib.lib()
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data

    def rejects(rc, name, word):
        assert rc == -1
        msg = L.desco_last_error()
        assert name in msg and word in msg, msg
        assert L.desco_rng_next(None, None, None) == -1          # (resets the message for the next case)

    def peel(graph_ptr=p, rowptr=p, col=p, G=1, ids=None, num_ids=0, max_words=64, key=p, status=p):
        return L.desco_peel_order_dev(graph_ptr, rowptr, col, G, ids, num_ids, max_words, key, p, status, None)

    name = b"desco_peel_order_dev"
    assert peel(G=0) == 0                                         # nothing to do
    rejects(peel(G=-1), name, b"negative")
    rejects(peel(ids=p, num_ids=-1), name, b"negative")
    rejects(peel(max_words=-1), name, b"negative")
    rejects(peel(max_words=40961), name, b"DESCO_PEEL_DEV_MAX_WORDS")
    rejects(peel(graph_ptr=None), name, b"graph_ptr is null")
    rejects(peel(rowptr=None), name, b"rowptr is null")
    rejects(peel(col=None), name, b"col is null")
    rejects(peel(key=None), name, b"key_out is null")
    rejects(peel(status=None), name, b"status is null")
    rejects(peel(rowptr=p + 4), name, b"aligned")

    def census(graph_ptr=p, rowptr=p, col=p, G=1, key=p, kmax=8, ids=None, num_ids=0, max_out=8, gc=p, status=p):
        return L.desco_clique_census_dev(graph_ptr, rowptr, col, G, key, kmax, ids, num_ids, max_out, gc, p, p, status,
                                         None)

    name = b"desco_clique_census_dev"
    assert census(G=0) == 0
    rejects(census(G=-1), name, b"negative")
    rejects(census(ids=p, num_ids=-1), name, b"negative")
    rejects(census(max_out=-1), name, b"negative")
    rejects(census(max_out=65), name, b"DESCO_CLIQUE_DEV_MAX_OUT")
    rejects(census(kmax=0), name, b"DESCO_CLIQUE_MAX_K")
    rejects(census(kmax=65), name, b"DESCO_CLIQUE_MAX_K")
    rejects(census(graph_ptr=None), name, b"graph_ptr is null")
    rejects(census(rowptr=None), name, b"rowptr is null")
    rejects(census(col=None), name, b"col is null")
    rejects(census(key=None), name, b"key is null")
    rejects(census(status=None), name, b"status is null")
    rejects(census(gc=p + 4), name, b"aligned")


def test_the_kernels_guard_themselves(sets, twins):
    """Hand-made arrays: a graph with an id of another graph, and one with an unsorted row, between two good graphs.
    Both kernels give them status -1 and leave their rows untouched; the good graphs are counted."""
    tri = [(0, 1), (0, 2), (1, 2), (2, 3)]
    good = GraphSet.from_edge_lists([(4, tri)] * 4)
    col = good.col.copy()
    e1 = int(good.rowptr[4])                                     # graph 1, node 0: its row (1, 2) -> (1, 9)
    assert col[e1:e1 + 2].tolist() == [5, 6]
    col[e1 + 1] = 9
    e2 = int(good.rowptr[8 + 2])                                 # graph 2, node 2: its row (0, 1, 3) -> (1, 0, 3)
    assert col[e2:e2 + 3].tolist() == [8, 9, 11]
    col[e2], col[e2 + 1] = 9, 8
    bad = GraphSet(good.graph_ptr, good.rowptr, col)
    want = C.clique_census(good, kmax=4, backend="host")
    key, core, status = (x.cpu().numpy() for x in C.peel_order_device(bad, fill=-7))
    assert status.tolist() == [0, -1, -1, 0]
    assert (key[4:12] == -7).all() and (core[4:12] == -7).all()
    assert np.array_equal(key[:4], want.key[:4]) and np.array_equal(key[12:], want.key[12:])
    for given in (None, want.key):                               # the census kernel behind the peel's refusal, and alone
        got = C.clique_census_device(bad, kmax=4, fill=-7, key=given).cpu()
        assert got.status.tolist() == [0, -1, -1, 0]
        assert (got.graph_cliques[1:3] == -7).all() and (got.omega[1:3] == -7).all() and (got.node_cliques[4:12] == -7).all()
        for i in (0, 3):
            assert np.array_equal(got.graph_cliques[i], want.graph_cliques[i]) and got.omega[i] == 3
            assert np.array_equal(got.node_cliques[4 * i:4 * i + 4], want.node_cliques[4 * i:4 * i + 4])


def test_a_graph_over_the_launch_bound_is_guarded(sets, twins):
    g, want = sets["dense"], twins["dense"]
    top = C._graph_max(g, C.out_degrees(g, want.key))
    bound = int(np.sort(top)[-2])                                 # the graph of the largest out-degree does not fit
    over = top > bound
    assert over.sum() == 1 and bound >= 4
    ids = np.arange(g.num_graphs, dtype=np.int64)
    got = C._device(g, ids, torch.device("cuda"), 8, True, fill=-7, max_out=bound)[0].cpu()
    assert got.status.tolist() == [-1 if o else 0 for o in over]
    node_over = over[g.node_graph_ids()]
    assert (got.graph_cliques[over] == -7).all() and (got.omega[over] == -7).all()
    assert (got.node_cliques[node_over] == -7).all()
    assert np.array_equal(got.graph_cliques[~over], want.graph_cliques[~over])
    assert np.array_equal(got.node_cliques[~node_over], want.node_cliques[~node_over])
    assert np.array_equal(got.omega[~over], want.omega[~over])
    key, core, status = C.peel_order_device(g)
    words = C.peel_words(*C._graph_sizes(g))
    small = int(np.sort(words)[-2])
    key2 = torch.full_like(key, -7)
    status2 = torch.full_like(status, C.NOT_LAUNCHED)
    C._peel_launches(g, C._Upload(g, key.device), ids, key.device, key2, None, status2, max_words=small)
    big = words > small
    assert status2.cpu().tolist() == [-1 if b else 0 for b in big] and big.sum() == 1
    node_big = big[g.node_graph_ids()]
    assert (key2.cpu().numpy()[node_big] == -7).all()
    assert np.array_equal(key2.cpu().numpy()[~node_big], key.cpu().numpy()[~node_big])
