"""Data-set statistics on the MI355X (csrc/subgraph_stats_dev.hip) against the host twin (csrc/subgraph_stats.cpp, itself
pinned to networkx by tests/test_subgraph_stats_host.py).  The six integers must match bit for bit; clustering_sum
within 1e-12 absolute -- each comparison prints whether it was in fact bit-identical (the two sides form the same terms
and add them in the same order, so it should be)."""
import numpy as np
import pytest
import torch

from desco_amd import _lib, analysis, synthetic
from desco_amd.graphs import GraphSet
from test_subgraph_stats_host import closed_form_problem, flat_sets, ints_of

pytestmark = pytest.mark.gpu
CLUSTERING_TOL = 1e-12
SIZES = (1, 2, 63, 64, 65, 128, 129, 512, 513, 1024, 1025)


def assert_equal_stats(name, dev, host):
    for f in analysis.STAT_FIELDS:
        assert np.array_equal(getattr(dev, f), getattr(host, f)), (name, f)
    d = float(np.abs(dev.clustering_sum - host.clustering_sum).max()) if len(dev) else 0.0
    same = dev.clustering_sum.tobytes() == host.clustering_sum.tobytes()
    print(f"[parity] {name}: {len(dev)} sets, integers equal, clustering_sum max |d| = {d:.2e} "
          f"(gate {CLUSTERING_TOL:.0e}), bit-identical: {same}")
    assert d <= CLUSTERING_TOL, name
    return same


@pytest.fixture(scope="module")
def sized():
    """One sparse graph of 1100 nodes (a few components, triangles) and one set per size in SIZES, plus the contiguous
    prefix of every size: (GraphSet, set_ptr, set_nodes, host statistics)."""
    rng = np.random.default_rng(17)
    n = 1100
    edges = [(v, v + 1) for v in range(n - 1) if v % 97]
    edges += [(int(a), int(b)) for a, b in rng.integers(0, n, size=(2200, 2))]
    edges += [(v, v + 2) for v in range(0, n - 2, 3)]
    gs = GraphSet.from_edge_lists([(n, edges)])
    sets = [(0, sorted(rng.choice(n, size=k, replace=False).tolist())) for k in SIZES]
    sets += [(0, range(k)) for k in SIZES]
    ptr, nodes = flat_sets(gs, sets)
    host = analysis.subgraph_statistics(gs, ptr, nodes, backend="host")
    assert host.triangles.sum() > 0 and (host.n < host.members).any() and host.diameter.max() > 5
    return gs, ptr, nodes, host


def test_every_size_and_the_host_route(sized):
    gs, ptr, nodes, host = sized
    dev = analysis.subgraph_statistics(gs, ptr, nodes, backend="device")
    assert analysis.last_stats_backend == "device+host"           # the two sets of 1025 members
    assert_equal_stats("sizes 1..1025, all five buckets in one call", dev, host)
    assert dev.members.tolist() == list(SIZES) * 2
    keep = np.nonzero(np.diff(ptr) <= analysis.DEVICE_SET_LIMIT)[0]
    sub_ptr = np.concatenate([[0], np.cumsum(np.diff(ptr)[keep])])
    sub_nodes = np.concatenate([nodes[ptr[k]:ptr[k + 1]] for k in keep])
    dev = analysis.subgraph_statistics(gs, sub_ptr, sub_nodes, backend="device")
    assert analysis.last_stats_backend == "device"
    assert np.array_equal(dev.dist_sum, host.dist_sum[keep])


def test_closed_forms_on_the_device():
    cases, gs, sets = closed_form_problem()
    ptr, nodes = flat_sets(gs, sets)
    dev = analysis.subgraph_statistics(gs, ptr, nodes, backend="device")
    assert analysis.last_stats_backend == "device"
    for k, (name, c) in enumerate(cases.items()):
        assert ints_of(dev, k) == c[2], name
        assert dev.clustering_sum[k] == c[3], name
    assert_equal_stats("closed forms", dev, analysis.subgraph_statistics(gs, ptr, nodes, backend="host"))


def test_hub_row():
    """A member with 200 neighbours inside a 300-member set: its row is built by a whole wave."""
    rng = np.random.default_rng(5)
    n = 400
    others = [v for v in range(n) if v != 150]
    edges = [(150, int(v)) for v in rng.choice(others, size=200, replace=False)]
    edges += [(int(a), int(b)) for a, b in rng.integers(0, n, size=(500, 2))]
    gs = GraphSet.from_edge_lists([(n, edges)])
    assert gs.rowptr[151] - gs.rowptr[150] >= 200
    members = sorted(set(rng.choice(others, size=299, replace=False).tolist()) | {150})
    ptr, nodes = flat_sets(gs, [(0, members), (0, range(n))])
    host = analysis.subgraph_statistics(gs, ptr, nodes, backend="host")
    assert host.triangles[0] > 0
    assert_equal_stats("hub of degree 200", analysis.subgraph_statistics(gs, ptr, nodes, backend="device"), host)


def test_forced_into_the_widest_bucket(sized):
    gs, ptr, nodes, _ = sized
    natural = analysis.subgraph_statistics(gs, ptr, nodes, backend="device")
    wide = analysis.subgraph_statistics(gs, ptr, nodes, backend="device", words=16)
    for f in analysis.STAT_FIELDS:
        assert np.array_equal(getattr(natural, f), getattr(wide, f)), f
    assert natural.clustering_sum.tobytes() == wide.clustering_sum.tobytes()
    # and a bucket too small refuses: everything above 64 members comes back from the host
    narrow = analysis.subgraph_statistics(gs, ptr, nodes, backend="device", words=1)
    assert analysis.last_stats_backend == "device+host"
    assert natural.clustering_sum.tobytes() == narrow.clustering_sum.tobytes()
    assert np.array_equal(natural.dist_sum, narrow.dist_sum)


def test_a_slice_of_the_ids_equals_the_full_launch(sized):
    gs, ptr, nodes, host = sized
    dev = torch.device("cuda")
    rowptr_d, col_d = torch.from_numpy(gs.rowptr).to(dev), torch.from_numpy(gs.col).to(dev)
    ptr_d, nodes_d = torch.from_numpy(ptr).to(dev), torch.from_numpy(nodes).to(dev)
    S = len(ptr) - 1
    ids = torch.nonzero((ptr_d[1:] - ptr_d[:-1]) <= 128).reshape(-1)            # W = 2 takes sizes 1 .. 128
    assert ids.numel() == 12

    def run(which):
        oi = torch.full((S, 6), -5, dtype=torch.int64, device=dev)
        of = torch.full((S,), -5.0, dtype=torch.float64, device=dev)
        analysis.subgraph_stats_launch(rowptr_d, col_d, gs.num_nodes, ptr_d, nodes_d, which, 2, oi, of)
        torch.cuda.synchronize()
        return oi.cpu().numpy(), of.cpu().numpy()

    full_i, full_f = run(ids)
    part = ids[3:8].contiguous()
    part_i, part_f = run(part)
    rows = part.cpu().numpy()
    assert np.array_equal(part_i[rows], full_i[rows]) and part_f[rows].tobytes() == full_f[rows].tobytes()
    rest = np.setdiff1d(np.arange(S), rows)
    assert (part_i[rest] == -5).all() and (part_f[rest] == -5.0).all()          # only the rows of the ids are written
    assert np.array_equal(full_i[ids.cpu().numpy(), 4], host.dist_sum[ids.cpu().numpy()])
    # a set that does not fit the bucket: members and n = -1, nothing else
    big = torch.nonzero((ptr_d[1:] - ptr_d[:-1]) == 513).reshape(-1)
    big_i, big_f = run(big)
    assert big_i[big.cpu().numpy()].tolist() == [[513, -1, 0, 0, 0, 0]] * 2 and (big_f[big.cpu().numpy()] == 0).all()


@pytest.mark.parametrize("which", ["cox2", "syn_1827", "syn_mid"])
def test_neighborhood_statistics(which):
    from desco_amd.partition import build_partition_device
    # syn_mid: ten graphs of 60 .. 250 nodes, whose neighborhoods fill the buckets of 1 and 2 words
    gs = {"cox2": lambda: synthetic.cox2_shaped(64), "syn_1827": lambda: synthetic.syn_1827_shaped().subset(300, 420),
          "syn_mid": lambda: synthetic.syn_1827_shaped(60).subset(40, 50)}[which]()
    part = build_partition_device(gs, 4)
    if which == "syn_mid":
        assert {w for w, _ in analysis.device_buckets(analysis.neighborhood_sets_device(part, gs)[0])[0]} >= {1, 2}
    dev = analysis.neighborhood_statistics(gs, depth=4, backend="device", partition=part)
    assert analysis.last_stats_backend == "device"
    assert part.downloads["count_orig"] == 0 and part.downloads["vcol"] == 0 and part.downloads["count_ptr"] == 0
    host = analysis.neighborhood_statistics(gs, depth=4, backend="host")
    assert np.array_equal(dev.neigh_index, part.device_arrays["neigh_index"].cpu().numpy())
    assert np.array_equal(dev.neigh_index, host.neigh_index)
    assert_equal_stats(f"neighborhoods of {which}", dev, host)
    assert (dev.n == dev.members).all() and dev.m.min() >= 1
    auto = analysis.neighborhood_statistics(gs, depth=4)                        # builds its own device partition
    assert analysis.last_stats_backend == "device" and np.array_equal(auto.dist_sum, host.dist_sum)


def test_bad_content_goes_to_the_host_which_names_it():
    gs = GraphSet.from_edge_lists([(5, [(0, 1), (1, 2), (2, 3), (3, 4)])])
    ptr = np.array([0, 3], dtype=np.int64)
    with pytest.raises(RuntimeError, match="strictly ascending"):
        analysis.subgraph_statistics(gs, ptr, np.array([2, 1, 0]), backend="device")
    with pytest.raises(RuntimeError, match="outside the graph"):
        analysis.subgraph_statistics(gs, ptr, np.array([1, 2, 9]), backend="device")


def test_bad_arguments_are_refused_before_any_launch():
    dev = torch.device("cuda")
    L = _lib.lib()
    gs = GraphSet.from_edge_lists([(5, [(0, 1), (1, 2), (2, 3), (3, 4)])])
    t = dict(rowptr=torch.from_numpy(gs.rowptr).to(dev), col=torch.from_numpy(gs.col).to(dev),
             set_ptr=torch.tensor([0, 3], device=dev), set_nodes=torch.tensor([0, 1, 2], dtype=torch.int32, device=dev),
             set_ids=torch.zeros(1, dtype=torch.int64, device=dev),
             out_i64=torch.full((1, 6), -5, dtype=torch.int64, device=dev),
             out_f64=torch.full((1,), -5.0, dtype=torch.float64, device=dev))
    st = torch.cuda.current_stream().cuda_stream

    def call(words=1, num_ids=1, **over):
        p = {k: v.data_ptr() for k, v in t.items()}
        p.update(over)
        rc = L.desco_subgraph_stats_dev(p["rowptr"], p["col"], gs.num_nodes, p["set_ptr"], p["set_nodes"], p["set_ids"],
                                        num_ids, words, p["out_i64"], p["out_f64"], st)
        return rc, L.desco_last_error().decode()

    for words in (0, 3, 5, 32, -1):
        rc, msg = call(words=words)
        assert rc != 0 and "words" in msg, (words, msg)
    for name in t:
        rc, msg = call(**{name: None})
        assert rc != 0 and name in msg and "null" in msg, (name, msg)
    rc, msg = call(num_ids=-1)
    assert rc != 0 and "num_ids" in msg
    rc, msg = call(out_i64=t["out_i64"].data_ptr() + 4)
    assert rc != 0 and "aligned" in msg
    torch.cuda.synchronize()
    assert (t["out_i64"] == -5).all() and (t["out_f64"] == -5.0).all()          # nothing ran
    assert call(num_ids=0)[0] == 0
    rc, _ = call()
    torch.cuda.synchronize()
    assert rc == 0 and t["out_i64"].cpu().tolist() == [[3, 3, 2, 2, 8, 0]]
    with pytest.raises(RuntimeError, match="on the GPU"):
        analysis.subgraph_stats_launch(t["rowptr"].cpu(), t["col"], 5, t["set_ptr"], t["set_nodes"], t["set_ids"], 1,
                                       t["out_i64"], t["out_f64"])
