"""The gfx950 graph generator (csrc/graph_gen_dev.hip) against its host twin: col, degrees and status bit for bit."""
import numpy as np
import pytest
import torch

from desco_amd import generators as G

pytestmark = pytest.mark.gpu
T32 = 1 << 32


def targets(n):
    top = n * (n - 1) // 2
    return [max(min(e, top), n - 1) for e in (n - 1, 2 * n, n * n // 4, top)]


def spec_of(rows, seed=3, graph_base=0):
    """rows: (family, n, param0, param1, threshold0, threshold1)"""
    r = np.array(rows, dtype=object)
    return G._Spec(r[:, 0], r[:, 1], r[:, 2:4].astype(np.int64), np.array(r[:, 4:6].tolist(), dtype=np.uint64), seed,
                   graph_base)


def by_edges(triples, seed=3, graph_base=0):
    f, n, e = zip(*triples)
    return G._spec(f, n, e, seed, graph_base)


def assert_same(d, h):
    d = d.cpu()
    for name in ("graph_ptr", "status", "deg", "rowptr", "col"):
        a, b = getattr(d, name), getattr(h, name)
        assert a.shape == b.shape and np.array_equal(a, b), name


def both(spec, **kw):
    h = G._host(spec, 4)
    d = G._device(spec, np.arange(spec.G, dtype=np.int64), torch.device("cuda"), **kw)
    assert_same(d, h)
    return h


@pytest.mark.parametrize("family", range(6), ids=G.FAMILIES)
def test_kernel_equals_twin_at_word_and_wave_boundaries(family):
    cases = [(family, n, e) for n in (1, 2, 3, 31, 32, 33, 63, 64, 65) for e in targets(n)[:3]]
    cases += [(family, 130, e) for e in targets(130)]
    both(by_edges(cases, seed=11))
    both(by_edges(cases, seed=(1 << 63) + 5, graph_base=1000))


@pytest.mark.parametrize("waves", (1, 4))
def test_both_workgroup_sizes_on_every_family(waves):
    cases = [(f, n, 2 * n + 3) for f in range(6) for n in (17, 65, 100)]
    both(by_edges(cases), waves=waves)


def test_er_far_below_the_connectivity_threshold():
    h = both(by_edges([(G.ER, 200, 100)] * 6, seed=5))
    assert (h.status >> 8).min() >= 50                   # many components: the connection at scale


def test_ws_every_edge_rewired_reaches_retries_and_the_fallback():
    """k = 2 with every edge rewired: a try is connected with a probability that falls only like n^-1/2 (1 in 6 at
    n = 1000), so retries are common but a hundred failures in a row are out of reach at any size the kernel takes;
    the Random fallback is entered through k // 2 == 0, which runs the same code behind the loop."""
    rows = [(G.WS, n, 2, n, T32, 0) for n in (12, 16, 20, 24, 30, 40, 50, 60) for _ in range(6)]
    rows += [(G.WS, n, k, n + 3, T32, 0) for n in (2, 12, 40) for k in (0, 1)]
    h = both(spec_of(rows, seed=7))
    tries = h.status & 0xff
    assert ((tries > 1) & (tries <= 100)).any(), tries
    assert (tries == G.WS_FELL_BACK).any(), tries


def test_random_at_nine_tenths_of_the_maximum():
    both(by_edges([(G.RANDOM, n, int(0.9 * n * (n - 1) // 2)) for n in (20, 64, 100)]))


def test_eba_all_three_branches_and_saturation():
    rows = []
    for n, m in ((12, 2), (20, 5), (40, 3), (64, 1)):
        rows += [(G.EBA, n, m, 0, int(0.5 * T32), int(0.95 * T32)),      # adding until saturated, then rewiring
                 (G.EBA, n, m, 0, int(0.05 * T32), int(0.9 * T32)),     # mostly rewiring
                 (G.EBA, n, m, 0, 0, 0)]                                # growth alone
    both(spec_of(rows, seed=9))


def test_power_at_m_one_and_with_every_triangle_step_taken():
    rows = [(G.POWER, n, 1, 0, int(0.5 * T32), 0) for n in (2, 10, 65)]
    rows += [(G.POWER, n, m, 0, T32, 0) for n, m in ((10, 3), (40, 5), (65, 8), (100, 2))]
    both(spec_of(rows, seed=13))


def test_mixed_launch_slices_and_repeats():
    fam, n, e = G.schedule(64, 10, 120, seed=2)
    fam = np.arange(64, dtype=np.int32) % 6              # all six families
    spec = G._spec(fam, n, e, 21, 0)
    h = both(spec)
    ids = np.arange(64, dtype=np.int64)
    again = G._device(spec, ids, torch.device("cuda"))
    assert_same(again, h)
    lo, hi = spec.subset(ids[:30]), spec.subset(ids[30:])
    a = G._device(lo, ids[:30], torch.device("cuda")).cpu()
    b = G._device(hi, ids[:34], torch.device("cuda")).cpu()
    assert np.array_equal(np.concatenate([a.deg, b.deg]), h.deg)
    assert np.array_equal(np.concatenate([a.status, b.status]), h.status)
    cut = int(h.graph_ptr[30])
    assert np.array_equal(np.concatenate([a.col, b.col + cut]), h.col)


def test_launch_bound_below_one_graph():
    spec = by_edges([(G.BA, 20, 40), (G.ER, 90, 300), (G.RANDOM, 25, 50)])
    bound = int(G.workspace_words(25))
    d = G._device(spec, np.arange(3, dtype=np.int64), torch.device("cuda"), max_words=bound).cpu()
    h = G._host(spec, 1)
    assert d.status[1] == -1 and (d.deg[20:110] == 0).all()          # refused, rows untouched
    assert np.array_equal(d.status[[0, 2]], h.status[[0, 2]])
    assert np.array_equal(d.deg[:20], h.deg[:20]) and np.array_equal(d.deg[110:], h.deg[110:])
    left = h.col[:h.rowptr[20]]
    right = h.col[h.rowptr[110]:]
    assert np.array_equal(d.col[:len(left)], left) and np.array_equal(d.col[len(left):], right)
    L = G._lib.lib()
    assert L.desco_graph_gen_dev(*([None] * 4), 1, None, 0, 0, 0, None, None, 0, 0, G.DEVICE_MAX_WORDS + 1, 0, 0,
                                 None, None, None, None) == -1
    assert b"DESCO_GRAPH_GEN_DEV_MAX_WORDS" in L.desco_last_error()


def test_auto_merges_a_graph_above_the_device_limit(monkeypatch):
    monkeypatch.setattr(G, "AUTO_TAKES_DEVICE", True)
    f, n, e = [G.BA, G.ER, G.WS], [30, 1100, 50], [60, 2400, 100]
    assert G.workspace_words(1100) > G.DEVICE_MAX_WORDS
    got = G.generate(f, n, e, seed=4, backend="auto")
    assert G.last_backend == "device+host"
    want = G.generate(f, n, e, seed=4, backend="host")
    for name in ("graph_ptr", "rowptr", "col"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), name


def test_the_device_route_refuses_a_graph_above_its_limit_by_name():
    """backend="device" and generate_device have no host to fall back on: a graph above DEVICE_MAX_WORDS raises,
    naming the limit, whether it stands alone or among graphs that fit -- it never comes back as empty rows."""
    assert G.workspace_words(1100) > G.DEVICE_MAX_WORDS
    for f, n, e in (([G.BA], [1100], [2400]), ([G.ER, G.BA, G.WS], [30, 1100, 50], [60, 2400, 100])):
        with pytest.raises(RuntimeError, match="DESCO_GRAPH_GEN_DEV_MAX_WORDS"):
            G.generate(f, n, e, seed=4, backend="device")
        with pytest.raises(RuntimeError, match="DESCO_GRAPH_GEN_DEV_MAX_WORDS"):
            G.generate_device(f, n, e, seed=4)
        with pytest.raises(RuntimeError, match="DESCO_GRAPH_GEN_DEV_MAX_WORDS"):
            G.generate_device(f, n, e, seed=4, max_words=int(G.workspace_words(1100)))
    edge = G.generate_device([G.BA], [1056], [2400], seed=4).cpu()          # the largest graph the kernel holds
    assert G.workspace_words(1056) <= G.DEVICE_MAX_WORDS < G.workspace_words(1057)
    assert edge.status[0] == 0 and np.array_equal(edge.col, G.generate([G.BA], [1056], [2400], seed=4, backend="host").col)


def test_the_1827_schedule_on_the_device_equals_the_twin():
    got = G.gen_synthetic(1827, seed=0, backend="device")
    assert G.last_backend == "device"
    want = G.gen_synthetic(1827, seed=0, backend="host")
    for name in ("graph_ptr", "rowptr", "col"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), name


def test_canonical_counts_of_a_generated_set_device_route_equals_host_route():
    from helpers import standard_queries
    from desco_amd import groundtruth as gt
    _, queries = standard_queries()
    graphs = G.gen_synthetic(24, 10, 40, seed=6, backend="device")
    dev = gt.canonical_counts(graphs, queries, backend="device")
    host = gt.canonical_counts(graphs, queries, backend="host")
    assert dev.shape[0] == graphs.num_nodes and torch.equal(dev.cpu(), host.cpu())
