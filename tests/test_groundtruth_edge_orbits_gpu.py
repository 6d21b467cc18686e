"""Exact per-edge orbit counts on the device (csrc/groundtruth_dev.hip, ge_count_kernel) against the host enumerator --
integers, bit for bit, in both forms -- and once against the brute-force yardstick tests/edge_orbit_reference.py."""
import networkx as nx
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import edge_orbit_reference as R  # noqa: E402
from desco_amd.graphs import GraphSet  # noqa: E402
from desco_amd.groundtruth import (census_classes, edge_orbit_columns, edge_orbit_counts,  # noqa: E402
                                   edge_orbit_counts_device, edge_orbit_rows)

CENSUS = [q for k in (2, 3, 4, 5) for q in census_classes(k)]
COLS = edge_orbit_columns()
FORMS = [True, False]
LEAVES = 70


def edges_of(g):
    return (g.number_of_nodes(), [tuple(e) for e in g.edges()])


def shuffled(graph, rng):
    n, edges = graph
    p = rng.permutation(n)
    return (n, [(int(p[a]), int(p[b])) for a, b in edges])


def families():
    rng = np.random.default_rng(23)
    out = [edges_of(nx.path_graph(9)), edges_of(nx.cycle_graph(11)), edges_of(nx.star_graph(12)),
           edges_of(nx.wheel_graph(8)), edges_of(nx.complete_graph(5)), edges_of(nx.complete_graph(6)),
           edges_of(nx.petersen_graph()), (0, []), (1, []), (2, [(0, 1)]),
           (12, [(0, 5), (5, 7), (7, 0), (7, 9), (2, 9)])]                   # isolated nodes 1, 3, 4, 6, 8, 10, 11
    out += [shuffled(edges_of(nx.gnp_random_graph(int(rng.integers(6, 13)), float(rng.uniform(0.2, 0.6)), seed=70 + i)),
                     rng) for i in range(4)]
    return out


def hard_shapes():
    """The smallest shapes at which the kernel can go wrong beyond the families."""
    chords = [(0, 1), (1, 2), (5, 40), (68, 69), (3, 69)]
    # a wave's third-node candidates exceed its 64 lanes: the round-robin dealing wraps.  Hub = the largest id (its items
    # hold every subset, the candidates come from v's row), then hub = the smallest id (they come from u0's row)
    hub_last = (LEAVES + 1, [(LEAVES, i) for i in range(LEAVES)] + chords)
    hub_first = (LEAVES + 1, [(0, i + 1) for i in range(LEAVES)] + [(a + 1, b + 1) for a, b in chords])
    return [hub_last, hub_first, edges_of(nx.complete_graph(12))]           # K12: every class, long runs, shared rows


def many_small():
    """About 40 small graphs whose edge counts are no multiples of the four waves of a block"""
    rng = np.random.default_rng(5)
    out = [shuffled(edges_of(nx.gnp_random_graph(int(rng.integers(3, 9)), 0.5, seed=200 + i)), rng) for i in range(41)]
    assert any(len(e) % 4 for _, e in out) and sum(len(e) for _, e in out) % 4
    return out


SETS = {"families": families, "hard": hard_shapes, "many": many_small}


@pytest.fixture(scope="module")
def host_truth():
    truth = {}
    for name, make in SETS.items():
        gs = GraphSet.from_edge_lists(make())
        truth[name] = (gs, {f: edge_orbit_counts(gs, backend="host", induced=f) for f in FORMS})
    return truth


@pytest.mark.parametrize("induced", FORMS)
@pytest.mark.parametrize("name", list(SETS))
def test_device_equals_host(host_truth, name, induced):
    gs, host = host_truth[name]
    dev = edge_orbit_counts_device(gs, induced=induced)
    assert dev.dtype == torch.int64 and dev.is_cuda and dev.shape == (edge_orbit_rows(gs).shape[0], 69)
    assert host[induced].sum() > 0
    assert torch.equal(dev.cpu().double(), host[induced]), (dev.cpu().double() - host[induced]).abs().max()
    again = edge_orbit_counts_device(gs, induced=induced)
    assert torch.equal(again, dev)                                           # two calls, bit-identical


def test_device_equals_the_yardstick():
    graphs = families()[:11]
    gs = GraphSet.from_edge_lists(graphs)
    for induced in FORMS:
        want = R.edge_orbit_counts_reference(graphs, CENSUS, induced=induced)
        assert want.sum() > 0
        assert (edge_orbit_counts_device(gs, induced=induced).cpu().numpy() == want).all()


@pytest.mark.parametrize("induced", FORMS)
def test_prefixes_and_single_classes(host_truth, induced):
    gs, host = host_truth["hard"]
    h = host[induced]
    three = [CENSUS[i] for i in range(0, 3)]                                 # kmax = 3: the enumeration stops early
    assert torch.equal(edge_orbit_counts_device(gs, three, induced=induced).cpu().double(), h[:, :3])
    four = [CENSUS[i] for i in range(0, 9)]                                  # kmax = 4
    width4 = sum(1 for qi, _, _ in COLS if qi < 9)
    assert width4 == 13
    assert torch.equal(edge_orbit_counts_device(gs, four, induced=induced).cpu().double(), h[:, :13])
    for qi in (9, 20, 29):                                                   # a single 5-node class alone
        pick = [j for j, c in enumerate(COLS) if c[0] == qi]
        got = edge_orbit_counts_device(gs, [CENSUS[qi]], induced=induced).cpu().double()
        assert torch.equal(got, h[:, pick]), qi
    mix = (20, 0, 5, 29, 12)                                                 # reordered; most masks stay at -1
    pick = [j for qi in mix for j, c in enumerate(COLS) if c[0] == qi]
    got = edge_orbit_counts_device(gs, [CENSUS[i] for i in mix], induced=induced).cpu().double()
    assert torch.equal(got, h[:, pick])
    # isomorphic and repeated queries: the tailed triangle with its tail at position 3, at position 0, and again
    dup = [(4, [(0, 1), (1, 2), (0, 2), (2, 3)]), (4, [(3, 1), (1, 2), (3, 2), (1, 0)]),
           (4, [(0, 1), (1, 2), (0, 2), (2, 3)])]
    got = edge_orbit_counts_device(gs, dup, induced=induced).cpu().double()
    assert torch.equal(got, edge_orbit_counts(gs, dup, backend="host", induced=induced)) and got.shape[1] == 9
    assert torch.equal(got[:, :3], got[:, 6:])


def test_empty_inputs_and_auto_backend(host_truth, monkeypatch):
    gs, host = host_truth["families"]
    empty = GraphSet.from_edge_lists([])
    out = edge_orbit_counts_device(empty)
    assert out.shape == (0, 69) and out.dtype == torch.int64 and out.is_cuda
    edgeless = GraphSet.from_edge_lists([(4, []), (1, [])])
    out = edge_orbit_counts_device(edgeless, induced=False)
    assert out.shape == (0, 69) and out.is_cuda
    assert edge_orbit_counts_device(gs, []).shape == (edge_orbit_rows(gs).shape[0], 0)
    assert edge_orbit_counts(empty).shape == (0, 69)
    import desco_amd.groundtruth as GT
    calls = []
    real = GT.edge_orbit_counts_device
    monkeypatch.setattr(GT, "edge_orbit_counts_device", lambda *a, **k: calls.append(1) or real(*a, **k))
    monkeypatch.setattr(GT, "_edge_orbit_host_raw", lambda *a, **k: pytest.fail("auto went to the host"))
    got = edge_orbit_counts(gs)
    assert calls == [1] and got.dtype == torch.double and not got.is_cuda and torch.equal(got, host[True])
    per_query = torch.zeros((got.shape[0], 30), dtype=torch.double).index_add_(
        1, torch.tensor([c[0] for c in COLS]), host[False])
    assert torch.equal(edge_orbit_counts(gs, backend="device", induced=False, per_query=True), per_query)


def test_entry_point_refuses_bad_arguments():
    """Refused by name before any launch: the pointers are device memory the call never gets to touch"""
    from desco_amd import _lib
    L = _lib.lib()
    one = torch.zeros(8, dtype=torch.int64, device="cuda")
    p = one.data_ptr()

    def call(table=p, kmax=5, columns=69, entry_row=p, rows=1, entries=2, col=p):
        return L.desco_edge_orbit_counts_dev(p, 1, 4, p, entries, col, p, p, p, 1, entry_row, rows, table, kmax, columns,
                                             p, None)

    for bad in (dict(columns=70), dict(table=None), dict(kmax=6), dict(kmax=1), dict(entry_row=None), dict(col=None),
                dict(rows=3), dict(entries=2 ** 31)):
        assert call(**bad) == -1 and b"desco_edge_orbit_counts_dev" in L.desco_last_error(), bad
        assert L.desco_gemm_f32_multi(5, None, None) == -1                   # (another message in between)
    assert call(rows=0) == 0 and call(columns=0) == 0 and call(entries=0, rows=0) == 0        # nothing to do
    torch.cuda.synchronize()
    assert (one == 0).all()
