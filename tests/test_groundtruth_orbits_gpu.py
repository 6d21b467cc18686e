"""Exact per-node orbit counts on the device (csrc/groundtruth_dev.hip, go_count_kernel) against the host enumerator and
the brute-force yardstick tests/orbit_reference.py -- integers, bit for bit."""
import math
import os
import subprocess
import sys

import networkx as nx
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import orbit_reference as R  # noqa: E402
from desco_amd.graphs import GraphSet  # noqa: E402
from desco_amd.groundtruth import (census_classes, orbit_columns, orbit_counts,  # noqa: E402
                                   orbit_counts_device)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENSUS = [q for k in (2, 3, 4, 5) for q in census_classes(k)]
COLS = orbit_columns()
LEAVES = 130


def edges_of(g):
    return (g.number_of_nodes(), [tuple(e) for e in g.edges()])


def shapes():
    """The shapes where the kernel can go wrong, in one set."""
    rng = np.random.default_rng(11)
    star = (LEAVES + 1, [(LEAVES, i) for i in range(LEAVES)])        # hub = the largest id: its items hold every subset;
    # 130 third-node candidates (lanes wrap), 131 nodes (3-word bitset rows)
    tree = [(int(rng.integers(0, v)), v) for v in range(1, 200)]     # 200 nodes (4 words): a random tree plus chords
    chords = {(int(min(a, b)), int(max(a, b))) for a, b in rng.integers(0, 200, size=(120, 2)) if a != b}
    big = (200, sorted(set(tree) | chords))
    small = edges_of(nx.gnp_random_graph(9, 0.5, seed=3))
    lonely = (12, [(0, 5), (5, 7), (7, 0), (7, 9), (2, 9)])          # isolated nodes 1, 3, 4, 6, 8, 10, 11
    hub_first = (71, [(0, i) for i in range(1, 71)])                 # hub = the smallest id: candidates from u0's row
    return [star, edges_of(nx.complete_graph(20)), big, small, small, lonely, hub_first, (5, [])]


@pytest.fixture(scope="module")
def shape_set():
    gs = GraphSet.from_edge_lists(shapes())
    return gs, {f: orbit_counts(gs, backend="host", induced=f) for f in (True, False)}


@pytest.mark.parametrize("induced", [True, False])
def test_device_equals_host_on_the_hard_shapes(shape_set, induced):
    gs, host = shape_set
    dev = orbit_counts_device(gs, induced=induced)
    assert dev.dtype == torch.int64 and dev.is_cuda and dev.shape == (gs.num_nodes, 73)
    dev = dev.cpu()
    assert torch.equal(dev.double(), host[induced]), (dev.double() - host[induced]).abs().max()
    # closed forms of the star: the hub is node 130 of graph 0, the leaves the rows before it
    s5 = nx.star_graph(4)
    centre, leaf = R.column_of(CENSUS, s5, 0), R.column_of(CENSUS, s5, 1)
    assert dev[LEAVES, centre] == math.comb(130, 4) == 11_358_880
    assert (dev[:LEAVES, leaf] == math.comb(129, 3)).all() and math.comb(129, 3) == 349_504
    k20 = dev[LEAVES + 1:LEAVES + 21]
    k5 = R.column_of(CENSUS, nx.complete_graph(5), 0)
    if induced:
        assert (k20[:, k5] == math.comb(19, 4)).all()
    n9 = LEAVES + 1 + 20 + 200
    assert torch.equal(dev[n9:n9 + 9], dev[n9 + 9:n9 + 18]) and dev[n9:n9 + 9].sum() > 0     # the graph given twice
    assert (dev[-5:] == 0).all()                                                            # the edgeless graph
    again = orbit_counts_device(gs, induced=induced).cpu()
    assert torch.equal(again, dev)                                                          # two calls, bit-identical


def test_device_equals_the_yardstick():
    rng = np.random.default_rng(2)
    graphs = [edges_of(nx.gnp_random_graph(int(rng.integers(5, 13)), float(rng.uniform(0.2, 0.6)), seed=40 + i))
              for i in range(8)]
    gs = GraphSet.from_edge_lists(graphs)
    for induced in (True, False):
        want = R.orbit_counts_reference(graphs, CENSUS, induced=induced)
        assert want.sum() > 0
        assert (orbit_counts_device(gs, induced=induced).cpu().numpy() == want).all()


@pytest.mark.parametrize("induced", [True, False])
def test_subsets_of_the_classes(shape_set, induced):
    gs, host = shape_set
    three = list(census_classes(3))                                          # kmax = 3: the enumeration stops early
    got = orbit_counts_device(gs, three, induced=induced).cpu().double()
    assert torch.equal(got, host[induced][:, 1:4])
    mix = [CENSUS[i] for i in (20, 0, 5, 29, 12)]                            # most masks stay at -1
    pick = [j for qi in (20, 0, 5, 29, 12) for j, c in enumerate(COLS) if c[0] == qi]
    got = orbit_counts_device(gs, mix, induced=induced).cpu().double()
    assert torch.equal(got, host[induced][:, pick])
    # isomorphic and repeated queries: P3 with the centre at position 1, at position 0 (centre column first), at 1 again
    dup = [(3, [(0, 1), (1, 2)]), (3, [(0, 1), (0, 2)]), (3, [(0, 1), (1, 2)])]
    got = orbit_counts_device(gs, dup, induced=induced).cpu().double()
    assert torch.equal(got, orbit_counts(gs, dup, backend="host", induced=induced)) and got.shape[1] == 6
    assert torch.equal(got[:, 0], got[:, 3]) and torch.equal(got[:, 0], got[:, 4])           # ends
    assert torch.equal(got[:, 1], got[:, 2]) and torch.equal(got[:, 1], got[:, 5])           # centre
    assert not torch.equal(got[:, 0], got[:, 1])


def test_empty_inputs_and_auto_backend(shape_set, monkeypatch):
    gs, host = shape_set
    empty = GraphSet.from_edge_lists([])
    out = orbit_counts_device(empty)
    assert out.shape == (0, 73) and out.dtype == torch.int64 and out.is_cuda
    assert orbit_counts_device(gs, []).shape == (gs.num_nodes, 0)
    assert orbit_counts(empty).shape == (0, 73)
    import desco_amd.groundtruth as GT
    calls = []
    real = GT.orbit_counts_device
    monkeypatch.setattr(GT, "orbit_counts_device", lambda *a, **k: calls.append(1) or real(*a, **k))
    monkeypatch.setattr(GT, "_orbit_host_raw", lambda *a, **k: pytest.fail("auto went to the host"))
    got = orbit_counts(gs)
    assert calls == [1] and got.dtype == torch.double and not got.is_cuda and torch.equal(got, host[True])
    per_query = torch.zeros((gs.num_nodes, 30), dtype=torch.double).index_add_(
        1, torch.tensor([c[0] for c in COLS]), host[False])
    assert torch.equal(orbit_counts(gs, backend="device", induced=False, per_query=True), per_query)


def test_entry_point_refuses_bad_arguments():
    from desco_amd import _lib
    L = _lib.lib()
    one = torch.zeros(8, dtype=torch.int64, device="cuda")
    p = one.data_ptr()
    assert L.desco_orbit_counts_dev(p, 1, 4, p, 0, None, p, p, p, 1, p, 5, 74, p, None) == -1      # 74 columns
    assert b"desco_orbit_counts_dev" in L.desco_last_error()
    assert L.desco_orbit_counts_dev(p, 1, 4, p, 0, None, p, p, p, 1, None, 5, 73, p, None) == -1    # no table
    assert L.desco_orbit_counts_dev(p, 1, 4, p, 0, None, p, p, p, 1, p, 6, 73, p, None) == -1       # kmax = 6
    assert L.desco_orbit_counts_dev(p, 1, 0, p, 0, None, p, p, p, 1, p, 5, 73, p, None) == 0        # nothing to do


def test_driver_writes_the_orbit_truth(tmp_path):
    """``main.py --orbit_truth`` in a fresh process on the MUTAG-shaped synthetic split: the CSV holds the 73 columns
    under their (query, orbit) header, and its column sums are |orbit| times those of the run's canonical truth."""
    import pandas as pd
    from desco_amd.data import gen_query_ids, load_data
    from desco_amd.workload import Workload
    out, data = tmp_path / "out", tmp_path / "data"
    cmd = [sys.executable, os.path.join(ROOT, "main.py"), "--data_root", str(data), "--gpu", "0",
           "--train_dataset", "MUTAG_train", "--valid_dataset", "MUTAG_val", "--test_dataset", "MUTAG_test",
           "--neigh_epoch_num", "1", "--neigh_batch_size", "64", "--neigh_model_path", str(tmp_path / "ckpt_n"),
           "--gossip_model_path", str(tmp_path / "ckpt_g"), "--train_neigh", "--output_dir", str(out), "--orbit_truth"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    gdv = pd.read_csv(out / "orbit_node_MUTAG_test.csv", index_col=0)
    assert list(gdv.columns) == [f"({q},{o})" for q, o, _ in COLS] and len(gdv.columns) == 73
    test_set = load_data("MUTAG_test", root_folder=str(data))
    assert gdv.shape[0] == test_set.num_nodes
    w = Workload(test_set, os.path.join(str(data), "MUTAG_test"))
    ids = gen_query_ids(query_size=[3, 4, 5])
    assert w.exist_groundtruth(query_ids=ids) and w.exist_orbit_groundtruth()
    canon = w.load_groundtruth(query_ids=ids).sum(0)                         # the 29 classes of 3..5 nodes
    sums = gdv.to_numpy().sum(0)
    assert sums[0] == test_set.num_directed_edges
    for j, (qi, _, mem) in enumerate(COLS):
        if qi:
            assert sums[j] == len(mem) * float(canon[qi - 1]), (j, qi)
    assert sums[1:].sum() > 0
