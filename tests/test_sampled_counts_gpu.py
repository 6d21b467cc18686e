"""Sampled counts on the MI355X (csrc/sampled_counts_dev.hip) against the host twin (csrc/sampled_counts.cpp) and the
exact census kernel: bit for bit, integers only."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import golden_graphs  # noqa: E402

from desco_amd import groundtruth as gt  # noqa: E402
from desco_amd import sampling, synthetic  # noqa: E402
from desco_amd.graphs import GraphSet  # noqa: E402

pytestmark = pytest.mark.gpu

SCHEDULES = {"uniform 0.5": dict(fraction=0.5), "uniform 0.05": dict(fraction=0.05),
             "(0.7, 1, 0.3, 1)": dict(probs=(0.7, 1.0, 0.3, 1.0))}


def _classes(kmax):
    return [(n, list(e)) for k in range(2, kmax + 1) for n, e in gt.census_classes(k)]


def _inputs():
    graphs = list(golden_graphs())
    graphs.append((12, [(a, b) for b in range(12) for a in range(b)]))                       # K12
    graphs.append((41, [(40, i) for i in range(40)]))                    # a 40-leaf star: C(40, 4) 5-subsets at one root
    # a node of degree 150 joined to a 150-path: more than 64 third-node candidates, lanes take several
    graphs.append((151, [(150, i) for i in range(150)] + [(i, i + 1) for i in range(149)]))
    syn = synthetic.syn_1827_shaped(60).edge_lists()
    graphs += sorted((g for g in syn if g[0] <= 160), key=lambda g: (g[0], len(g[1])))[-4:]
    graphs += synthetic.cox2_shaped(8).edge_lists()
    graphs += [(1, []), (5, [])]                                          # a single node, an edgeless graph
    return GraphSet.from_edge_lists(graphs)


@pytest.fixture(scope="module")
def graphs():
    return _inputs()


@pytest.mark.parametrize("kmax", [3, 4, 5])
@pytest.mark.parametrize("name", list(SCHEDULES))
def test_device_equals_twin(graphs, kmax, name):
    kw = {k: (v[:kmax - 1] if k == "probs" else v) for k, v in SCHEDULES[name].items()}
    args = dict(replicas=3, seed=11, level="node", **kw)
    host = sampling.sampled_tallies(graphs, _classes(kmax), backend="host", **args)
    dev = sampling.sampled_tallies(graphs, _classes(kmax), backend="device", **args)
    assert sampling.last_backend == "device"
    assert host.shape == dev.shape == (3, graphs.num_nodes, len(_classes(kmax)))
    print(f"[sampled] kmax {kmax} {name}: {int(host.sum())} kept subsets")
    assert host.sum() > 0
    assert torch.equal(host, dev)


def test_all_ones_is_the_exact_census(graphs):
    exact = gt.canonical_counts_device(graphs, _classes(5)).cpu()
    got = sampling.sampled_tallies_device(graphs, None, probs=(1, 1, 1, 1), replicas=2, level="node").cpu()
    assert torch.equal(got[0], exact) and torch.equal(got[1], exact)


def test_repeats_slices_and_chunks(graphs):
    small = graphs.subset(0, 12)
    args = dict(fraction=0.3, seed=3)
    whole = sampling.sampled_tallies_device(small, None, replicas=7, level="node", **args)
    for _ in range(4):                                                     # 5 launches in all: the same bits
        assert torch.equal(sampling.sampled_tallies_device(small, None, replicas=7, level="node", **args), whole)
    n0, n1 = int(small.graph_ptr[4]), int(small.graph_ptr[9])
    part = sampling.sampled_tallies_device(small.subset(4, 9), None, replicas=7, level="node", graph_base=4, **args)
    assert torch.equal(part, whole[:, n0:n1])
    part = sampling.sampled_tallies_device(small, None, replicas=3, level="node", replica_base=2, **args)
    assert torch.equal(part, whole[2:5])
    # 3 chunks (3 + 3 + 1 replicas) = one chunk, at both levels; level="graph" = the row sums of level="node"
    per_replica = 8 * small.num_graphs * 30
    assert torch.equal(sampling.sampled_tallies_device(small, None, replicas=7, level="node",
                                                       max_bytes=3 * 8 * small.num_nodes * 30, **args), whole)
    one = sampling.sampled_tallies_device(small, None, replicas=7, **args)
    three = sampling.sampled_tallies_device(small, None, replicas=7, max_bytes=3 * per_replica, **args)
    sums = torch.stack([whole[:, int(a):int(b)].sum(dim=1) for a, b in zip(small.graph_ptr[:-1], small.graph_ptr[1:])],
                       dim=1)
    assert one.shape == (7, 12, 30)
    assert torch.equal(one, three) and torch.equal(one, sums)
    assert torch.equal(sampling.sampled_tallies(small, None, replicas=7, backend="device", max_bytes=3 * per_replica,
                                                **args), one.cpu())


def test_routing(graphs, monkeypatch):
    small = graphs.subset(0, 6)
    monkeypatch.setattr(sampling, "AUTO_USES_DEVICE", True)
    ref = sampling.sampled_tallies(small, None, fraction=0.4, replicas=2, backend="host")
    words = gt._bitset_words(small)
    monkeypatch.setattr(gt, "_DEVICE_BITSET_LIMIT_WORDS", int(words.max()) - 1)             # the largest graph is over it
    got = sampling.sampled_tallies(small, None, fraction=0.4, replicas=2, backend="auto")
    assert sampling.last_backend == "device+host"
    assert torch.equal(got, ref)
    with pytest.raises(RuntimeError, match="2..5 nodes"):
        sampling.sampled_tallies(small, [gt.census_classes(6)[0]], fraction=0.4, backend="device")
