"""The shared device ESU walk (csrc/groundtruth_esu_dev.hpp) under all three of its visitors -- canonical, labelled and
orbit counts -- over the same inputs, so that a slip in the walk cannot hide behind one kernel's own host twin.  The
host ESU enumerator is the reference; every comparison is of exact integers."""
import networkx as nx
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from desco_amd.graphs import GraphSet  # noqa: E402
from desco_amd.groundtruth import (canonical_counts, canonical_counts_device,  # noqa: E402
                                   canonical_counts_labelled_device, census_classes, orbit_columns,
                                   orbit_counts_device)
from test_groundtruth_orbits_gpu import shapes  # noqa: E402

CENSUS = [(k, list(e)) for n in (2, 3, 4, 5) for k, e in census_classes(n)]       # the 30 classes of 2..5 nodes
# number of leading classes -> the largest subset the walk then builds (kmax)
PREFIXES = {1: 2, 3: 3, 30: 5}


def one_label(query):
    """the query as a networkx graph whose nodes all carry the feature [0.0]"""
    k, edges = query
    g = nx.Graph()
    g.add_nodes_from(range(k), feat=[0.0])
    g.add_edges_from(edges)
    return g


@pytest.fixture(scope="module")
def walk_set():
    graphs = shapes()
    gs = GraphSet.from_edge_lists(graphs, node_feat=np.zeros((sum(n for n, _ in graphs), 1), dtype=np.float32))
    return gs, canonical_counts(gs, CENSUS, backend="host")          # computed once, never written to


@pytest.mark.parametrize("classes", sorted(PREFIXES), ids=[f"kmax{PREFIXES[c]}" for c in sorted(PREFIXES)])
def test_three_visitors_agree_with_the_host(walk_set, classes):
    gs, host = walk_set
    queries = CENSUS[:classes]
    assert max(k for k, _ in queries) == PREFIXES[classes]
    want = host[:, :classes]
    assert want.sum() > 0

    canon = canonical_counts_device(gs, queries)
    assert canon.dtype == torch.int64 and canon.is_cuda and canon.shape == (gs.num_nodes, classes)
    assert torch.equal(canon.cpu().double(), want), (canon.cpu().double() - want).abs().max()

    labelled = canonical_counts_labelled_device(gs, [one_label(q) for q in queries])
    assert labelled.dtype == torch.int64 and torch.equal(labelled, canon)

    orbits = orbit_counts_device(gs, queries).cpu()
    columns = orbit_columns(queries)
    assert orbits.dtype == torch.int64 and orbits.shape == (gs.num_nodes, len(columns))
    canon = canon.cpu()
    for g in range(gs.num_graphs):
        n0, n1 = int(gs.graph_ptr[g]), int(gs.graph_ptr[g + 1])
        per_query = canon[n0:n1].sum(dim=0)
        per_column = orbits[n0:n1].sum(dim=0)
        for j, (qi, _, members) in enumerate(columns):
            assert per_column[j] == len(members) * per_query[qi], (g, j, qi)
