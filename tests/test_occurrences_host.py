"""The host occurrence lister (desco_list_occurrences through desco_amd.occurrences) against the yardstick of
occurrence_reference.py, on the cases of occurrence_cases.py: every property of the definition, both modes."""
import functools

import networkx as nx
import numpy as np
import pytest

import occurrence_cases as C
from desco_amd import _lib, groundtruth, occurrences
from desco_amd.graphs import GraphSet
from desco_amd.groundtruth import iter_occurrences, list_occurrences, match_plan


@functools.lru_cache(maxsize=None)
def listing(name, induced):
    return list_occurrences(C.CASES[name][0](), C.CASES[name][1], induced=induced, backend="host", num_threads=4)


@pytest.mark.parametrize("name,induced", C.CASE_MODES)
def test_listing_meets_the_definition(name, induced):
    occ = listing(name, induced)
    assert occurrences.last_backend == "host" and occ.k == C.CASES[name][1][0] and len(occ) == len(occ.rows)
    C.check_listing(name, induced, occ)


@pytest.mark.parametrize("name,induced", C.CASE_MODES)
def test_thread_count_does_not_change_the_bits(name, induced):
    one = list_occurrences(C.CASES[name][0](), C.CASES[name][1], induced=induced, backend="host", num_threads=1)
    four = listing(name, induced)
    assert np.array_equal(one.rows, four.rows) and np.array_equal(one.ptr, four.ptr)


@pytest.mark.parametrize("name,induced", C.CASE_MODES)
def test_chunks_concatenate_to_the_listing(name, induced):
    whole = listing(name, induced)
    counts = np.diff(whole.ptr)
    # the smallest bound that still takes the largest anchor: cuts between anchors wherever two do not fit together
    bound = max(int(counts.max()), 1)
    chunks = list(iter_occurrences(C.CASES[name][0](), C.CASES[name][1], induced=induced, backend="host",
                                   max_rows=bound))
    assert all(len(c) <= bound for c in chunks)
    assert [c.v0 for c in chunks[1:]] == [c.v1 for c in chunks[:-1]] and chunks[0].v0 == 0
    assert chunks[-1].v1 == len(counts)
    if len(whole) > bound:
        assert len(chunks) > 1
    assert np.array_equal(np.concatenate([c.rows for c in chunks]), whole.rows)
    assert np.array_equal(np.concatenate([c.ptr[:-1] for c in chunks] + [chunks[-1].ptr[-1:]]), whole.ptr)
    for c in chunks:
        assert len(c.rows) == c.ptr[-1] - c.ptr[0]


def test_max_rows_refusals_name_the_total_and_the_node():
    graphs = C.k6_set()
    whole = listing("k6-p3", False)                            # 60 copies of P3 in K6, 30 of them at node 5
    assert len(whole) == 60
    with pytest.raises(ValueError, match=r"60 occurrences.*max_rows = 59.*iter_occurrences"):
        list_occurrences(graphs, C.P3, induced=False, backend="host", max_rows=59)
    assert len(list_occurrences(graphs, C.P3, induced=False, backend="host", max_rows=60)) == 60
    with pytest.raises(ValueError, match=r"node 5 alone anchors 30 occurrences.*max_rows = 29"):
        list(iter_occurrences(graphs, C.P3, induced=False, backend="host", max_rows=29))


def test_accessors():
    graphs = C.three_set()
    occ = listing("three-triangle", True)
    assert occ.query == C.TRIANGLE and occ.induced is True
    assert np.array_equal(occ.graph, graphs.node_graph_ids()[occ.rows[:, 2]])
    assert set(occ.graph.tolist()) == {0, 2, 4}                 # the edgeless graph and the tree hold no triangle
    sub = occ.subsets()
    assert (np.diff(sub, axis=1) > 0).all() and np.array_equal(sub[:, -1], occ.rows.max(axis=1))
    t = occ.table()
    assert list(t) == ["graph", "v0", "v1", "v2"]
    assert np.array_equal(t["v1"] + graphs.graph_ptr[:-1][t["graph"]], occ.rows[:, 1])
    # a networkx query numbers its nodes in iteration order
    g = nx.Graph([("a", "b"), ("b", "c"), ("a", "c")])
    assert np.array_equal(list_occurrences(graphs, g, backend="host").rows, occ.rows)
    assert groundtruth.Occurrences is occurrences.Occurrences


def test_vf2_backend_returns_the_same_bits():
    for name, induced in (("tailed", True), ("k6-c4", False), ("p3", False)):
        got = list_occurrences(C.CASES[name][0](), C.CASES[name][1], induced=induced, backend="vf2")
        assert occurrences.last_backend == "vf2"
        want = listing(name, induced)
        assert np.array_equal(got.rows, want.rows) and np.array_equal(got.ptr, want.ptr)


def test_empty_inputs():
    none = GraphSet.from_edge_lists([])
    occ = list_occurrences(none, C.TRIANGLE, backend="host")
    assert occ.rows.shape == (0, 3) and occ.ptr.tolist() == [0] and list(iter_occurrences(none, C.TRIANGLE)) == []
    edgeless = GraphSet.from_edge_lists([(4, [])])
    occ = list_occurrences(edgeless, C.EDGE, backend="host")
    assert occ.rows.shape == (0, 2) and occ.ptr.tolist() == [0] * 5 and occ.graph.shape == (0,)


def test_queries_outside_the_limits_are_refused():
    graphs = C.k6_set()
    with pytest.raises(RuntimeError, match="2..16 nodes"):
        list_occurrences(graphs, (17, [(i, i + 1) for i in range(16)]), backend="host")
    with pytest.raises(RuntimeError, match="connected"):
        list_occurrences(graphs, (4, [(0, 1), (2, 3)]), backend="host")
    with pytest.raises(ValueError, match="unknown backend"):
        list_occurrences(graphs, C.P3, backend="cuda")


def raw_host(graphs, plan, ptr, rows, induced=1, v0=0, v1=None, capacity=None, null=None, **over):
    a = dict(graph_ptr=graphs.graph_ptr.ctypes.data, rowptr=graphs.rowptr.ctypes.data, col=graphs.col.ctypes.data,
             plan=plan.ctypes.data, ptr=ptr.ctypes.data, rows=rows.ctypes.data, num_graphs=graphs.num_graphs,
             plan_entries=len(plan))
    a.update(over)
    if null:
        a[null] = None
    return _lib.lib().desco_list_occurrences(
        a["graph_ptr"], a["num_graphs"], a["rowptr"], a["col"], a["plan"], a["plan_entries"], induced, 2, v0,
        graphs.num_nodes if v1 is None else v1, a["ptr"], len(rows) if capacity is None else capacity, a["rows"])


def test_raw_entry_point_refuses_by_name():
    L = _lib.lib()
    graphs = C.k6_set()
    whole = listing("k6-triangle", True)
    plan = match_plan([C.TRIANGLE])
    ptr = whole.ptr.copy()
    rows = np.full((len(whole) + 4, 3), -7, dtype=np.int32)

    def refused(rc, what):
        assert rc == -1
        msg = L.desco_last_error().decode()
        assert "desco_list_occurrences" in msg and what in msg, msg

    assert raw_host(graphs, plan, ptr, rows) == 0
    assert np.array_equal(rows[:len(whole)], whole.rows) and (rows[len(whole):] == -7).all()
    refused(raw_host(graphs, match_plan([C.TRIANGLE, C.P3]), ptr, rows), "plan[0] must be 1")
    refused(raw_host(graphs, plan, ptr, rows, plan_entries=len(plan) - 1), "not a plan")
    swapped = plan.copy()
    swapped[2 + 4 + 1] = swapped[2 + 4 + 2]                     # two positions on one query node
    refused(raw_host(graphs, swapped, ptr, rows), "permute")
    for null in ("graph_ptr", "rowptr", "ptr", "rows", "plan"):
        refused(raw_host(graphs, plan, ptr, rows, null=null), "null pointer" if null != "plan" else "plan")
    refused(raw_host(graphs, plan, ptr, rows, num_graphs=-1), "negative size")
    refused(raw_host(graphs, plan, ptr, rows, capacity=-1), "negative size")
    refused(raw_host(graphs, plan, ptr, rows, induced=2), "induced must be 0 or 1")
    refused(raw_host(graphs, plan, ptr, rows, v0=-1), "node range")
    refused(raw_host(graphs, plan, ptr, rows, v1=7), "node range")
    refused(raw_host(graphs, plan, ptr, rows, v0=4, v1=3), "node range")
    refused(raw_host(graphs, plan, ptr, rows, capacity=len(whole) - 1), "rows_capacity")
    down = ptr.copy()
    down[3] = down[4] + 1
    refused(raw_host(graphs, plan, down, rows), "descend")
    # a ptr that is not the scan of the counts: named, and nothing is stored outside a segment
    short = np.concatenate([[0], np.cumsum(np.maximum(np.diff(ptr) - 1, 0))]).astype(np.int64)
    rows[:] = -7
    refused(raw_host(graphs, plan, short, rows), "first at node 2")
    assert (rows[int(short[-1]):] == -7).all()
