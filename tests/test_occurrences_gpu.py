"""Listing occurrences on the MI355X (csrc/occurrences_dev.hip through desco_amd.occurrences): bit identity with the
host twin on the cases of occurrence_cases.py, under slicing and chunking, and the no-stray-store condition of the raw
entry point -- tested with sentinel rows inside and behind the buffer, never by provoking a fault."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import occurrence_cases as C  # noqa: E402
from desco_amd import _lib, occurrences, synthetic  # noqa: E402
from desco_amd import groundtruth as gt  # noqa: E402
from desco_amd.groundtruth import (canonical_counts, iter_occurrences, list_occurrences,  # noqa: E402
                                   list_occurrences_device, match_plan)


@functools.lru_cache(maxsize=None)
def host(name, induced):
    return list_occurrences(C.CASES[name][0](), C.CASES[name][1], induced=induced, backend="host")


def same(got, want):
    return np.array_equal(got.rows, want.rows) and np.array_equal(got.ptr, want.ptr) and got.rows.dtype == np.int32


@pytest.mark.parametrize("name,induced", C.CASE_MODES)
def test_device_equals_host_bit_for_bit(name, induced):
    dev = list_occurrences_device(C.CASES[name][0](), C.CASES[name][1], induced=induced)
    assert dev.rows.is_cuda and dev.rows.dtype == torch.int32 and dev.ptr.is_cuda and dev.ptr.dtype == torch.int64
    assert same(dev.cpu(), host(name, induced))


@pytest.mark.parametrize("name,induced", [("p3", True), ("p3", False), ("diamond", True), ("k6-c4", False),
                                          ("three-c4", True), ("p16", True)])
def test_one_entry_per_slice_does_not_change_the_result(name, induced):
    """slice_entries = 1: every slice boundary but the rows' own falls inside a node's row, so the cursors must survive
    between launches."""
    dev = list_occurrences_device(C.CASES[name][0](), C.CASES[name][1], induced=induced, slice_entries=1)
    assert same(dev.cpu(), host(name, induced))


@pytest.mark.parametrize("name,induced", [("three-tailed", False), ("star5-in-k1,70", True), ("k6-p3", False),
                                          ("edge", True)])
def test_device_chunks_concatenate_to_the_listing(name, induced):
    want = host(name, induced)
    bound = max(int(np.diff(want.ptr).max()), 1)
    chunks = list(iter_occurrences(C.CASES[name][0](), C.CASES[name][1], induced=induced, backend="device",
                                   max_rows=bound, slice_entries=37))
    assert occurrences.last_backend == "device"
    assert len(chunks) > 1 and all(len(c) <= bound for c in chunks)
    assert np.array_equal(np.concatenate([c.rows for c in chunks]), want.rows)
    assert np.array_equal(np.concatenate([c.ptr[:-1] for c in chunks] + [chunks[-1].ptr[-1:]]), want.ptr)


def test_backends_auto_and_device_equal_the_host():
    for name, induced in (("three-c4", True), ("k6-c4", False)):
        graphs, query = C.CASES[name][0](), C.CASES[name][1]
        assert same(list_occurrences(graphs, query, induced=induced, backend="auto"), host(name, induced))
        assert occurrences.last_backend == occurrences._AUTO_BACKEND
        assert same(list_occurrences(graphs, query, induced=induced, backend="device"), host(name, induced))
        assert occurrences.last_backend == "device"
    with pytest.raises(ValueError, match=r"occurrences exceed max_rows = 10"):
        list_occurrences_device(C.k6_set(), C.P3, induced=False, max_rows=10)


SENTINEL = -7


def raw_emit(graphs, query, induced, seg, capacity, guard_rows=16):
    """desco_list_occurrences_dev over all entries in one slice with ptr = the scan of ``seg``, into a buffer of
    ``capacity`` rows followed by ``guard_rows`` more, all SENTINEL beforehand.  Returns (rows with the guard, cursor,
    overflow, ptr) on the host."""
    dev = torch.device("cuda")
    d = gt._DeviceGraphs(graphs, dev)
    plan = match_plan([query])
    plan_d = d.put(plan, np.int32)
    ptr = np.concatenate([[0], np.cumsum(seg)]).astype(np.int64)
    ptr_d = d.put(ptr, np.int64)
    rows = torch.full((capacity + guard_rows, query[0]), SENTINEL, dtype=torch.int32, device=dev)
    cursor = torch.full((d.N,), 99, dtype=torch.int32, device=dev)          # (the first slice zeroes them)
    overflow = torch.full((1,), 99, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev)
    _lib.check(_lib.lib().desco_list_occurrences_dev(
        *d.head, plan.ctypes.data, plan_d.data_ptr(), len(plan), 1, int(induced), 0, d.E, ptr_d.data_ptr(), 0,
        cursor.data_ptr(), capacity, rows.data_ptr(), overflow.data_ptr(), stream.cuda_stream),
        "desco_list_occurrences_dev")
    stream.synchronize()
    return rows.cpu().numpy(), cursor.cpu().numpy(), int(overflow.item()), ptr


@pytest.mark.parametrize("name,induced", [("three-triangle", True), ("three-c4", False)])
def test_a_short_ptr_sets_overflow_and_stores_nothing_outside_the_segments(name, induced):
    graphs, query = C.CASES[name][0](), C.CASES[name][1]
    want = host(name, induced)
    counts = np.diff(want.ptr)
    listed = [set(map(tuple, want.rows[want.ptr[v]:want.ptr[v + 1]].tolist())) for v in range(graphs.num_nodes)]
    assert (counts > 1).any() and (counts == 0).any()
    short = np.maximum(counts - 1, 0)

    def check(seg, capacity):
        rows, cursor, overflow, ptr = raw_emit(graphs, query, induced, seg, capacity)
        assert overflow == 1
        assert np.array_equal(cursor, counts)                    # every map asked for a slot, stored or not
        assert (rows[capacity:] == SENTINEL).all()               # the guard band behind rows_capacity
        for v in range(graphs.num_nodes):                        # a segment holds rows of its own anchor only
            lo, hi = int(ptr[v]), min(int(ptr[v + 1]), capacity)
            if counts[v] == 0:
                assert (rows[lo:hi] == SENTINEL).all()           # a guard row right behind a shortened segment
            elif lo < hi:
                mine = set(map(tuple, rows[lo:hi].tolist()))
                assert len(mine) == hi - lo and mine <= listed[v]
        return rows

    # every count minus one, clipped at 0
    check(short, int(short.sum()))
    # the same with one guard row in place of every empty segment: inside rows_capacity, so that only the slot check
    # protects it; guards follow shortened segments directly
    gapped = np.where(counts == 0, 1, short)
    assert ((counts[:-1] > 0) & (counts[1:] == 0)).any()
    check(gapped, int(gapped.sum()))
    # the right ptr into a buffer that ends inside the listing: only the row check protects the rest
    half = int(counts.sum()) // 2
    rows, cursor, overflow, _ = raw_emit(graphs, query, induced, counts, half)
    assert overflow == 1 and np.array_equal(cursor, counts) and (rows[half:] == SENTINEL).all()
    assert (rows[:int(want.ptr[np.searchsorted(want.ptr, half, side="right") - 1])] != SENTINEL).all()
    # and with the right ptr and room for everything nothing is flagged
    rows, cursor, overflow, _ = raw_emit(graphs, query, induced, counts, int(counts.sum()))
    assert overflow == 0 and np.array_equal(cursor, counts) and (rows[int(counts.sum()):] == SENTINEL).all()
    got = occurrences.sort_segments_device(torch.from_numpy(rows[:int(counts.sum())]).cuda()).cpu().numpy()
    assert np.array_equal(got, want.rows)


@functools.lru_cache(maxsize=None)
def benchmark_slice(which):
    if which == "syn":                                           # whole graphs of the Syn_1827 shape, about 200 nodes
        full = synthetic.syn_1827_shaped(40)
        g1 = int(np.searchsorted(full.graph_ptr, 200, side="left"))
        return full.subset(0, max(g1, 1))
    return synthetic.cox2_shaped(24)


@pytest.mark.parametrize("which", ["syn", "cox2"])
@pytest.mark.parametrize("qname", ["triangle", "c4", "house"])
@pytest.mark.parametrize("induced", [True, False])
def test_benchmark_shaped_slices(which, qname, induced):
    graphs = benchmark_slice(which)
    query = {"triangle": C.TRIANGLE, "c4": C.C4, "house": C.HOUSE}[qname]
    want = list_occurrences(graphs, query, induced=induced, backend="host")
    dev = list_occurrences_device(graphs, query, induced=induced).cpu()
    assert same(dev, want)
    esu = canonical_counts(graphs, [query], backend="host", induced=induced)[:, 0].long().numpy()
    assert np.array_equal(np.diff(dev.ptr), esu) and dev.ptr[0] == 0
