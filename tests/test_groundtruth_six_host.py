"""The class table of the 6-node device enumerator (desco_canonical_class_table6, csrc/groundtruth.cpp) and the
argument checks of desco_canonical_counts6_dev that return before any GPU call.  CPU only."""
import ctypes

import networkx as nx
import numpy as np
import pytest

from desco_amd import _lib
from desco_amd.groundtruth import _flatten_queries, census_classes

OFF = [0, 0, 0, 2, 10, 74, 1098, 33866]
ALL = [q for k in (2, 3, 4, 5, 6) for q in census_classes(k)]          # 1 + 2 + 6 + 21 + 112 = 142


def table6(queries, expect=0):
    _, qn, qp, qe = _flatten_queries(queries)
    table = np.full(33866, 77, dtype=np.int16)
    kmax = ctypes.c_int(-1)
    rc = _lib.lib().desco_canonical_class_table6(qn.ctypes.data, qp.ctypes.data, qe.ctypes.data if len(qe) else None,
                                                 len(qn), table.ctypes.data, ctypes.byref(kmax))
    assert rc == expect, _lib.lib().desco_last_error()
    return table, kmax.value


def graph_of_mask(k, mask):
    g = nx.Graph()
    g.add_nodes_from(range(k))
    g.add_edges_from((a, b) for b in range(1, k) for a in range(b) if mask >> (b * (b - 1) // 2 + a) & 1)
    return g


def graph_of_query(q):
    g = nx.Graph()
    g.add_nodes_from(range(q[0]))
    g.add_edges_from(q[1])
    return g


@pytest.fixture(scope="module")
def full():
    return table6(ALL)


def test_block_sizes_are_the_numbers_of_connected_labelled_graphs(full):
    table, kmax = full
    assert len(ALL) == 142 and kmax == 6
    assert [int((table[OFF[k]:OFF[k + 1]] >= 0).sum()) for k in (2, 3, 4, 5, 6)] == [1, 4, 38, 728, 26704]
    assert table.min() == -1 and table.max() == 141
    for k in (2, 3, 4, 5, 6):                           # an entry of the k-block names a k-node query
        block = table[OFF[k]:OFF[k + 1]]
        assert all(ALL[q][0] == k for q in np.unique(block[block >= 0]))


def test_entries_name_an_isomorphic_query_and_disconnected_masks_are_minus_one(full):
    table, _ = full
    rng = np.random.default_rng(6)
    sample6 = set(rng.choice(1 << 15, size=2500, replace=False).tolist()) | {0, (1 << 15) - 1}
    checked = 0
    for k in (2, 3, 4, 5, 6):
        masks = range(1 << (k * (k - 1) // 2)) if k < 6 else sorted(sample6)
        for m in masks:
            g, q = graph_of_mask(k, m), int(table[OFF[k] + m])
            if not nx.is_connected(g):
                assert q == -1, (k, m)
            else:
                assert q >= 0 and nx.is_isomorphic(g, graph_of_query(ALL[q])), (k, m, q)
                checked += k == 6
    assert checked >= 2000
    # every disconnected 6-node mask, without networkx: reachability from position 0 over the pair bits
    m = np.arange(1 << 15)
    reach = np.ones(1 << 15, dtype=np.int64)
    for _ in range(6):
        for b in range(1, 6):
            for a in range(b):
                hit = ((m >> (b * (b - 1) // 2 + a)) & 1).astype(bool) & (((reach >> a) | (reach >> b)) & 1).astype(bool)
                reach[hit] |= (1 << a) | (1 << b)
    connected = reach == 63
    assert int(connected.sum()) == 26704
    assert ((table[OFF[6]:] >= 0) == connected).all()


def test_small_blocks_equal_the_five_node_table(full):
    table, _ = full
    small = ALL[:30]
    _, qn, qp, qe = _flatten_queries(small)
    five = np.empty(1098, dtype=np.int16)
    kmax = ctypes.c_int(0)
    assert _lib.lib().desco_canonical_class_table(qn.ctypes.data, qp.ctypes.data, qe.ctypes.data, 30,
                                                  five.ctypes.data, ctypes.byref(kmax)) == 0
    assert kmax.value == 5 and (table[:1098] == five).all()
    only_small, k5 = table6(small)
    assert k5 == 5 and (only_small[:1098] == five).all() and (only_small[1098:] == -1).all()


def test_a_subset_of_the_queries_renumbers_and_blanks_the_rest(full):
    table, _ = full
    keep = [0, 2, 9, 29, 30, 77, 141, 100]                 # (not in ascending order: the index is the position)
    sub, kmax = table6([ALL[i] for i in keep])
    want = np.full(33866, -1, dtype=np.int16)
    for new, old in enumerate(keep):
        want[table == old] = new
    assert kmax == 6 and (sub == want).all()
    sub4, kmax4 = table6([ALL[5], ALL[1]])
    assert kmax4 == 4 and (sub4[OFF[5]:] == -1).all()
    none, kmax0 = table6([])
    assert kmax0 == 0 and (none == -1).all()


def test_table_refusals_name_the_reason():
    L = _lib.lib()
    path6, star6 = (6, [(i, i + 1) for i in range(5)]), (6, [(0, i) for i in range(1, 6)])

    def refused(queries, word):
        assert L.desco_gemm_f32_multi(5, None, None) == -1                   # (another entry point's message in between)
        table6(queries, expect=-1)
        msg = L.desco_last_error()
        assert b"desco_canonical_class_table6" in msg and word in msg, msg

    refused([(1, [])], b"2..6 nodes")
    refused([path6, (7, [(i, i + 1) for i in range(6)])], b"2..6 nodes")
    refused([path6, star6, (6, [(5, 4), (4, 3), (3, 0), (0, 1), (1, 2)])], b"isomorphic")
    refused([(6, [(0, 1), (2, 2)])], b"bad query edge")
    refused([(6, [(0, 6)])], b"bad query edge")
    refused([(6, [(-1, 2)])], b"bad query edge")
    refused(ALL + [path6], b"142")
    _, qn, qp, qe = _flatten_queries([path6])
    table = np.zeros(33866, dtype=np.int16)
    kmax = ctypes.c_int(0)
    good = [qn.ctypes.data, qp.ctypes.data, qe.ctypes.data, 1, table.ctypes.data, ctypes.byref(kmax)]
    assert L.desco_canonical_class_table6(*good) == 0
    for null in (0, 1, 4, 5):
        args = list(good)
        args[null] = None
        assert L.desco_gemm_f32_multi(5, None, None) == -1
        assert L.desco_canonical_class_table6(*args) == -1
        assert b"desco_canonical_class_table6" in L.desco_last_error()
    args = list(good)
    args[3] = -1
    assert L.desco_canonical_class_table6(*args) == -1


def test_device_entry_refuses_bad_arguments_before_any_gpu_call():
    L = _lib.lib()
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data                              # host memory: a refused call never touches it

    def dev(graph_ptr=p, graphs=1, nodes=4, rowptr=p, entries=8, col=p, node_graph=p, bit_off=p, bits=p, words=1,
            cls=p, kmax=6, queries=142, e0=0, e1=8, out=p):
        return L.desco_canonical_counts6_dev(graph_ptr, graphs, nodes, rowptr, entries, col, node_graph, bit_off, bits,
                                             words, cls, kmax, queries, e0, e1, out, None)

    for bad in (dict(graph_ptr=None), dict(rowptr=None), dict(col=None), dict(node_graph=None), dict(bit_off=None),
                dict(bits=None), dict(cls=None), dict(out=None), dict(kmax=1), dict(kmax=7), dict(queries=143),
                dict(queries=-1), dict(e0=5, e1=4), dict(e1=9), dict(e0=-1), dict(graphs=-1), dict(nodes=-1),
                dict(entries=-1, e1=0), dict(words=-1)):
        assert L.desco_gemm_f32_multi(5, None, None) == -1                   # (another entry point's message in between)
        assert dev(**bad) == -1 and b"desco_canonical_counts6_dev" in L.desco_last_error(), bad
    assert dev(queries=0) == 0 and dev(nodes=0) == 0                         # nothing to do
    assert (buf == 0).all()
