"""Host side of gnn_model.THIRD_LAYER_TABLE: NeighborhoodBatch.layer3_table_index on CPU tensors against a brute-force dict
over the tuples that define the classes -- a canonical row of X_2 by (canon_id, ordered first-layer table ids of its segment),
a count row of X_3 by (its X_2 class, per CSR entry in order the source's X_2 class: count class in slots 0 and 1, canonical
class in the table slots).

The partitions are degree-sorted, as InferencePipeline's are.  The small blocks lower the profit bounds (LAYER3_MIN_ROWS,
LAYER*_MIN_ROWS_PER_CLASS) on their own batch object to have the classes built; the defaults are tested as refusals."""
import numpy as np
import pytest

from desco_amd import synthetic
from desco_amd.batch import NeighborhoodBatch
from desco_amd.graphs import GraphSet
from desco_amd.partition import build_partition

S = 4


def _batch(graphs, min_rows=1, per_class=1, per_class2=1):
    gs = graphs if isinstance(graphs, GraphSet) else GraphSet.from_edge_lists(graphs)
    b = NeighborhoodBatch(build_partition(gs, 4).degree_sorted(), "cpu")
    if min_rows is not None:
        b.LAYER3_MIN_ROWS = min_rows
    if per_class is not None:
        b.LAYER3_MIN_ROWS_PER_CLASS = per_class
    if per_class2 is not None:
        b.LAYER2_MIN_ROWS_PER_CLASS = per_class2
    return b


def _brute_force(b):
    """(canonical keys, canonical classes, count keys, count classes): dict key -> rows in row order; the class ids inside
    the count keys are the brute force's own (numbered by first appearance), not the index's"""
    nc, n = b.num_count, b.num_rows
    vr = np.asarray(b.part.vrowptr, dtype=np.int64)
    vcol = np.asarray(b.part.vcol, dtype=np.int64)
    _, canon_id, vcol_tc = (t.numpy().astype(np.int64) for t in b.canonical_table_index())
    cls2 = b.layer2_table_index()[0].numpy().astype(np.int64)
    ckeys, cclasses = [], {}
    for j in range(n - nc):
        i = nc + j
        k = (int(canon_id[j]), tuple(vcol_tc[vr[S * i]:vr[S * i + S]].tolist()))
        ckeys.append(k)
        cclasses.setdefault(k, []).append(j)
    cnum = {k: c for c, k in enumerate(cclasses)}
    cc = np.array([cnum[k] for k in ckeys], dtype=np.int64)
    keys, classes = [], {}
    for i in range(nc):
        lo, mid, hi = vr[S * i], vr[S * i + 2], vr[S * i + S]
        k = (int(cls2[i]), tuple(cls2[vcol[lo:mid]].tolist()), tuple(cc[vcol[mid:hi] - nc].tolist()))
        keys.append(k)
        classes.setdefault(k, []).append(i)
    return ckeys, cclasses, keys, classes


def _check_index(b):
    idx = b.layer3_table_index()
    assert idx is not None and b.layer3_table_index() is idx             # built once, cached
    assert all(t.element_size() == 4 and not t.dtype.is_floating_point for t in idx[:6])
    cls3, rep_uptr, rep_vcol, rep_self, vcol_3, ccls2, crep = (t.numpy().astype(np.int64) for t in idx)
    nc, n = b.num_count, b.num_rows
    cls2 = b.layer2_table_index()[0].numpy().astype(np.int64)
    u2 = int(cls2.max()) + 1
    ckeys, cclasses, keys, classes = _brute_force(b)
    uc2, u3 = len(cclasses), len(classes)
    # canonical classes: one id per distinct key, ids 0 .. U_c2 - 1, crep the lowest canonical row of its class
    assert ccls2.shape == (n - nc,) and sorted(set(ccls2.tolist())) == list(range(uc2)) and crep.shape == (uc2,)
    assert len({(ckeys[j], int(ccls2[j])) for j in range(n - nc)}) == uc2
    for k, rows in cclasses.items():
        assert crep[ccls2[rows[0]]] == rows[0] == min(rows)
    # count classes likewise
    assert cls3.shape == (nc,) and sorted(set(cls3.tolist())) == list(range(u3))
    assert len({(keys[i], int(cls3[i])) for i in range(nc)}) == u3
    # the compact CSR: class c's row is its LOWEST row's degrees and segment, sources remapped; its own row in table2
    vr = np.asarray(b.part.vrowptr, dtype=np.int64)
    vcol = np.asarray(b.part.vcol, dtype=np.int64)
    assert rep_uptr.shape == (u3 * S + 1,) and rep_uptr[0] == 0 and rep_vcol.shape == (rep_uptr[-1],)
    assert rep_self.shape == (u3,)
    for k, rows in classes.items():
        r, c = rows[0], int(cls3[rows[0]])
        assert r == min(rows) and rep_self[c] == cls2[r] == k[0]
        assert np.array_equal(np.diff(rep_uptr[S * c:S * c + S + 1]), np.diff(vr[S * r:S * r + S + 1]))
        lo, mid, hi = vr[S * r], vr[S * r + 2], vr[S * r + S]
        want = cls2[vcol[lo:mid]].tolist() + ccls2[vcol[mid:hi] - nc].tolist()
        assert rep_vcol[rep_uptr[S * c]:rep_uptr[S * c + S]].tolist() == want
    # only valid table rows are addressed: table2 in slots 0 and 1, the [U_c2, 64] table product in the table slots
    rlow = np.repeat(np.arange(u3 * S) % S, np.diff(rep_uptr)) < 2
    assert rep_vcol.min() >= 0 and (rep_vcol[rlow] < u2).all() and (rep_vcol[~rlow] < uc2).all()
    assert rep_self.min() >= 0 and rep_self.max() < u2
    # vcol_3: the sources of slots 0 and 1 (count rows) by their class, canonical rows' segments too; slots 2, 3 untouched
    low = np.repeat(np.arange(n * S) % S, np.diff(vr)) < 2
    assert vcol_3.shape == vcol.shape and low[vr[S * nc]:].any()
    assert np.array_equal(vcol_3[low], cls3[vcol[low]]) and np.array_equal(vcol_3[~low], vcol[~low])
    assert vcol_3[low].min() >= 0 and vcol_3[low].max() < u3
    # the canonical rows of X_3 (not indexed: their launch stays; the figure pins the two class arrays together)
    uc3 = len({(int(ccls2[j]), tuple(cls2[vcol[vr[S * (nc + j)]:vr[S * (nc + j) + 2]]].tolist())) for j in range(n - nc)})
    return u3, uc3, uc2, u2


def test_layer3_classes_of_mutag24_match_a_brute_force_dict():
    b = _batch(synthetic.mutag_shaped(24))
    assert b.num_count == 2795
    assert _check_index(b) == (1427, 89, 20, 309)


def test_layer3_classes_of_cox2_at_the_default_class_bounds():
    """the real, un-replicated COX2 size: 10.6 rows per class pass the default bounds; only the row bound is lowered"""
    b = _batch(synthetic.cox2_shaped(), min_rows=1, per_class=None, per_class2=None)
    assert b.num_count == 130022 and b.LAYER3_MIN_ROWS_PER_CLASS == 8 and b.LAYER3_MAX_CLASSES == 1 << 14
    assert _check_index(b) == (12316, 460, 29, 531)


def test_replication_adds_no_class():
    one = _batch(synthetic.mutag_shaped(24))
    b = _batch(synthetic.mutag_shaped(24).replicate(4), per_class=2, per_class2=None)
    assert b.layer3_table_index()[3].numel() == one.layer3_table_index()[3].numel() == 1427
    _check_index(b)


@pytest.mark.parametrize("name", ["rows", "rows_per_class", "mutag", "max_classes", "dense", "both_table_slots"])
def test_layer3_index_refusals(name):
    if name == "rows":                                   # below LAYER3_MIN_ROWS: refused before any work
        b = _batch(synthetic.mutag_shaped(24).replicate(8), min_rows=None, per_class=1)
        assert b.LAYER3_MIN_ROWS >= 1 << 19 > b.num_count
        assert b.layer3_table_index() is None and "_layer2_table" not in b.__dict__
    elif name == "rows_per_class":                       # LAYER3_MIN_ROWS_PER_CLASS U_3 > N_c
        b = _batch(synthetic.mutag_shaped(24), per_class=None)
        assert b.layer2_table_index() is not None and 8 * 1427 > b.num_count and b.layer3_table_index() is None
    elif name == "mutag":                                # the natural case: MUTAG-shaped x1 has 3.5 rows per X_3 class
        b = _batch(synthetic.mutag_shaped(), per_class=None, per_class2=None)
        assert b.num_count == 22386 and b.layer2_table_index() is not None and b.layer3_table_index() is None
        b = _batch(synthetic.mutag_shaped())
        assert _check_index(b)[:3] == (6452, 296, 27)
    elif name == "max_classes":
        b = _batch(synthetic.mutag_shaped(24))
        b.LAYER3_MAX_CLASSES = 1426
        assert b.layer3_table_index() is None
        b = _batch(synthetic.mutag_shaped(24))
        b.LAYER3_MAX_CLASSES = 1427
        assert b.layer3_table_index() is not None
    elif name == "dense":                                # degree above 8
        b = _batch(synthetic.syn_1827_shaped(8))
        assert b.layer2_table_index() is None and b.layer3_table_index() is None
    else:                                                # a triangle: entries in both table slots
        ring, path = (6, [(i, (i + 1) % 6) for i in range(6)]), (6, [(i, i + 1) for i in range(5)])
        b = _batch([ring, path, (3, [(0, 1), (1, 2), (0, 2)])] * 20)
        assert b.table_empty == 0 and b.layer3_table_index() is None
