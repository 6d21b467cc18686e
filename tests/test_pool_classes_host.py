"""Host side of gnn_model.POOL_CLASS_TABLE: NeighborhoodBatch.pool_class_index on CPU tensors against a brute-force dict over
the triples that define the classes -- a neighborhood by (its anchor class, count_ptr & 15, the ordered top-level count classes
of its rows).

The partitions are degree-sorted, as InferencePipeline's are.  The small blocks lower the profit bounds on their own batch
object; the defaults are tested as refusals."""
import numpy as np
import pytest

from desco_amd import synthetic
from desco_amd.batch import NeighborhoodBatch
from desco_amd.graphs import GraphSet
from desco_amd.partition import build_partition


def _batch(graphs, min_rows=1, per_class=1, max_level=None, anchor=True):
    gs = graphs if isinstance(graphs, GraphSet) else GraphSet.from_edge_lists(graphs)
    b = NeighborhoodBatch(build_partition(gs, 4).degree_sorted(), "cpu")
    b.LAYER3_MIN_ROWS, b.LAYER3_MIN_ROWS_PER_CLASS, b.LAYER2_MIN_ROWS_PER_CLASS = 1, 1, 1
    b.DEEP_TABLE_MIN_ROWS, b.DEEP_TABLE_MIN_ROWS_PER_CLASS, b.DEEP_TABLE_MAX_CLASSES = 1, 1, 1 << 17
    if anchor:
        b.ANCHOR_CLASS_MIN_ROWS, b.ANCHOR_CLASS_MIN_ROWS_PER_CLASS = 1, 1
    if min_rows is not None:
        b.POOL_CLASS_MIN_ROWS = min_rows
    if per_class is not None:
        b.POOL_CLASS_MIN_ROWS_PER_CLASS = per_class
    if max_level is not None:
        b.DEEP_TABLE_MAX_LEVEL = max_level
    return b


def _brute_force(b, L=8, aligned=True):
    """the neighborhoods' classes by the defining triples, numbered by first appearance"""
    acls = b.anchor_class_index(L)[0].tolist()
    cls = b._table_level(L)[0].tolist()
    cp = np.asarray(b.part.count_ptr, dtype=np.int64).tolist()
    d = {}
    return [d.setdefault((acls[q], cp[q] & 15 if aligned else 0, tuple(cls[cp[q]:cp[q + 1]])), len(d)) for q in range(len(acls))]


def _same_partition(a, b):
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    return a.shape == b.shape and len(set(zip(a.tolist(), b.tolist()))) == len(set(a.tolist())) == len(set(b.tolist()))


def _refines(fine, coarse):
    return len(set(zip(np.asarray(fine).tolist(), np.asarray(coarse).tolist()))) == len(set(np.asarray(fine).tolist()))


def _small_set():
    """the hand-made set of tests/test_anchor_classes_host.py: rings, paths, a star, a branched ring"""
    ring = lambda k: (k, [(i, (i + 1) % k) for i in range(k)])
    path = lambda k: (k, [(i, i + 1) for i in range(k - 1)])
    star = (5, [(0, i) for i in range(1, 5)])
    branched = (9, [(i, (i + 1) % 6) for i in range(6)] + [(0, 6), (6, 7), (3, 8)])
    return [ring(6), path(6), star, branched, ring(5), path(9), ring(8), branched] * 3


SETS = {"mutag24": lambda: synthetic.mutag_shaped(24), "cox2_12": lambda: synthetic.cox2_shaped(12), "small": _small_set}


@pytest.fixture(scope="module")
def built():
    """per set: the batch with its brute-force classes at L = 8 (computed once, left unchanged)"""
    out = {}
    for name, make in SETS.items():
        b = _batch(make())
        out[name] = (b, _brute_force(b))
    return out


@pytest.mark.parametrize("name", list(SETS))
def test_the_classes_are_the_dictionarys_and_the_representatives_their_lowest_members(built, name):
    b, bf = built[name]
    B = b.num_rows - b.num_count
    idx = b.pool_class_index(8)
    assert idx is not None and b.pool_class_index(8) is idx                        # built once, cached
    pcls, prep = idx
    assert pcls.dtype.is_floating_point is False and pcls.element_size() == 4 and prep.element_size() == 8
    pcls, prep = pcls.numpy().astype(np.int64), prep.numpy()
    up = len(set(bf))
    # ids dense, the class count and the classes the brute force's
    assert pcls.shape == (B,) and sorted(set(pcls.tolist())) == list(range(up)) and _same_partition(pcls, bf)
    first = {}
    for q, c in enumerate(pcls.tolist()):
        first.setdefault(c, q)
    assert prep.shape == (up,) and [first[c] for c in range(up)] == prep.tolist()
    # the classes refine the anchor classes; members of one class agree in row count and in their start inside a tile
    assert _refines(pcls, b.anchor_class_index(8)[0].numpy())
    cp = np.asarray(b.part.count_ptr, dtype=np.int64)
    assert _refines(pcls, np.diff(cp)) and _refines(pcls, cp[:-1] & 15)


@pytest.mark.parametrize("name", ["mutag24", "small"])
def test_a_shallower_model_takes_its_last_level(name):
    b = _batch(SETS[name](), max_level=5)
    pcls, prep = b.pool_class_index(5)
    bf = _brute_force(b, 5)
    assert _same_partition(pcls.numpy(), bf) and prep.numel() == len(set(bf))


def test_replication_multiplies_the_classes_by_at_most_the_sixteen_alignments():
    one = _batch(synthetic.mutag_shaped(24))
    three = _batch(synthetic.mutag_shaped(24).replicate(3))
    unaligned = len(set(_brute_force(one, aligned=False)))
    assert len(set(_brute_force(three, aligned=False))) == unaligned
    assert unaligned <= one.pool_class_index(8)[1].numel() <= three.pool_class_index(8)[1].numel() <= 16 * unaligned
    assert _same_partition(three.pool_class_index(8)[0].numpy(), _brute_force(three))


@pytest.mark.parametrize("name", ["no anchor index", "rows", "rows_per_class", "levels", "dense"])
def test_refusals(name):
    g = synthetic.mutag_shaped(24)
    up = _batch(g).pool_class_index(8)[1].numel()
    if name == "no anchor index":                        # the anchor index's own bounds at their defaults
        b = _batch(g, anchor=False)
        assert b.anchor_class_index(8) is None and b.pool_class_index(8) is None
    elif name == "rows":                                 # below POOL_CLASS_MIN_ROWS neighborhoods: refused before any work
        b = _batch(g, min_rows=None)
        B = b.num_rows - b.num_count
        assert b.POOL_CLASS_MIN_ROWS == NeighborhoodBatch.POOL_CLASS_MIN_ROWS >= 1 << 20 > B
        assert b.pool_class_index(8) is None and "_anchor_class" not in b.__dict__
        assert _batch(g, min_rows=B + 1).pool_class_index(8) is None and _batch(g, min_rows=B).pool_class_index(8) is not None
    elif name == "rows_per_class":                       # POOL_CLASS_MIN_ROWS_PER_CLASS U_p > B: the default, the bound, one past
        b = _batch(g, per_class=None)
        B = b.num_rows - b.num_count
        assert b.POOL_CLASS_MIN_ROWS_PER_CLASS == NeighborhoodBatch.POOL_CLASS_MIN_ROWS_PER_CLASS == 8 and 8 * up > B
        assert b.pool_class_index(8) is None
        assert _batch(g, per_class=B // up).pool_class_index(8) is not None
        assert _batch(g, per_class=B // up + 1).pool_class_index(8) is None
    elif name == "levels":                               # L without table levels up to it
        b = _batch(g, max_level=6)
        assert b.pool_class_index(8) is None and b.pool_class_index(5) is None and b.pool_class_index(3) is None
        assert b.pool_class_index(6) is not None
    else:                                                # rows of degree above 8: no table level at all
        assert _batch(synthetic.syn_1827_shaped(8)).pool_class_index(8) is None
