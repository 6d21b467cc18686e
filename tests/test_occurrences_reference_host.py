"""The yardstick checks itself: networkx VF2 grouped by occurrence equals the brute force over node subsets, on the
small golden graphs, for every small query and both modes (no project code is under test here)."""
import pytest

import occurrence_cases as C
import occurrence_reference as R

QUERIES = {"edge": C.EDGE, "p3": C.P3, "triangle": C.TRIANGLE, "c4": C.C4, "tailed": C.TAILED, "diamond": C.DIAMOND,
           "star5": C.STAR5, "house": C.HOUSE}


@pytest.mark.parametrize("induced", [True, False])
@pytest.mark.parametrize("name", list(QUERIES))
def test_vf2_groups_equal_brute_force(name, induced):
    graphs, query = C.small_set(), QUERIES[name]
    vf2 = R.vf2_groups(graphs, query, induced)
    assert vf2 == R.brute_force_groups(graphs, query, induced)
    for v, keys in vf2.items():                                  # keyed by the largest node
        for key in keys:
            assert (max(key) if induced else max(max(e) for e in key)) == v


def test_the_set_exercises_the_difference_between_the_modes():
    graphs = C.small_set()
    total = lambda q, induced: sum(len(s) for s in R.vf2_groups(graphs, q, induced).values())    # noqa: E731
    assert total(C.P3, False) > total(C.P3, True) > 0            # P3 inside triangles: copies that are not induced
    assert total(C.C4, False) > total(C.C4, True) > 0
    assert total(C.DIAMOND, True) > 0 and total(C.TAILED, True) > 0


def test_row_key():
    assert R.row_key([5, 2, 9], C.P3, True) == (2, 5, 9)
    assert R.row_key([5, 2, 9], C.P3, False) == ((2, 5), (2, 9))
    assert R.row_key([9, 2, 5], C.P3, False) == R.row_key([5, 2, 9], C.P3, False)      # the same copy, reversed
    assert R.row_key([2, 5, 9], C.P3, False) != R.row_key([5, 2, 9], C.P3, False)      # another copy on the same nodes
