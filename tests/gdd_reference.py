"""A plain-Python restatement of the graphlet degree distribution definitions (include/desco_hip.h, "GRAPHLET DEGREE
DISTRIBUTION"): what tests/test_gdd_host.py and tests/test_gdd_gpu.py hold the C routines to.  Every double operation
is numpy's / Python's correctly rounded one; the fma is exact rational arithmetic rounded once."""
import math
from fractions import Fraction

import numpy as np


def fma(a: float, b: float, c: float) -> float:
    """a * b + c with one rounding: exact rational arithmetic, then the correctly rounded conversion."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def distribution(column: np.ndarray):
    """(keys int64 [r], N float64 [r]) of one column of one segment."""
    column = np.asarray(column, dtype=np.int64)
    keys, mult = np.unique(column[column >= 1], return_counts=True)
    shares = [float(int(d)) / float(int(k)) for d, k in zip(mult, keys)]     # int -> float rounds to nearest
    T = 0.0
    for s in shares:
        T = T + s
    return keys.astype(np.int64), np.array([s / T for s in shares], dtype=np.float64)


def segment_lists(X: np.ndarray):
    return [distribution(X[:, c]) for c in range(X.shape[1])]


def column_agreement(x, y) -> float:
    """A_c of two (keys, N) lists: the fma chain over the union of the keys, ascending."""
    nx = {int(k): float(v) for k, v in zip(*x)}
    ny = {int(k): float(v) for k, v in zip(*y)}
    acc = 0.0
    for k in sorted(set(nx) | set(ny)):
        t = nx.get(k, 0.0) - ny.get(k, 0.0)
        acc = fma(t, t, acc)
    D = math.sqrt(0.5 * acc)
    return 0.0 if D > 1.0 else 1.0 - D


def pair(xl, yl):
    """(agree, [A_c]) of two segments given as lists of (keys, N) per column."""
    per = [column_agreement(x, y) for x, y in zip(xl, yl)]
    total = 0.0
    for a in per:
        total = total + a
    return total / float(len(per)), per


def geometric(per) -> float:
    if any(a == 0.0 for a in per):
        return 0.0
    return math.exp(math.fsum(math.log(a) for a in per) / len(per))


def random_table(rng, n: int, C: int, kind: str = "mixed") -> np.ndarray:
    """An int64 [n, C] table shaped like orbit counts: all-zero, constant, heavily tied, all-distinct and huge columns."""
    X = np.zeros((n, C), dtype=np.int64)
    for c in range(C):
        k = c % 6 if kind == "mixed" else {"zeros": 0, "constant": 1, "ties": 2, "distinct": 3, "huge": 5}[kind]
        if k == 0:
            X[:, c] = 0                                        # nobody touches the orbit: an empty list
        elif k == 1:
            X[:, c] = 7                                        # one entry
        elif k == 2:
            X[:, c] = rng.integers(0, 4, n)                    # heavy ties, zeros among them
        elif k == 3:
            X[:, c] = rng.permutation(n) * 3 + 1               # all distinct
        elif k == 4:
            X[:, c] = rng.integers(0, max(n // 2, 2), n) ** 2
        else:                                                  # above 2^53 (odd: the conversion rounds) and near 2^62
            X[:, c] = np.where(rng.integers(0, 2, n) == 0, (1 << 53) + 1 + 2 * rng.integers(0, 3, n),
                               (1 << 62) - 1 - rng.integers(0, 3, n))
    return X
