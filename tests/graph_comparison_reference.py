"""A numpy / scipy restatement of the graphlet correlation definitions (include/desco_hip.h, "GRAPHLET CORRELATION"):
what tests/test_graph_comparison_host.py and tests/test_graph_comparison_gpu.py hold the C routines to."""
from fractions import Fraction

import numpy as np
import scipy.stats


def with_dummy(X: np.ndarray, dummy_row: bool) -> np.ndarray:
    X = np.asarray(X, dtype=np.int64)
    return np.vstack([X, np.ones((1, X.shape[1]), dtype=np.int64)]) if dummy_row else X


def doubled_ranks(X: np.ndarray) -> np.ndarray:
    """int64 [n', C]: 2 * (average rank) - (n' + 1) of every column.  Average ranks are multiples of 1/2, so this is exact."""
    n = X.shape[0]
    if n == 0:
        return np.zeros(X.shape, dtype=np.int64)
    twice = 2.0 * scipy.stats.rankdata(X, axis=0)
    assert (twice == np.rint(twice)).all()
    return twice.astype(np.int64) - (n + 1)


def matrix(D: np.ndarray) -> np.ndarray:
    return D.T @ D


def rho_from_matrix(S: np.ndarray) -> np.ndarray:
    """The definition's three rounded operations in numpy's float64."""
    diag = np.diag(S).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = S.astype(np.float64) / np.sqrt(diag[:, None] * diag[None, :])
    rho[(diag == 0)[:, None] | (diag == 0)[None, :]] = 0.0
    np.fill_diagonal(rho, 1.0)
    return rho


def segment(X: np.ndarray, dummy_row: bool):
    """(D, S, rho) of one segment."""
    D = doubled_ranks(with_dummy(X, dummy_row))
    S = matrix(D)
    return D, S, rho_from_matrix(S)


def spearman(X: np.ndarray, dummy_row: bool) -> np.ndarray:
    """scipy's Spearman matrix of the columns, NaN beside a constant column (scipy is asked for the varying ones only:
    one constant column makes it return a single NaN)."""
    X = with_dummy(X, dummy_row)
    C = X.shape[1]
    varies = np.flatnonzero((X != X[:1]).any(axis=0))
    out = np.full((C, C), np.nan)
    if len(varies) >= 2:
        r = scipy.stats.spearmanr(X[:, varies]).correlation
        out[np.ix_(varies, varies)] = np.full((2, 2), r) if np.ndim(r) == 0 else r
        if np.ndim(r) == 0:
            out[varies, varies] = 1.0
    return out


def upper(rho: np.ndarray) -> np.ndarray:
    iu = np.triu_indices(rho.shape[-1], 1)
    return np.ascontiguousarray(rho[..., iu[0], iu[1]])


def fma(a: float, b: float, c: float) -> float:
    """a * b + c with one rounding: exact rational arithmetic, then the correctly rounded conversion."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def gcd_chain(x: np.ndarray, y: np.ndarray) -> float:
    acc = 0.0
    for p in range(len(x)):
        t = float(x[p]) - float(y[p])
        acc = fma(t, t, acc)
    return float(np.sqrt(np.float64(acc)))


def gcd_matrix(x: np.ndarray, y: np.ndarray) -> np.ndarray:
    return np.array([[gcd_chain(a, b) for b in y] for a in x], dtype=np.float64).reshape(len(x), len(y))


def random_table(rng, n: int, C: int, kind: str = "mixed") -> np.ndarray:
    """An int64 [n, C] table shaped like orbit counts: many ties, some constant and some all-distinct columns."""
    X = np.zeros((n, C), dtype=np.int64)
    for c in range(C):
        k = c % 5 if kind == "mixed" else {"ties": 1, "distinct": 2, "constant": 0}[kind]
        if k == 0:
            X[:, c] = 0 if c % 2 == 0 else 7                  # constant (zeros: not constant with the dummy row)
        elif k == 1:
            X[:, c] = rng.integers(0, 3, n)                   # heavy ties
        elif k == 2:
            X[:, c] = rng.permutation(n) * 3 + 2              # all distinct
        elif k == 3:
            X[:, c] = rng.integers(0, max(n // 2, 2), n) ** 2
        else:
            X[:, c] = rng.integers(0, 1 << 40, n)             # large values
    return X
