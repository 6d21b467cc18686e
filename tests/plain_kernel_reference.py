"""Host reference of the fused plain-layer kernel (header of csrc/plain_layer.hip; the docstring of ops.plain_layer),
written from the documented contract alone: numpy + torch on the CPU, no call into ``desco_amd.ops``.

    z[r] = sum over row r of the plain CSR of x[col[e], :]  (CSR order)  + s x[r]          (s = 0 when there is none)
    h    = z W1 + b1;       num_mats == 2:  h = relu(h) W2 + b2;       out[r] = relu(h)

A *case* is a dict: x [N, Wp], rowptr [N + 1] / col (int64), W1, W2 (K-major [Wp, Wp]; W2 None for num_mats 1), b1, b2,
s (None, 0.0 or 0.25) -- and what the GPU test launches on it: row0, num_rows (rows outside the range are sources only),
out_mode ("out", "out2", "both"), out2_row0, x_strided, H (true width of a zero-padded case, or None), bare (rows with
z == 0: relu(b1) exactly for one product), dead (rows whose relu(h) is all zero: relu(b2) exactly for two products).
``evaluate`` returns all N rows in the dtype asked for: float64 is the reference, float32 the *fp32 evaluation* the
kernel is held to (neighbours added one after the other in CSR order, s x rounded on its own, one matmul per product).
``mag`` is the scale an output's rounding errors live on: |z| |W1| + |b1| on absolute values, pushed WITHOUT the relu
through |W2|, |b2| for two products."""
import numpy as np
import torch

import wide_reference as W
from wide_reference import scaled_error  # noqa: F401

WIDTHS, MATS = (64, 128, 192, 256), (1, 2)
RANGES = W.RANGES
TAIL = W.TAIL


def evaluate(case, dtype=torch.float64, absolute=False):
    conv = (lambda t: t.to(dtype).abs()) if absolute else (lambda t: t.to(dtype))    # noqa: E731
    x = conv(case["x"])
    z = W.gather((case["x"], case["rowptr"], case["col"]), dtype, absolute)
    if case["s"] is not None:
        s = torch.tensor(abs(case["s"]) if absolute else case["s"], dtype=torch.float32).to(dtype)
        z = z + s * x
    h = z @ conv(case["W1"]) + conv(case["b1"])
    if case["W2"] is not None:
        h = (h if absolute else torch.relu(h)) @ conv(case["W2"]) + conv(case["b2"])
    return h if absolute else torch.relu(h)


def mag(case):
    return evaluate(case, torch.float64, absolute=True)


def layer_case(wp, mats, s=None, row0=37, num_rows=203, regime="o1", H=None, edges=True, out_mode="both",
               out2_row0=None, x_strided=True, seed=0):
    """One case.  Rows [row0, row0 + num_rows) are computed; rows before and the TAIL rows behind are sources only; every
    row has edges (also those outside the range), sources drawn from all N rows.  Degrees: wide_reference.degree_mix
    (every degree 0..9 forced once, hubs of 301, 203 and 77 sources, a third of the rows empty).  ``regime``: o1, range,
    big, small, zero as in wide_reference.layer_case; ``dead``: b1 strongly negative, three rows of the range without
    sources and with tiny x, so that relu(h) is all zero there."""
    rng = np.random.default_rng(5000 + seed)
    g = torch.Generator().manual_seed(6000 + seed)
    N = row0 + num_rows + TAIL
    x = torch.randn(N, wp, generator=g)
    W1 = torch.randn(wp, wp, generator=g) / np.sqrt(wp)
    b1 = torch.randn(wp, generator=g) / 4
    W2 = torch.randn(wp, wp, generator=g) / np.sqrt(wp) if mats == 2 else None
    b2 = torch.randn(wp, generator=g) / 4 if mats == 2 else None
    deg = W.degree_mix(N, np.arange(row0, row0 + num_rows), rng) if edges else np.zeros(N, np.int64)
    bare, dead = [], []
    if regime == "zero":
        zero = rng.random(N) < 0.3
        bare = [int(r) for r in row0 + rng.permutation(num_rows)[:3]]
        zero[bare] = True
        x[torch.from_numpy(zero)] = 0
        deg[bare] = 0
    elif regime == "dead":
        dead = [int(r) for r in row0 + rng.permutation(num_rows)[:3]]
        deg[dead] = 0
        x[dead] = x[dead] * 1e-3
        b1 = -0.5 - b1.abs()
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = rng.integers(0, N, int(rowptr[-1])).astype(np.int64)
    if regime == "range":
        x = x * 2.0 ** torch.randint(-16, 17, (N, 1), generator=g).float()
    elif regime in ("big", "small"):
        f = 1e5 if regime == "big" else 1e-4
        x, W1, b1 = x * f, W1 * f, b1 * (f * f)
        if mats == 2:
            W2, b2 = W2 * f, b2 * (f * f * f)
    else:
        assert regime in ("o1", "zero", "dead")
    if H is not None:
        x[:, H:] = 0
        for m, b in ((W1, b1), (W2, b2)):
            if m is not None:
                m[H:, :] = 0
                m[:, H:] = 0
                b[H:] = 0
    return dict(x=x, rowptr=torch.from_numpy(rowptr), col=torch.from_numpy(col), W1=W1, b1=b1, W2=W2, b2=b2, s=s,
                mats=mats, row0=row0, num_rows=num_rows, regime=regime, H=H, bare=bare, dead=dead, out_mode=out_mode,
                out2_row0=row0 if out2_row0 is None else out2_row0, x_strided=x_strided)


CASES = {}


def _add(name, **kw):
    assert name not in CASES
    CASES[name] = dict(kw, seed=len(CASES))


for _wp in WIDTHS:                               # every instantiation: rows (37, 203), four tiles with a clamped last one
    for _m in MATS:
        _add(f"instantiation Wp {_wp} mats {_m}", wp=_wp, mats=_m, s=0.25 if _m == 2 else None)
for _r0, _n in RANGES:
    _add(f"range ({_r0}, {_n}) Wp 128 mats 2", wp=128, mats=2, s=0.25, row0=_r0, num_rows=_n)
    _add(f"range ({_r0}, {_n}) Wp 192 mats 1", wp=192, mats=1, row0=_r0, num_rows=_n)
for _m in MATS:                                  # self_scale NULL, 0 and 0.25
    for _s in (None, 0.0, 0.25):
        _add(f"arguments self_scale {_s} Wp 64 mats {_m}", wp=64, mats=_m, s=_s, row0=5, num_rows=65)
for _mode in ("out", "out2", "both"):            # out2 starts behind row0: the rows before it go to out only
    _add(f"outputs {_mode}, out2_row0 40, x strided", wp=128, mats=2, row0=5, num_rows=65, out_mode=_mode, out2_row0=40)
_add("outputs both, out2_row0 = row0, x contiguous", wp=256, mats=1, s=0.25, row0=5, num_rows=65, x_strided=False)
_add("degrees empty col Wp 64 mats 2", wp=64, mats=2, s=0.25, edges=False)
_add("degrees empty col Wp 256 mats 1", wp=256, mats=1, edges=False, row0=5, num_rows=65)
for _reg in ("range", "big", "small", "zero", "dead"):
    _add(f"regime {_reg} Wp 128 mats 2", wp=128, mats=2, s=0.25, regime=_reg)
    _add(f"regime {_reg} Wp 256 mats 1", wp=256, mats=1, regime=_reg)
_add("regime dead Wp 64 mats 2 no self", wp=64, mats=2, regime="dead")
_add("padding H 100 in Wp 128 mats 2", wp=128, mats=2, s=0.25, H=100)
_add("padding H 32 in Wp 64 mats 1", wp=64, mats=1, H=32)
_add("padding H 100 in Wp 128 mats 2, zero rows", wp=128, mats=2, H=100, regime="zero")


def make(name):
    return layer_case(**CASES[name])
