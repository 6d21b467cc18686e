"""Host reference of the kernels of the neighborhood models of other widths than 64 (header of csrc/shmp_wide.hip; the
docstrings of ops.shmp_layer_wide and ops.csr_gather_sum_wide), written from the documented contract alone: numpy + torch
on the CPU, no call into ``desco_amd.ops`` or ``desco_amd.autograd``.  Used by tests/test_wide_kernels_gpu.py (the
kernels and the autograd nodes against it) and by tests/test_wide_reference_host.py (the reference against a dense
incidence-matrix formula, and the gate against the kernel's restated arithmetic and a second fp32 summation order).

    agg_s[i] = sum over virtual row i vslots + s of x[vcol[e], :]        (s < slots <= vslots, CSR order)
    out[i]   = relu([agg_0[i] | .. | agg_{S-1}[i] | x[i]] Wt + bias)     Wt [(S + 1) Wp, Wp], bias [Wp]

A *case* is a dict: x [N, Wp], vrowptr [N vslots + 1] / vcol (int64 tensors), vslots, slots, Wt, bias -- and what the
GPU test launches on it: row0, num_rows (the rows the kernel computes; the others are sources only), out_mode ("out",
"out2", "both"), x_strided, H (the true width of a zero-padded case, or None), bare (rows with x == 0 and no source:
relu(bias) exactly).  ``evaluate`` returns all N rows in the dtype asked for: float64 is the reference, float32 the *fp32
evaluation* the kernel is held to (neighbours added one after the other in CSR order, one matmul over K).  ``mag`` is
the same evaluation on |x|, |Wt|, |bias| without the relu: the sum of |terms| of every output, the scale its rounding
errors live on.  ``gather`` is the aggregation alone; in float32 it adds strictly in CSR order with one rounding per
add, which is the value csr_gather_sum_wide documents.  ``emulate_f16x3`` restates the layer kernel's arithmetic."""
import numpy as np
import torch

from shmp_reference import scaled_error  # noqa: F401  (the figure every wide test reports)

WIDTHS, SLOTS = (64, 128, 192, 256), (2, 4)
RANGES = [(0, 1), (0, 63), (0, 64), (5, 65), (37, 203)]          # (row0, num_rows): tiles of 64 rows, clamped last tiles
HUBS = (301, 203, 77)                                            # hub degrees, none a multiple of 4
TAIL = 6                                                         # source-only rows behind the range


# ---- the formula ----------------------------------------------------------------------------------------------------
def _args(case_or_args):
    if isinstance(case_or_args, dict):
        return case_or_args["x"], case_or_args["vrowptr"], case_or_args["vcol"]
    return case_or_args


def gather(case_or_args, dtype=torch.float64, absolute=False):
    """out[v] = sum over virtual row v of x[vcol[e], :] -> [len(vrowptr) - 1, W].  float32: strictly in CSR order, one
    rounding per add (position p of every virtual row that has one is added in step p)."""
    x, vrowptr, vcol = _args(case_or_args)
    x = x.to(dtype).abs() if absolute else x.to(dtype)
    nv = vrowptr.numel() - 1
    deg = vrowptr[1:] - vrowptr[:-1]
    out = torch.zeros(nv, x.shape[1], dtype=dtype)
    if dtype == torch.float64:
        return out.index_add_(0, torch.repeat_interleave(torch.arange(nv), deg), x[vcol])
    for p in range(int(deg.max()) if nv else 0):
        live = (deg > p).nonzero().flatten()
        out[live] = out[live] + x[vcol[vrowptr[live] + p]]
    return out


def blocks(case, dtype=torch.float64, absolute=False):
    """the S + 1 operand blocks [N, Wp] of every row: agg_0 .. agg_{S-1}, x"""
    x = case["x"].to(dtype).abs() if absolute else case["x"].to(dtype)
    N, wp = x.shape
    agg = gather(case, dtype, absolute).view(N, case["vslots"], wp)
    return [agg[:, s] for s in range(case["slots"])] + [x]


def evaluate(case, dtype=torch.float64, absolute=False, order="whole"):
    """relu([agg_0 | .. | agg_{S-1} | x] Wt + bias) for all N rows.  ``order``: "whole" (one matmul over K) or
    "blocks_reversed" (one matmul per Wp-wide block, accumulated from the last block to the first).  ``absolute``: on
    |x|, |Wt|, |bias| and without the relu."""
    conv = (lambda t: t.to(dtype).abs()) if absolute else (lambda t: t.to(dtype))    # noqa: E731
    bl, Wt, bias = blocks(case, dtype, absolute), conv(case["Wt"]), conv(case["bias"])
    wp = bl[0].shape[1]
    if order == "whole":
        z = torch.cat(bl, 1) @ Wt
    else:
        assert order == "blocks_reversed"
        z = None
        for b in range(len(bl) - 1, -1, -1):
            part = bl[b] @ Wt[b * wp:(b + 1) * wp]
            z = part if z is None else z + part
    z = z + bias
    return z if absolute else torch.relu(z)


def mag(case):
    return evaluate(case, torch.float64, absolute=True)


# ---- the kernel's arithmetic, restated ------------------------------------------------------------------------------
def _pow2_scale(mx):
    """the power of two s with s mx in [2^14, 2^15) for mx > 0 (at most 2^126), 1 for mx == 0; float32 arrays"""
    _, e = np.frexp(mx)                                              # mx = m 2^e, m in [0.5, 1)
    s = np.ldexp(np.float32(1), np.minimum(15 - e, 126)).astype(np.float32)
    return np.where(mx > 0, s, np.float32(1))


def _split(v):
    """v (float32, already scaled) = hi + lo: hi = fp16(v), lo = fp16(v - hi), both returned as float32"""
    hi = v.astype(np.float16).astype(np.float32)
    return hi, (v - hi).astype(np.float16).astype(np.float32)


def emulate_f16x3(case):
    """The layer kernel's documented arithmetic on the host -> [N, Wp] float32: every block gathered in fp32 in CSR
    order; each (row, block) scaled by its own power of two and split into fp16 hi / lo; the weights scaled by one power
    of two per matrix and split; lo hi, hi lo, hi hi accumulated in fp32 per 32-wide K step; the block's scales undone
    into an fp32 accumulator; bias, relu.  (Host arithmetic: the sum inside one 32-wide step is numpy's, not the MFMA's.)"""
    f32 = np.float32
    Wt, bias = case["Wt"].numpy().astype(f32), case["bias"].numpy().astype(f32)
    ws = _pow2_scale(np.abs(Wt).max().astype(f32))
    winv = f32(1) / ws
    wh, wl = _split(Wt * ws)
    bl = [b.numpy() for b in blocks(case, torch.float32)]
    N, wp = bl[0].shape
    acc = np.zeros((N, wp), f32)
    for b, v in enumerate(bl):
        sc = _pow2_scale(np.abs(v).max(1)) if N else np.ones(0, f32)
        ah, al = _split(v * sc[:, None])
        tmp = np.zeros((N, wp), f32)
        for k in range(0, wp, 32):
            bh, bw = wh[b * wp + k:b * wp + k + 32], wl[b * wp + k:b * wp + k + 32]
            tmp = tmp + al[:, k:k + 32] @ bh                          # smallest terms first
            tmp = tmp + ah[:, k:k + 32] @ bw
            tmp = tmp + ah[:, k:k + 32] @ bh
        acc = acc + tmp * ((f32(1) / sc) * winv)[:, None]
    return torch.from_numpy(np.maximum(acc + bias, f32(0)))


# ---- the cases --------------------------------------------------------------------------------------------------------
def degree_mix(nv, used, rng, hubs=HUBS):
    """degrees of ``nv`` virtual rows: about a third empty, the others 1..9; among the ``used`` ones (the virtual rows a
    launch reads) every degree 0..9 is forced once and the hub degrees once each, as far as there is room"""
    deg = np.where(rng.random(nv) < 1 / 3, 0, rng.integers(1, 10, nv))
    pick = rng.permutation(used)
    forced = list(range(10)) if len(pick) >= 20 else []
    hubs = list(hubs)[:max(0, (len(pick) - len(forced)) // 2)] if len(pick) >= 2 else []
    for v, d in zip(pick, forced + hubs):
        deg[v] = d
    return deg


def layer_case(wp, S, vslots=None, row0=37, num_rows=203, regime="o1", H=None, edges=True, out_mode="both",
               x_strided=True, seed=0):
    """One case of the layer kernel.  Rows [row0, row0 + num_rows) are computed; rows before and the TAIL rows behind
    are sources only.  Every virtual row -- also of the rows outside the range and of the slots >= S a launch must not
    read -- has edges; sources are drawn from all N rows in no particular order.  ``regime``:
      o1      randn rows
      range   the rows of x scaled by 2^-16 .. 2^16
      big     x, Wt scaled by 1e5 (bias by 1e10)              small   x, Wt scaled by 1e-4 (bias by 1e-8)
      zero    30 % all-zero rows; three ``bare`` rows of the range with x == 0 and no source at all; one row whose slot
              0 reads zero rows only (an all-zero block next to live ones)
      block   odd rows at 2^-20 of the even ones; slot 1 reads odd rows only, the other slots even rows only
    ``H``: zero padding beyond the true width H (x columns, weight rows of every block, weight columns, bias)."""
    vslots = S if vslots is None else vslots
    assert S <= vslots <= 4
    rng = np.random.default_rng(1000 + seed)
    g = torch.Generator().manual_seed(2000 + seed)
    N, K = row0 + num_rows + TAIL, (S + 1) * wp
    x = torch.randn(N, wp, generator=g)
    Wt = torch.randn(K, wp, generator=g) / np.sqrt(K)
    bias = torch.randn(wp, generator=g) / 4
    used = np.array([i * vslots + s for i in range(row0, row0 + num_rows) for s in range(S)])
    deg = degree_mix(N * vslots, used, rng) if edges else np.zeros(N * vslots, np.int64)
    bare = []
    if regime == "zero":
        zero = rng.random(N) < 0.3
        bare = [int(r) for r in row0 + rng.permutation(num_rows)[:3]]
        zero[bare] = True
        x[torch.from_numpy(zero)] = 0
        for r in bare:
            deg[r * vslots:(r + 1) * vslots] = 0
    vrowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    vcol = rng.integers(0, N, int(vrowptr[-1])).astype(np.int64)
    if regime == "zero":
        r = next(i for i in range(row0, row0 + num_rows) if not zero[i] and deg[i * vslots] > 0 and deg[i * vslots + 1] > 0)
        vcol[vrowptr[r * vslots]:vrowptr[r * vslots + 1]] = rng.choice(np.flatnonzero(zero), int(deg[r * vslots]))
    elif regime == "range":
        x = x * 2.0 ** torch.randint(-16, 17, (N, 1), generator=g).float()
    elif regime in ("big", "small"):
        f = 1e5 if regime == "big" else 1e-4
        x, Wt, bias = x * f, Wt * f, bias * (f * f)
    elif regime == "block":
        x[1::2] *= 2.0 ** -20
        slot = np.repeat(np.arange(N * vslots) % vslots, deg)
        vcol = 2 * (vcol // 2) + (slot == 1)
        vcol = np.where(vcol >= N, vcol - 2, vcol)
        assert ((vcol % 2 == 1) == (slot == 1)).all() and vcol.min() >= 0 and vcol.max() < N
    else:
        assert regime == "o1"
    if H is not None:
        x[:, H:] = 0
        Wt.view(S + 1, wp, wp)[:, H:, :] = 0
        Wt[:, H:] = 0
        bias[H:] = 0
    return dict(x=x, vrowptr=torch.from_numpy(vrowptr), vcol=torch.from_numpy(vcol), vslots=vslots, slots=S, Wt=Wt,
                bias=bias, row0=row0, num_rows=num_rows, regime=regime, H=H, bare=bare, out_mode=out_mode,
                x_strided=x_strided)


# name -> layer_case arguments; tests/test_wide_kernels_gpu.py runs every one, tests/test_wide_reference_host.py proves
# each one's gate reachable.  Families by the first word of the name.
CASES = {}


def _add(name, **kw):
    assert name not in CASES
    CASES[name] = dict(kw, seed=len(CASES))


for _wp in WIDTHS:                               # every instantiation, as the canonical launches run: slots 2 of 4, row0 > 0
    for _S in SLOTS:
        _add(f"instantiation Wp {_wp} S {_S}", wp=_wp, S=_S, vslots=4)
for _r0, _n in RANGES:                           # tiles, clamped rows, rows outside the range
    _add(f"range ({_r0}, {_n}) Wp 128 S 4", wp=128, S=4, row0=_r0, num_rows=_n)
    _add(f"range ({_r0}, {_n}) Wp 192 S 2", wp=192, S=2, vslots=4, row0=_r0, num_rows=_n)
_add("arguments vslots 4 slots 2 row0 37", wp=64, S=2, vslots=4, row0=37)
_add("arguments vslots 2 slots 2", wp=64, S=2, vslots=2, row0=0)
_add("arguments vslots 4 slots 4", wp=64, S=4, vslots=4, row0=0)
for _m in ("out", "out2", "both"):
    _add(f"outputs {_m}, x strided", wp=128, S=2, vslots=4, row0=5, num_rows=65, out_mode=_m)
_add("outputs both, x contiguous", wp=256, S=4, row0=5, num_rows=65, x_strided=False)
_add("degrees empty vcol Wp 64 S 2", wp=64, S=2, edges=False)
_add("degrees empty vcol Wp 256 S 4", wp=256, S=4, edges=False, row0=5, num_rows=65)
for _reg in ("range", "big", "small", "zero", "block"):
    _add(f"regime {_reg} Wp 128 S 4", wp=128, S=4, regime=_reg)
    _add(f"regime {_reg} Wp 256 S 2", wp=256, S=2, vslots=4, regime=_reg)
_add("padding H 100 in Wp 128", wp=128, S=4, H=100)
_add("padding H 32 in Wp 64", wp=64, S=2, vslots=4, H=32)
_add("padding H 100 in Wp 128, zero rows", wp=128, S=2, H=100, regime="zero")


def make(name):
    return layer_case(**CASES[name])


# csr_gather_sum_wide: every width (the early exit of lanes 4 lane >= width: 100 and 252 are no multiples of 64), every
# slot count, row counts around the four virtual rows of a workgroup
GATHER_WIDTHS, GATHER_SLOTS, GATHER_ROWS = (4, 32, 100, 128, 252, 256), (1, 2, 4), (1, 3, 4, 5, 203)


def gather_case(width, slots, num_rows, edges=True, seed=0):
    """(x [n_src, width], vrowptr [num_rows slots + 1], vcol): the degree mix of the layer cases, n_src != num_rows"""
    rng = np.random.default_rng(3000 + seed)
    g = torch.Generator().manual_seed(4000 + seed)
    n_src, nv = num_rows + 9, num_rows * slots
    deg = degree_mix(nv, np.arange(nv), rng) if edges else np.zeros(nv, np.int64)
    vrowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    vcol = rng.integers(0, n_src, int(vrowptr[-1])).astype(np.int64)
    return torch.randn(n_src, width, generator=g), torch.from_numpy(vrowptr), torch.from_numpy(vcol)
