"""Host reference of the single-problem split-precision GEMMs (headers of csrc/gemm_split.hip and csrc/gemm_f16x3.hip; the
docstrings of ops.gemm_split, ops.gemm_bf16, ops.gemm_f16x3, ops.gemm_split_desc and ops.linear64), written from the
documented contract alone: numpy + torch on the CPU, no call into ``desco_amd.ops``.  Used by
tests/test_gemm_split_kernels_gpu.py (the kernels against it) and by tests/test_gemm_split_reference_host.py (the reference
against a plain loop over K, and the gate against each mode's restated arithmetic and a second fp32 summation order).

    out = act(A W^T + bias[r % bias_rows] + sum_j s[r, j] ws[r % ws_rows, j, :])  *  f[r, c]  *  act'(gate[r, c])

A = [a1 | a2] [m, k1 + k2], W [n, k1 + k2]; f = the dropout factor of (row, column) from oracle/dropout.py (0 or 1 / (1 -
p)); act' = 1 where gate > 0, else 0 (relu), gate_slope (leaky) or 1 (none).  ``mode`` names the product's arithmetic:
"bf16x6" and "f16x3" are products of the fp32 operands, "bf16" is the product of the operands rounded to nearest-even
bf16.

A *case* is a dict: a1, a2, w, bias, s, ws, gate (float32 tensors or None), act / slope, gate_act / gate_slope, drop
(dict seed, step, site, p, or None), mode -- and what the GPU test launches on it: m (the kernel runs on the first m of
the parent's ``max(m, 257)`` rows; E_f32 is taken over the whole parent, because the fp32 figure of a one-row case is a
sample of 64 numbers), entry ("gemm", "desc", "linear64"), store (how ``out`` lies in its NaN-filled parent) and
a1_contig.  ``evaluate`` returns all parent rows in the dtype asked for: float64 is the reference, float32 the *fp32
evaluation* the kernels are held to (one matmul over K, then the terms added in the order above).  ``mag`` is the same
evaluation on absolute values without the activation, times f |act'|: the sum of |terms| of every output, and 0 exactly
where the element is dropped or gated out.  ``emulate`` restates the arithmetic of the case's mode."""
import numpy as np
import torch

from oracle.dropout import dropout_factor
from shmp_reference import scaled_error  # noqa: F401  (the figure every test here reports)

MODES = ("bf16x6", "bf16", "f16x3")
PARENT_ROWS = 257
ACTS = ("none", "relu", "leaky")                 # ops.ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2
STORES = ("wide", "offset5", "ldc")


# ---- the exact operations ---------------------------------------------------------------------------------------------
def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _from_hi16(u):
    """bf16 bit patterns (uint32, low 16 bits) -> float32"""
    return (u.astype(np.uint32) << np.uint32(16)).view(np.float32)


def split_bf16x3(x):
    """float32 array -> int16 [3, *x.shape]: the truncation split hi = x's upper 16 bits, mid = those of x - hi, lo =
    those of x - hi - mid (both subtractions exact), as bf16 bit patterns.  hi + mid + lo == x bit for bit."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    uh = _bits(x) & np.uint32(0xffff0000)
    r1 = x - uh.view(np.float32)
    um = _bits(r1) & np.uint32(0xffff0000)
    r2 = r1 - um.view(np.float32)
    return np.stack([uh >> np.uint32(16), um >> np.uint32(16), _bits(r2) >> np.uint32(16)]).astype(np.uint16).view(np.int16)


def round_bf16(x):
    """float32 array (finite) -> int16: round-to-nearest-even bf16 bit patterns"""
    u = _bits(x).astype(np.uint64)
    r = (u + np.uint64(0x7fff) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)
    return r.astype(np.uint16).view(np.int16)


def bf16_value(planes):
    """int16 bf16 bit patterns -> float32 values"""
    return _from_hi16(np.ascontiguousarray(planes).view(np.uint16))


def pow2_scale(mx):
    """the power of two s with s mx in [2^14, 2^15) for mx > 0 (at most 2^126), 1 for mx == 0; float32 arrays"""
    mx = np.asarray(mx, dtype=np.float32)
    _, e = np.frexp(mx)                                              # mx = f 2^e, f in [0.5, 1)
    s = np.ldexp(np.float32(1), np.minimum(15 - e, 126)).astype(np.float32)
    return np.where(mx > 0, s, np.float32(1)).astype(np.float32)


def _split_f16(v):
    """v (float32, already scaled) -> (hi, lo) float16: hi = rne(v), lo = rne(v - hi)"""
    hi = v.astype(np.float16)
    return hi, (v - hi.astype(np.float32)).astype(np.float16)


def split_f16x2(w):
    """float32 array -> (int16 [2, *w.shape], float32 [2]): the fp16 planes hi = rne(w s), lo = rne(w s - hi) and the pair
    {s, 1 / s}, s = the power of two that puts the largest |w| into [2^14, 2^15) (1 for a matrix of zeros)"""
    w = np.ascontiguousarray(w, dtype=np.float32)
    s = pow2_scale(np.abs(w).max() if w.size else np.float32(0))
    hi, lo = _split_f16(w * s)
    return np.stack([hi, lo]).view(np.int16), np.array([s, np.float32(1) / s], np.float32)


def row_absmax(a1, a2=None):
    """[m] float32: max_k |[a1 | a2][i, k]|"""
    a = np.abs(np.asarray(a1, dtype=np.float32)).max(1)
    return a if a2 is None else np.maximum(a, np.abs(np.asarray(a2, dtype=np.float32)).max(1))


# ---- the formula ----------------------------------------------------------------------------------------------------
def operands(case, dtype=torch.float64, absolute=False):
    """(A [M, K], W [n, K]) in ``dtype``; mode "bf16": both rounded to nearest-even bf16 first"""
    A = case["a1"] if case["a2"] is None else torch.cat([case["a1"], case["a2"]], 1)
    W = case["w"]
    if case["mode"] == "bf16":
        A = torch.from_numpy(bf16_value(round_bf16(A.numpy())))
        W = torch.from_numpy(bf16_value(round_bf16(W.numpy())))
    A, W = A.to(dtype), W.to(dtype)
    return (A.abs(), W.abs()) if absolute else (A, W)


def factor(case):
    """[M, n] float32: the dropout factor of the case's site (ones without one)"""
    M, n = case["a1"].shape[0], case["w"].shape[0]
    d = case["drop"]
    if d is None:
        return torch.ones(M, n)
    return torch.from_numpy(dropout_factor(d["seed"], d["step"], d["site"], d["p"], M, n))


def gate_derivative(case):
    """[M, n] float32: act'(gate) -- 1 where gate > 0, else 0 (relu), gate_slope (leaky) or 1 (none); ones without a gate"""
    M, n = case["a1"].shape[0], case["w"].shape[0]
    g = case["gate"]
    if g is None or case["gate_act"] == "none":
        return torch.ones(M, n)
    low = 0.0 if case["gate_act"] == "relu" else case["gate_slope"]
    return torch.where(g > 0, 1.0, low).float()


def _activate(z, act, slope):
    if act == "relu":
        return torch.where(z > 0, z, torch.zeros_like(z))
    if act == "leaky":
        return torch.where(z > 0, z, z * slope)
    return z


def finish(case, z, dtype=torch.float64, absolute=False, pre=False):
    """the epilogue on the product ``z`` [M, n], in the documented order: bias of the row class, the scalar tail term by
    term, the activation, the dropout factor, the gate derivative.  ``pre``: stop before the activation."""
    conv = (lambda t: t.to(dtype).abs()) if absolute else (lambda t: t.to(dtype))    # noqa: E731
    M = z.shape[0]
    r = torch.arange(M)
    if case["bias"] is not None:
        b = conv(case["bias"])
        z = z + (b if b.dim() == 1 else b[r % b.shape[0]])
    if case["s"] is not None:
        s, ws = conv(case["s"]), conv(case["ws"])
        for j in range(s.shape[1]):
            z = z + s[:, j:j + 1] * ws[r % ws.shape[0], j, :]
    if pre:
        return z
    if not absolute:
        z = _activate(z, case["act"], case["slope"])
    return z * conv(factor(case)) * conv(gate_derivative(case))


def product(case, dtype=torch.float64, absolute=False, order="whole"):
    """A W^T.  ``order``: "whole" (one matmul over K) or "blocks_reversed" (one matmul per 32-wide K block, accumulated
    from the last block to the first)."""
    A, W = operands(case, dtype, absolute)
    if order == "whole":
        return A @ W.t()
    assert order == "blocks_reversed"
    z = None
    for k in range(A.shape[1] - 32, -1, -32):
        part = A[:, k:k + 32] @ W[:, k:k + 32].t()
        z = part if z is None else z + part
    return z


def evaluate(case, dtype=torch.float64, absolute=False, order="whole", pre=False):
    return finish(case, product(case, dtype, absolute, order), dtype, absolute, pre)


def mag(case):
    return evaluate(case, torch.float64, absolute=True)


# ---- the kernels' arithmetic, restated -----------------------------------------------------------------------------------
def _steps(K):
    return range(0, K, 16)


def accumulate_bf16x6(A, W):
    """truncation split of both operands; per 16-deep step lo hi, hi lo, mid mid, mid hi, hi mid, hi hi into an fp32
    accumulator (A's plane first).  (Host arithmetic: the sum inside one step is numpy's, not the MFMA's.)"""
    ah, am, al = (bf16_value(p) for p in split_bf16x3(A))
    bh, bm, bl = (bf16_value(p).T.copy() for p in split_bf16x3(W))
    acc = np.zeros((A.shape[0], W.shape[0]), np.float32)
    for k in _steps(A.shape[1]):
        a, b = slice(k, k + 16), slice(k, k + 16)
        for x, y in ((al, bh), (ah, bl), (am, bm), (am, bh), (ah, bm), (ah, bh)):
            acc = acc + x[:, a] @ y[b]
    return acc


def accumulate_bf16(A, W):
    """one nearest-even bf16 plane per operand, one product per 16-deep step, fp32 accumulator"""
    a, b = bf16_value(round_bf16(A)), bf16_value(round_bf16(W)).T.copy()
    acc = np.zeros((A.shape[0], W.shape[0]), np.float32)
    for k in _steps(A.shape[1]):
        acc = acc + a[:, k:k + 16] @ b[k:k + 16]
    return acc


def accumulate_f16x3(A, W):
    """one power of two per row of A (over the whole K extent) and one per weight matrix; nearest-even hi / lo fp16
    split of the scaled operands; lo hi, hi lo, hi hi per 16-deep step into an fp32 accumulator; the scales undone"""
    f32 = np.float32
    planes, wsc = split_f16x2(W)
    bh, bl = (p.astype(f32).T.copy() for p in planes.view(np.float16))
    sc = pow2_scale(row_absmax(A))
    ah, al = (p.astype(f32) for p in _split_f16(A * sc[:, None]))
    acc = np.zeros((A.shape[0], W.shape[0]), f32)
    for k in _steps(A.shape[1]):
        a, b = slice(k, k + 16), slice(k, k + 16)
        for x, y in ((al, bh), (ah, bl), (ah, bh)):
            acc = acc + x[:, a] @ y[b]
    return acc * ((f32(1) / sc) * wsc[1])[:, None]


ACCUMULATE = {"bf16x6": accumulate_bf16x6, "bf16": accumulate_bf16, "f16x3": accumulate_f16x3}


def emulate(case):
    """the documented arithmetic of the case's mode on the host -> [M, n] float32 (the epilogue in float32, in order)"""
    A = case["a1"] if case["a2"] is None else torch.cat([case["a1"], case["a2"]], 1)
    acc = ACCUMULATE[case["mode"]](A.numpy(), case["w"].numpy())
    return finish(case, torch.from_numpy(acc), torch.float32)


# ---- the cases --------------------------------------------------------------------------------------------------------
def split_case(mode, m, n, k1, k2=0, regime="o1", bias_rows=1, ns=0, ws_rows=1, act="none", slope=0.1, gate=None,
               gate_slope=0.2, drop_p=None, entry="gemm", store="wide", a1_contig=False, seed=0):
    """One case.  The operands are drawn as a parent of max(m, 257) rows.  ``bias_rows``: 0 = no bias, 1 = [n], more =
    [bias_rows, n].  ``regime``:
      o1      randn rows, weights randn / sqrt(K)
      range   the rows of A scaled by 2^-16 .. 2^16
      big     A, W, s, ws scaled by 1e5 (bias by 1e10)         small   by 1e-4 (bias by 1e-8)
      inrow   the even columns of A at 2^-20 of the odd ones
      zero    30 % all-zero rows (s too): such a row is act(bias), and exactly 0 without a bias"""
    assert mode in MODES and act in ACTS and store in STORES and k1 % 32 == 0 and k2 % 32 == 0 and n % 64 == 0
    g = torch.Generator().manual_seed(7000 + seed)
    M, K = max(m, PARENT_ROWS), k1 + k2
    A = torch.randn(M, K, generator=g)
    W = torch.randn(n, K, generator=g) / np.sqrt(K)
    bias = torch.randn(max(bias_rows, 1), n, generator=g) / 4
    s = torch.randn(M, max(ns, 1), generator=g)
    ws = torch.randn(ws_rows, max(ns, 1), n, generator=g) / 4
    gt = torch.randn(M, n, generator=g)
    aux = torch.rand(M, generator=g)
    expo = torch.randint(-16, 17, (M, 1), generator=g)
    if regime == "range":
        A = A * 2.0 ** expo.float()
    elif regime in ("big", "small"):
        f = 1e5 if regime == "big" else 1e-4
        A, W, s, ws, bias = A * f, W * f, s * f, ws * f, bias * (f * f)
    elif regime == "inrow":
        A[:, 0::2] *= 2.0 ** -20
    elif regime == "zero":
        A[aux < 0.3] = 0
        s[aux < 0.3] = 0
    else:
        assert regime == "o1"
    if gate is not None:                            # +0.0, -0.0 and negative values next to positive ones
        gt.view(-1)[0::7] = 0.0
        gt.view(-1)[3::7] = -0.0
    drop = None if drop_p is None else dict(seed=0x5eed0000 + seed, step=11 + seed, site=seed % 256, p=drop_p)
    slope, gate_slope = float(np.float32(slope)), float(np.float32(gate_slope))     # the kernels take them as C floats
    return dict(mode=mode, m=m, n=n, k1=k1, k2=k2, regime=regime, entry=entry, store=store, a1_contig=a1_contig,
                a1=A[:, :k1].contiguous(), a2=A[:, k1:].contiguous() if k2 else None, w=W,
                bias=None if bias_rows == 0 else (bias[0] if bias_rows == 1 else bias),
                s=s if ns else None, ws=ws if ns else None, act=act, slope=slope,
                gate=gt if gate is not None else None, gate_act=gate or "none", gate_slope=gate_slope, drop=drop)


# name -> split_case arguments; tests/test_gemm_split_kernels_gpu.py runs every one, tests/test_gemm_split_reference_host.py
# proves each one's gate reachable.  Families by the first word of the name.
CASES = {}


def _add(name, **kw):
    assert name not in CASES
    i = len(CASES)
    kw.setdefault("store", STORES[i % 3] if kw.get("entry") != "linear64" else "wide")
    CASES[name] = dict(kw, seed=i)


ROW_EDGES = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129)
SEAMS = ((32, 0), (64, 0), (96, 0), (160, 0), (32, 32), (64, 32), (32, 96))
REGIMES = ("o1", "range", "big", "small", "inrow", "zero")
EPILOGUE_N = (64, 128, 192)
LINEAR64_M, LINEAR64_N = (1, 63, 64, 65, 257), (64, 128, 192)

for _mode in MODES:
    for _n in (64, 128, 192, 256, 320, 384):     # WN = 1, 2, 3; ny = 2, 5, 2
        _add(f"instantiation {_mode} n {_n}", mode=_mode, m=129, n=_n, k1=96)
    for _m in ROW_EDGES:                          # 32-row half tiles, 64-row wave tiles, the 128-row block
        _add(f"rows {_mode} m {_m}", mode=_mode, m=_m, n=64, k1=32, k2=32)
    _add(f"rows {_mode} m 1025 n 64", mode=_mode, m=1025, n=64, k1=64)          # nine row tiles: the second XCD round
    _add(f"rows {_mode} m 1153 n 384", mode=_mode, m=1153, n=384, k1=32, k2=32)  # local / ny and local % ny both > 0
    for _k1, _k2 in SEAMS:                        # one chunk, the prologue of two, the clamp of three; the operand seam
        _add(f"seam {_mode} k ({_k1}, {_k2})", mode=_mode, m=129, n=64, k1=_k1, k2=_k2, a1_contig=(_k1, _k2) == (64, 32))
    _add(f"seam {_mode} k (576, 0) anchor", mode=_mode, m=300, n=576, k1=576)
    for _reg in REGIMES:
        _add(f"regime {_mode} {_reg} (129, 64, 128)", mode=_mode, m=129, n=64, k1=64, k2=64, regime=_reg)
        _add(f"regime {_mode} {_reg} (257, 192, 192)", mode=_mode, m=257, n=192, k1=192, regime=_reg,
             bias_rows=0 if _reg == "zero" else 1)
    for _n in (64, 192):
        for _st in STORES:
            _add(f"store {_mode} {_st} n {_n}", mode=_mode, m=129, n=_n, k1=96, store=_st)
for _n in EPILOGUE_N:                             # m = 333: 29 and 37 row classes wrap inside and across the tiles
    _e = dict(mode="bf16x6", entry="desc", m=333, n=_n, k1=32, k2=32)
    for _br in (1, 29):
        _add(f"epilogue desc n {_n} bias_rows {_br}", **_e, bias_rows=_br)
    for _ns in (1, 3, 4):
        for _wr in (1, 29, 37):
            _add(f"epilogue desc n {_n} tail ns {_ns} ws_rows {_wr}", **_e, ns=_ns, ws_rows=_wr)
    _add(f"epilogue desc n {_n} tail ns 3 ws_rows 5", **_e, ns=3, ws_rows=5)      # below 28: a lane's rows wrap more than once
    _add(f"epilogue desc n {_n} act relu", **_e, act="relu")
    _add(f"epilogue desc n {_n} act leaky", **_e, act="leaky")
    _add(f"epilogue desc n {_n} gate relu", **_e, gate="relu")
    _add(f"epilogue desc n {_n} gate leaky", **_e, gate="leaky")
    _add(f"epilogue desc n {_n} drop 0.3", **_e, drop_p=0.3)
    _add(f"epilogue desc n {_n} drop 1.0", **_e, drop_p=1.0)
    _add(f"epilogue desc n {_n} gate drop tail", **_e, bias_rows=29, ns=3, ws_rows=37, act="leaky", gate="leaky", drop_p=0.3)
    _add(f"epilogue desc n {_n} gate relu drop tail relu", **_e, ns=4, ws_rows=29, act="relu", gate="relu", drop_p=0.3)
    # (a negative gate slope: the only setting in which the gate applied before the activation is another function)
    _add(f"epilogue desc n {_n} gate slope -0.25 drop relu", **_e, act="relu", gate="leaky", gate_slope=-0.25, drop_p=0.3)
    for _mode in ("f16x3", "bf16"):
        _g = dict(mode=_mode, m=333, n=_n, k1=32, k2=32)
        for _br in (1, 29):
            _add(f"epilogue {_mode} n {_n} bias_rows {_br}", **_g, bias_rows=_br, act="relu")
        for _ns in (1, 3, 4):
            _add(f"epilogue {_mode} n {_n} tail ns {_ns}", **_g, ns=_ns, act="leaky")
for _n in LINEAR64_N:                             # the streaming projection: same arithmetic, K = 64
    for _i, _m in enumerate(LINEAR64_M):
        _add(f"linear64 m {_m} n {_n}", mode="bf16x6", entry="linear64", m=_m, n=_n, k1=64,
             act=ACTS[(_i + _n // 64) % 3], bias_rows=(_i + _n // 64) % 2)


def make(name):
    return split_case(**CASES[name])


def family(case_or_name):
    """the family a case's worst ratio is reported under"""
    c = CASES[case_or_name] if isinstance(case_or_name, str) else case_or_name
    entry = c.get("entry", "gemm")
    return {"desc": "desc epilogue", "linear64": "linear64"}.get(entry, c["mode"])


# ---- the routing probe --------------------------------------------------------------------------------------------------
def routing_case(mode, n, K, m=129):
    """(A [m, K], W [n, K], want [m, n]): row i of A is 2^(i % 5) at column perm(i) = (5 i + 3) % K and 0 elsewhere, so
    out[i, j] = 2^(i % 5) W[j, perm(i)] exactly in every mode.  W holds the distinct integers 1 + j K + k (<= 18 432: 15
    bits, exact in hi + mid + lo and in the fp16 hi + lo); for the single bf16 plane of mode "bf16", which holds 8 bits,
    the integers 1 + (31 j + 7 k) % 255, distinct along every row and every column stretch of 8."""
    j, k = np.arange(n)[:, None], np.arange(K)[None, :]
    W = (1 + (31 * j + 7 * k) % 255 if mode == "bf16" else 1 + j * K + k).astype(np.float32)
    i = np.arange(m)
    perm = (5 * i + 3) % K
    A = np.zeros((m, K), np.float32)
    A[i, perm] = 2.0 ** (i % 5)
    want = (2.0 ** (i % 5))[:, None] * W[:, perm].T
    return torch.from_numpy(A), torch.from_numpy(W), torch.from_numpy(want.astype(np.float32))
