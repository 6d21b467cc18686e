"""Host reference of the exact-fp32 GEMM family -- csrc/gemm_f32.hip (desco_gemm_f32, desco_gemm_f32_multi) and the
split-M reductions of csrc/train_ops.hip (desco_gemm_tn_f32, desco_linear_bwd_w_f32, desco_linear_bwd_w_multi_f32,
desco_colsum_f32, desco_linear_smallk_bwd_f32, desco_rowdot_bwd_f32) -- written from the documented contract alone:
numpy on the CPU, no GPU, no call into the library.  Used by tests/test_gemm_f32_kernels_gpu.py (the kernels against it)
and by tests/test_gemm_f32_reference_host.py (``fma32`` against libm's fmaf, the restated split formulas against the
library's workspace functions, the gate's reachability, and known wrong evaluators against bit-equality and the gate).

This family is held to more than a tolerance.  gemm_f32.hip states that v_mfma_f32_32x32x2_f32 is an fmaf chain per
output element in k order, train_ops.hip that every partial sum is reduced in a fixed order; so the result is defined
bit for bit, and ``evaluate(case, np.float32)`` is that definition: float32 at every step, the products fused into the
running sum by ``fma32`` (an exact fmaf), every other operation one numpy float32 operation.  ``evaluate(case)`` in
float64 is the plain mathematical reference, ``mag`` the same formula on absolute values.

A *case* is a dict (``make(name)``) with ``kind`` in gemm, tn, bwdw, colsum, rowdot, smallk, float32 numpy operands and
the placement the GPU test gives them (column blocks of wider parents, leading dimensions).  Evaluators return a dict of
the entry point's outputs.  Terms a compiler may or may not contract into an fma (the ``s`` / ``ws`` tail of gemm, its
dropout factor followed directly by accum, dw / db of rowdot_bwd, smallk_bwd) are evaluated both ways (``fused``); they
are gated, not bit-pinned.

Operands are randn, clipped to |x| >= 2^-4, times 2^randint(-8, 8) per row and per column: a product is 0 or within
2^-40 .. 2^40, every partial sum far inside the float32 normal range -- denormal handling is not what is tested, and a
dropped small term cannot hide behind a large tensor maximum because every element is judged at its own scale."""
import functools

import numpy as np

F32, F64 = np.float32, np.float64
ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2          # the values of desco_amd.ops.ACT_*
CEILING = 1e-4                                   # the family ceiling of tests/test_pool_kernels_gpu.py
BM, BN, BK = 128, 64, 32                         # gemm_f32.hip:50
TK, TN, TMC = 64, 64, 32                         # train_ops.hip:15


# ---- an exact float32 fused multiply-add ----------------------------------------------------------------------------------
def fma32(a, b, c):
    """float32(a * b + c) with ONE rounding, elementwise on float32 arrays (broadcast).  The product of two float32 is
    exact in float64 (24 + 24 bits); the float64 sum with c is rounded to odd (TwoSum gives the rounding error; where it
    is non-zero and the sum's last mantissa bit is even, the sum moves one float64 ulp towards the error), which makes
    the final cast to float32 the only rounding that counts.  The naive float32(float64(a) * b + c) rounds twice."""
    a, b, c = (np.asarray(v, F32).astype(F64) for v in (a, b, c))
    p = a * b
    p, c = np.broadcast_arrays(p, c)
    s = np.asarray(p + c)
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64)
    need = (err != 0) & ((bits & 1) == 0)
    grow = (err > 0) == (s > 0)                                  # the exact sum is larger in magnitude than s
    bits = np.where(need, np.where(grow, bits + 1, bits - 1), bits)
    return bits.view(F64).astype(F32)


def fma32_naive(a, b, c):
    """the double rounding ``fma32`` avoids (the host test shows a triple on which it is wrong)"""
    a, b, c = (np.asarray(v, F32).astype(F64) for v in (a, b, c))
    return (a * b + c).astype(F32)


DOUBLE_ROUNDING_TRIPLE = (8 * (1 + 2.0 ** -18), 8 * (1 - 2.0 ** -18), 2.0 ** 30 + 2.0 ** 7)   # fmaf gives c, naive c + 2^7


# ---- the split formulas, restated -----------------------------------------------------------------------------------------
def _slab32(m, splits):
    slab = -(-m // splits)
    return max((slab + TMC - 1) // TMC * TMC, TMC)


def tn_splits(m, k, n):
    """desco_gemm_tn_workspace (train_ops.hip:391-400) -> (splits, slab of desco_gemm_tn_f32, :410-412: rounded up to
    32, at least 32)"""
    tiles = (k // TK) * (n // TN)
    splits = max(min((1024 + tiles - 1) // max(tiles, 1), (m + 511) // 512), 1)
    return splits, _slab32(m, splits)


def bwdw_splits(m, k, n):
    """linear_bwd_w_splits (train_ops.hip:423-430; k = k1 + k2) -> (splits, slab of desco_linear_bwd_w_f32, :445-447)"""
    tiles = (k // TK + 1) * (n // TN)
    splits = max(min((1024 + tiles - 1) // tiles, (m + 255) // 256), 1)
    return splits, _slab32(m, splits)


def tn_workspace_bytes(m, k, n):
    return 4 * tn_splits(m, k, n)[0] * k * n


def bwdw_workspace_bytes(m, k, n):
    return 4 * bwdw_splits(m, k, n)[0] * (k + 1) * n


def rows_splits(m, cap):
    """desco_colsum_f32 (train_ops.hip:511-514, cap 512), desco_linear_smallk_bwd_f32 (:563-566, cap 512),
    desco_rowdot_bwd_f32 (:631-634, cap 1024): splits = min(ceil(m / 256), cap), slab = ceil(m / splits), both >= 1"""
    splits = max(min((m + 255) // 256, cap), 1)
    return splits, max(-(-m // splits), 1)


# ---- building blocks --------------------------------------------------------------------------------------------------------
def _conv(dtype, absolute):
    return (lambda t: np.abs(t.astype(dtype))) if absolute else (lambda t: t.astype(dtype))


def _const(v, dtype):
    """a float kernel argument (slope, scale): its float32 value, in the dtype of the evaluation"""
    return dtype(F32(v))


def _slabs(m, slab, splits, mutate=None):
    beg = np.arange(splits, dtype=np.int64) * slab
    end = np.minimum(beg + slab, m)
    if mutate == "slab_shift" and splits > 1:                    # the first boundary moved by 32: a reordering
        beg[1] += 32
        end[0] = min(beg[1], m)
    end = np.maximum(end, beg)
    if mutate == "drop_last_row":
        end = np.where(end > beg, end - 1, end)
    return beg, end


def _pad(x):
    """x with one zero row after the last: the row an index past a slab's end is sent to"""
    return np.concatenate([x, np.zeros((1,) + x.shape[1:], x.dtype)])


def _chain_tn(a, b, m, slab, splits, mutate=None):
    """[splits, k, n] float32: per slab ONE fmaf chain over its rows in order (train_ops.hip:39-59, :135-151: the
    32x32x2 MFMA takes rows 2 mm, 2 mm + 1 of the chunk in that order; rows past the slab's end are zero operands, and
    fma(0, 0, acc) = acc because a chain that starts at +0 never holds -0)"""
    beg, end = _slabs(m, slab, splits, mutate)
    ap, bp = _pad(a), _pad(b)
    acc = np.zeros((splits, a.shape[1], b.shape[1]), F32)
    for r in range(int((end - beg).max()) if splits else 0):
        idx = np.where(beg + r < end, beg + r, m)
        acc = fma32(ap[idx][:, :, None], bp[idx][:, None, :], acc)
    return acc


def _fold(parts, reverse=False):
    """s = 0.f; s += parts[i] in order (reduce_partials_kernel, train_ops.hip:245-246 and its kin)"""
    s = np.zeros(parts.shape[1:], F32)
    for i in (range(parts.shape[0] - 1, -1, -1) if reverse else range(parts.shape[0])):
        s = s + parts[i]
    return s


def _group_sums(x, m, slab, splits, groups, f=None, fused=False, mutate=None):
    """[splits, groups, n] float32: running sum r of slab s over rows beg + r, beg + r + groups, ... in order, each term
    x[row] (f is None), f[row] * x[row] rounded and then added (unfused) or fma32(f[row], x[row], sum) (fused)"""
    beg, end = _slabs(m, slab, splits, mutate)
    xp = _pad(x)
    fp = None if f is None else _pad(f.reshape(m, 1))
    acc = np.zeros((splits, groups, x.shape[1]), F32)
    r = np.arange(groups, dtype=np.int64)
    span = int((end - beg).max()) if splits else 0
    for j in range(-(-span // groups)):
        rows = beg[:, None] + r[None, :] + groups * j
        idx = np.where(rows < end[:, None], rows, m)
        if f is None:
            acc = acc + xp[idx]
        elif fused:
            acc = fma32(fp[idx], xp[idx], acc)
        else:
            acc = acc + fp[idx] * xp[idx]
    return acc


def _act(v, act, slope, dtype, absolute):
    if act == ACT_NONE:
        return v
    if absolute:                                                 # |act(z)| <= max(1, slope) |z|
        return v * max(1.0, float(F32(slope))) if act == ACT_LEAKY else v
    if act == ACT_RELU:
        return np.where(v > 0, v, dtype(0))
    return np.where(v > 0, v, v * _const(slope, dtype))


# ---- gemm / gemm_multi --------------------------------------------------------------------------------------------------------
def gemm(case, dtype=F64, absolute=False, fused=False, mutate=None, fac=None):
    """c = gate(drop(act([a1 | a2] wt + bias[row % bias_rows] + s ws))) (+ prev)            -> {"c": [m, n]}

    float32, the order of gemm_f32_tile: acc = 0, then one fma32 per k = 0 .. k1 + k2 - 1, a1's columns first, then
    a2's (gemm_f32.hip:123-141; the chunk's 16 MFMAs take k = 2 kk, 2 kk + 1 in order, :128-137); + bias as a float32
    add (:173-178); the tail v += s[row, j] * ws[j, col] for j = 0 .. ns - 1 (:179; unfused or ``fused``); activation
    (:180, common_device.hpp:38-42: leaky is one multiplication); times the dropout factor ``fac`` (:181; default the
    case's own); the gate on the saved output, ``> 0`` keeps (:182-185); + the previous output with accum (:186).

    Each epilogue step is its own float32 operation as long as the compiler contracts no multiplication with the add
    that follows it.  The selects of the activation and of the gate stand between their multiplications and ``+= c``;
    the one directly contractible pair is the dropout factor with accum and no gate, v * fac + c.  Cases of that pair
    (family "dropacc") are therefore gated, not bit-pinned, and ``fused`` evaluates them as fma32(v, fac, c)."""
    conv = _conv(dtype, absolute)
    f32 = dtype == F32 and not absolute
    a = case["a1"] if case["a2"] is None else np.concatenate([case["a1"], case["a2"]], 1)
    if mutate == "swap_segments" and case["a2"] is not None:
        a = np.concatenate([case["a2"], case["a1"]], 1)
    m, k = a.shape
    n = case["wt"].shape[1]
    if mutate == "row_block_shift":                              # r1 = r0 + 31: rows 32..63 of a tile read one row up
        a = a.copy()
        rows = np.arange(m)
        sel = rows[(rows % BM >= 32) & (rows % BM < 64)]
        a[sel] = a[sel - 1]
    if f32:
        ks = list(range(k))
        if mutate == "skip_chunk":
            c0 = BK if k > BK else 0
            ks = [kk for kk in ks if not c0 <= kk < c0 + BK]
        v = np.zeros((m, n), F32)
        for kk in ks:
            v = fma32(a[:, kk:kk + 1], case["wt"][kk:kk + 1, :], v)
    else:
        v = conv(a) @ conv(case["wt"])
    if case["bias"] is not None:
        br = case["bias"].shape[0]
        v = v + conv(case["bias"])[(np.arange(m) + (mutate == "bias_row_off")) % br]
    if case["s"] is not None:
        s, ws = conv(case["s"]), conv(case["ws"])
        for j in range(s.shape[1]):
            v = fma32(s[:, j:j + 1], ws[j:j + 1, :], v) if (f32 and fused) else v + s[:, j:j + 1] * ws[j:j + 1, :]
    v = _act(v, case["act"], case["slope"], dtype, absolute)
    fac = case.get("fac") if fac is None else fac
    contract = f32 and fused and fac is not None and case.get("prev") is not None and case.get("gate") is None
    if fac is not None and not contract:
        v = v * fac.astype(dtype)
    if case.get("gate") is not None:
        pos = case["gate"] >= 0 if mutate == "gate_ge" else case["gate"] > 0
        if case["gate_act"] == ACT_RELU:
            v = np.where(pos, v, dtype(0))
        elif case["gate_act"] == ACT_LEAKY:
            gs = _const(case["gate_slope"], dtype)
            v = np.where(pos, v, v * (abs(gs) if absolute else gs))
    if contract:                                                 # v * fac + prev with nothing in between: one fma
        v = fma32(v, fac, case["prev"])
    elif case.get("prev") is not None:
        v = v + conv(case["prev"])
    if mutate == "transpose_block":
        v = v.copy()
        for r0 in range(0, m - 31, 32):
            for c0 in range(0, n, 32):
                v[r0:r0 + 32, c0:c0 + 32] = v[r0:r0 + 32, c0:c0 + 32].T.copy()
    return {"c": v.astype(dtype)}


def quad_factor(m, n, p, scale, tile_relative=False):
    """a host stand-in for the dropout factor with the kernels' structure: one draw of four words per (row >> 2,
    column), word row & 3 decides the element (common_device.hpp:133-145; gemm_f32.hip:156-166 forms the quad from the
    ABSOLUTE row m0 + ...).  ``tile_relative``: the quad index taken from the row within its 128-row tile.  The words
    are a hash, not Philox: the GPU test takes the real factors from ops.dropout_mask."""
    rows = np.arange(m, dtype=np.uint64)[:, None]
    q = (rows % BM if tile_relative else rows) >> np.uint64(2)
    h = (q * np.uint64(0x9E3779B97F4A7C15) + np.arange(n, dtype=np.uint64)[None, :] * np.uint64(0xC2B2AE3D27D4EB4F)
         + (rows & np.uint64(3)) * np.uint64(0x165667B19E3779F9))
    h ^= h >> np.uint64(29)
    h *= np.uint64(0xBF58476D1CE4E5B9)
    h ^= h >> np.uint64(32)
    word = (h & np.uint64(0xffffffff)).astype(F64) / 4294967296.0
    return np.where(word < p, F32(0), F32(scale)).astype(F32)


# ---- gemm_tn, linear_bwd_w ----------------------------------------------------------------------------------------------------
def gemm_tn(case, dtype=F64, absolute=False, fused=False, mutate=None):
    """out[k, n] (+)= a^T b                                                                   -> {"out": [k, n]}

    float32: per slab (``tn_splits``) one fma32 chain over the slab's rows in order, the slab results added in slab
    order from 0.f (reduce_partials_kernel, train_ops.hip:245-246), then written or added to ``prev`` (:248)."""
    conv = _conv(dtype, absolute)
    a, b = case["a"], case["b"]
    m, k = a.shape
    n = b.shape[1]
    if dtype == F32 and not absolute:
        splits, slab = tn_splits(m, k, n)
        out = _fold(_chain_tn(a, b, m, slab, splits, mutate))
    else:
        out = conv(a).T @ conv(b)
    if case.get("prev") is not None:
        out = conv(case["prev"]) + out
    return {"out": out.astype(dtype)}


def linear_bwd_w(case, dtype=F64, absolute=False, fused=False, mutate=None):
    """dwt = [a1 | a2]^T dz, dbias = column sums of dz                          -> {"dwt": [k, n], "dbias": [n]}

    float32: the slabs of ``bwdw_splits``; per slab one fma32 chain per weight element (train_ops.hip:135-151) and, for
    the bias row, 16 running float32 sums over rows m_beg + r, m_beg + r + 16, ... folded r = 0 .. 15 from 0.f
    (:93-105); one slab: that is the result (:106-107, :153); more: the slabs folded in order from 0.f (:229-230)."""
    conv = _conv(dtype, absolute)
    a = case["a1"] if case["a2"] is None else np.concatenate([case["a1"], case["a2"]], 1)
    dz = case["dz"]
    m, k = a.shape
    n = dz.shape[1]
    if dtype == F32 and not absolute:
        splits, slab = bwdw_splits(m, k, n)
        w = _chain_tn(a, dz, m, slab, splits, mutate)
        g = _group_sums(dz, m, slab, splits, 16, mutate=mutate)
        t = np.zeros((splits, n), F32)
        for r in (range(15, -1, -1) if mutate == "bias_groups_reversed" else range(16)):
            t = t + g[:, r]
        dwt, db = (w[0], t[0]) if splits == 1 else (_fold(w), _fold(t))
    else:
        dwt, db = conv(a).T @ conv(dz), conv(dz).sum(0)
    return {"dwt": dwt.astype(dtype), "dbias": db.astype(dtype)}


# ---- colsum -----------------------------------------------------------------------------------------------------------------
def colsum_kernel(case):
    """which of the two kernels desco_colsum_f32 launches (train_ops.hip:516): "partial4" for 16-byte aligned rows with
    n % 4 == 0 and ldx % 4 == 0, else "scalar" """
    n = case["x"].shape[1]
    return "partial4" if n % 4 == 0 and case["ldx"] % 4 == 0 and case["lead"] % 4 == 0 else "scalar"


def colsum(case, dtype=F64, absolute=False, fused=False, mutate=None):
    """out[n] (+)= sum over the rows of x                                                     -> {"out": [n]}

    float32, slabs of ``rows_splits(m, 512)``.  Scalar kernel (train_ops.hip:273-279): 4 running sums over rows
    m_beg + w + 4 j, folded ((r0 + r1) + r2) + r3.  colsum_partial4_kernel (:293-323): 16 row groups, each with four
    accumulators over rows m, m + 16, m + 32, m + 48 stepping by 64 while m + 48 < m_end, the remaining rows into the
    first; (s0 + s1) + (s2 + s3); the groups folded 0 .. 15 from 0.f.  Then the slabs in order from 0.f, then
    accumulate (:245-248)."""
    conv = _conv(dtype, absolute)
    x = case["x"]
    m, n = x.shape
    if dtype == F32 and not absolute:
        splits, slab = rows_splits(m, 512)
        if colsum_kernel(case) == "scalar":
            g = _group_sums(x, m, slab, splits, 4, mutate=mutate)
            part = ((g[:, 0] + g[:, 1]) + g[:, 2]) + g[:, 3]
        else:
            beg, end = _slabs(m, slab, splits, mutate)
            xp = _pad(x)
            base = beg[:, None] + np.arange(16, dtype=np.int64)[None, :]                  # [splits, 16]
            e = end[:, None]
            nmain = np.maximum(-(-(e - (base + 48)) // 64), 0)
            s = [np.zeros((splits, 16, n), F32) for _ in range(4)]
            for t in range(int(nmain.max()) if splits else 0):
                for q in range(4):
                    s[q] = s[q] + xp[np.where(t < nmain, base + 64 * t + 16 * q, m)]
            rem = base + 64 * nmain + (16 if mutate == "remainder_skip" else 0)
            for u in range(4):
                rows = rem + 16 * u
                s[0] = s[0] + xp[np.where(rows < e, rows, m)]
            g = (s[0] + s[1]) + (s[2] + s[3])
            part = np.zeros((splits, n), F32)
            for r in range(16):
                part = part + g[:, r]
        out = _fold(part)
    else:
        out = conv(x).sum(0)
    if case.get("prev") is not None:
        out = conv(case["prev"]) + out
    return {"out": out.astype(dtype)}


# ---- smallk_bwd, rowdot_bwd ---------------------------------------------------------------------------------------------------
def smallk_bwd(case, dtype=F64, absolute=False, fused=False, mutate=None):
    """dwb[k] = sum_m feat[m, k] dout[m, :] (k < K), dwb[K] = sum_m dout[m, :]                -> {"dwb": [K + 1, 64]}

    float32 (train_ops.hip:538-553): slabs of ``rows_splits(m, 512)``; 16 running sums over rows m_beg + r + 16 j with
    the term f * v (f = 1.f for the bias row), folded r = 0 .. 15 from 0.f, the slabs folded in order from 0.f
    (:258-259).  ``fused``: the term enters by fma32."""
    conv = _conv(dtype, absolute)
    feat, dout = case["feat"], case["dout"]
    m, K = feat.shape
    if dtype == F32 and not absolute:
        splits, slab = rows_splits(m, 512)
        rows = []
        for k in range(K + 1):
            f = feat[:, k] if k < K else np.ones(m, F32)
            g = _group_sums(dout, m, slab, splits, 16, f=f, fused=fused, mutate=mutate)
            part = np.zeros((splits, 64), F32)
            for r in range(16):
                part = part + g[:, r]
            rows.append(_fold(part))
        out = np.stack(rows)
    else:
        out = np.concatenate([conv(feat).T @ conv(dout), conv(dout).sum(0, keepdims=True)])
    return {"dwb": out.astype(dtype)}


def rowdot_bwd(case, dtype=F64, absolute=False, fused=False, mutate=None):
    """dz = (y > 0) dout w^T, dwb = (y^T dout | sum dout)                        -> {"dz": [R, n], "dwb": [n + 1]}

    float32 (train_ops.hip:583-620): dz is one product d * w where y > 0, else 0.f (:594-597); slabs of
    ``rows_splits(R, 1024)``; rpi = 1024 / n running sums per column over rows r_beg + tr + rpi j with the term d * v
    (:599; the db column adds d, :600), folded g = 0 .. rpi - 1 from 0.f (:609-618), the slabs in order from 0.f."""
    conv = _conv(dtype, absolute)
    y, w, d = case["y"], case["w"], case["dout"]
    R, n = y.shape
    dz = np.where(y > 0, conv(d)[:, None] * conv(w)[None, :], dtype(0))
    if dtype == F32 and not absolute:
        splits, slab = rows_splits(R, 1024)
        rpi = 1024 // n
        g = _group_sums(y, R, slab, splits, rpi, f=d, fused=fused, mutate=mutate)
        gb = _group_sums(d.reshape(R, 1), R, slab, splits, rpi, mutate=mutate)
        part = np.zeros((splits, n + 1), F32)
        for r in range(rpi):
            part = part + np.concatenate([g[:, r], gb[:, r]], 1)
        dwb = _fold(part)
    else:
        dwb = np.concatenate([conv(y).T @ conv(d), conv(d).sum(keepdims=True)])
    return {"dz": dz.astype(dtype), "dwb": dwb.astype(dtype)}


_EVAL = {"gemm": gemm, "tn": gemm_tn, "bwdw": linear_bwd_w, "colsum": colsum, "smallk": smallk_bwd, "rowdot": rowdot_bwd}
CONTRACTIBLE = {"smallk": ("dwb",), "rowdot": ("dwb",)}          # outputs whose products a compiler may or may not fuse


def evaluate(case, dtype=F64, fused=False, mutate=None, **kw):
    """the entry point's outputs: float64 the plain mathematical reference, float32 the kernels' documented order"""
    return _EVAL[case["kind"]](case, dtype, False, fused, mutate, **kw)


def mag(case, **kw):
    """the same formula on absolute values: the scale every element is judged at"""
    return _EVAL[case["kind"]](case, F64, True, False, None, **kw)


def scaled_error(got, ref, m):
    """(E = max |got - ref| / mag over the elements, flat index of the worst one); an exact element counts 0 whatever
    mag, a wrong one at mag 0 (and a NaN) counts inf -- shmp_reference.scaled_error on numpy arrays"""
    err = np.abs(np.asarray(got, F64).reshape(ref.shape) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(err == 0, 0.0, err / m)
    e = np.where(np.isnan(e), np.inf, e).ravel()
    i = int(e.argmax()) if e.size else 0
    return (float(e[i]) if e.size else 0.0), i


def _drop_accum(case):
    return case.get("drop") is not None and case.get("prev") is not None and case.get("gate") is None


def is_pinned(case, key):
    """whether output ``key`` of the case is defined bit for bit by the documented order"""
    if case["kind"] == "gemm":
        return case["s"] is None and not _drop_accum(case)
    return key not in CONTRACTIBLE.get(case["kind"], ())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool((a.view(np.int32) == b.view(np.int32)).all())


def ulp_distance(a, b):
    """elementwise distance in float32 ulps (the integers of the two bit patterns on the number line)"""
    def key(x):
        i = np.ascontiguousarray(x, F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


# ---- the cases --------------------------------------------------------------------------------------------------------------
def _rand(rng, r, c, zeros=0.0, scaled=True):
    """randn clipped to |x| >= 2^-4, times 2^randint(-8, 8) per row and per column; ``zeros``: that share of the elements
    exactly 0, as relu outputs are"""
    x = rng.standard_normal((r, c))
    x = np.sign(x) * np.maximum(np.abs(x), 2.0 ** -4)
    if scaled:
        x = x * 2.0 ** rng.integers(-8, 8, (r, 1)) * 2.0 ** rng.integers(-8, 8, (1, c))
    if zeros:
        x = np.where(rng.random((r, c)) < zeros, 0.0, x)
    return x.astype(F32)


def _gate(rng, m, n):
    """a saved activation output: a third positive, a third negative, +0.0 and -0.0 among the rest"""
    g = _rand(rng, m, n, scaled=False)
    u = rng.random((m, n))
    g = np.where(u < 0.15, F32(0.0), np.where(u < 0.3, F32(-0.0), g))
    return g.astype(F32)


_ACTS = {"none": (ACT_NONE, 0.0), "relu": (ACT_RELU, 0.0), "leaky0.1": (ACT_LEAKY, 0.1), "leaky1.5": (ACT_LEAKY, 1.5)}


def gemm_case(seed, m, k1, k2, n, bias_rows=0, ns=0, act="none", a1_block=False, a2_ld=0, ldc3=True, zeros=0.3,
              gate=None, gate_slope=0.1, accum=False, drop=None):
    """``a1_block``: a1 is a column block (lead 4) of a wider tensor; ``a2_ld``: a2's leading dimension (0: natural);
    ``ldc3``: the output is a block of a NaN-filled parent with ldc = n + 3; ``gate``: None, "relu", "leaky" (the saved
    output has +0.0 and -0.0: neither is > 0); ``drop``: p (the GPU test regenerates the factors from a key; the host
    tests use ``quad_factor``)"""
    rng = np.random.default_rng(1000 + seed)
    a_act, slope = _ACTS[act]
    case = dict(kind="gemm", m=m, n=n, a1=_rand(rng, m, k1, zeros), a2=_rand(rng, m, k2, zeros) if k2 else None,
                wt=_rand(rng, k1 + k2, n), bias=_rand(rng, bias_rows, n) if bias_rows else None,
                s=_rand(rng, m, ns) if ns else None, ws=_rand(rng, ns, n) if ns else None, act=a_act, slope=slope,
                a1_block=a1_block, a2_ld=a2_ld, ldc=n + 3 if ldc3 else n, gate=None, gate_act=ACT_NONE, gate_slope=0.0,
                prev=None, drop=drop, fac=None)
    if gate:
        case.update(gate=_gate(rng, m, n), gate_act=ACT_RELU if gate == "relu" else ACT_LEAKY,
                    gate_slope=gate_slope if gate == "leaky" else 0.0, ldg=n + 4)
    if accum:
        case["prev"] = _rand(rng, m, n)
    if drop is not None:
        case["fac"] = quad_factor(m, n, drop, F32(1.0 / (1.0 - drop)))
    return case


def tn_case(seed, m, k, n, strided=False, out="plain", accumulate=False):
    """``strided``: a and b are column blocks of wider tensors; ``out``: "plain", "rowblock" (dwt[:k] of a [2 k, n]
    tensor, as autograd.py passes it) or "colblock" (ldo = n + 4)"""
    rng = np.random.default_rng(2000 + seed)
    return dict(kind="tn", m=m, a=_rand(rng, m, k, 0.3), b=_rand(rng, m, n), strided=strided, out=out,
                prev=_rand(rng, k, n) if accumulate else None)


def bwdw_case(seed, m, k1, k2, n, a1_block=False, want_bias=True):
    rng = np.random.default_rng(3000 + seed)
    return dict(kind="bwdw", m=m, a1=_rand(rng, m, k1, 0.3), a2=_rand(rng, m, k2, 0.3) if k2 else None,
                dz=_rand(rng, m, n), a1_block=a1_block, want_bias=want_bias)


def colsum_case(seed, m, n, place="aligned", accumulate=False):
    """``place``: "aligned" (a tensor of its own), "offset1" (parent[:, 1:n + 1]: misaligned rows, the scalar kernel at
    any n) or "ldx_odd" (a column block at offset 0 of a parent with n + 1 columns: ldx % 4 != 0 when n % 4 == 0)"""
    rng = np.random.default_rng(4000 + seed)
    lead, ldx = {"aligned": (0, n), "offset1": (1, n + 4), "ldx_odd": (0, n + 1)}[place]
    return dict(kind="colsum", m=m, x=_rand(rng, m, n), place=place, lead=lead, ldx=ldx,
                prev=_rand(rng, 1, n)[0] if accumulate else None)


def rowdot_case(seed, R, n, strided=False):
    """y is a relu output with signed zeros among its entries; ``strided``: a column block of a wider tensor"""
    rng = np.random.default_rng(5000 + seed)
    y = _rand(rng, R, n)
    u = rng.random((R, n))
    y = np.where(y < 0, F32(0.0), y)
    y = np.where(u < 0.1, F32(-0.0), y).astype(F32)
    return dict(kind="rowdot", R=R, y=y, w=_rand(rng, 1, n)[0], dout=_rand(rng, R, 1)[:, 0], strided=strided)


def smallk_case(seed, m, k, views=False):
    """``views``: feat is a column block of a wider tensor, dout a row-offset view"""
    rng = np.random.default_rng(6000 + seed)
    return dict(kind="smallk", m=m, feat=_rand(rng, m, k, 0.2), dout=_rand(rng, m, 64), views=views)


CASES = {}


def _add(name, fn, **kw):
    assert name not in CASES, name
    CASES[name] = (fn, dict(kw, seed=len(CASES)))


# gemm: every m of 1, 31, 32, 33, 127, 128, 129, 257; every (k1, k2) of (32, 0) [one chunk: the prefetch re-reads it],
# (64, 0), (32, 32), (96, 64) [odd chunk count, the segment switch inside], (576, 64); n = 64, 192; bias_rows none, 1, 7,
# 29 with m no multiple of it; ns = 0, 1, 2, 4; every activation; a1 as a column block, a2 with another ld; ldc = n + 3
_GEMM = [
    # m, k1, k2, n, bias_rows, ns, act, a1_block, a2_ld, ldc3
    (32, 32, 0, 64, 0, 0, "none", False, 0, False),              # the smallest: one tile row of one wave, one chunk
    (1, 32, 0, 64, 1, 0, "relu", False, 0, True),
    (1, 96, 64, 192, 7, 0, "leaky0.1", True, 72, True),
    (31, 64, 0, 192, 7, 0, "leaky0.1", True, 0, True),
    (32, 32, 32, 64, 29, 0, "leaky1.5", False, 40, True),
    (33, 32, 32, 64, 7, 0, "none", False, 0, True),              # bias_rows = 7 with m = 33
    (33, 96, 64, 64, 29, 0, "leaky1.5", True, 68, True),
    (127, 32, 32, 192, 29, 0, "relu", True, 36, True),
    (127, 64, 0, 64, 0, 0, "leaky0.1", False, 0, False),
    (128, 96, 64, 64, 1, 0, "leaky0.1", False, 64, True),
    (128, 576, 64, 64, 7, 0, "none", True, 0, True),
    (129, 32, 0, 192, 7, 0, "relu", True, 0, True),
    (129, 576, 64, 64, 0, 0, "none", False, 68, True),
    (257, 64, 0, 192, 7, 0, "leaky1.5", False, 0, True),
    (257, 96, 64, 64, 29, 0, "relu", True, 72, True),
    (257, 32, 0, 64, 1, 0, "none", False, 0, True),
    # the s / ws tail (gated, not bit-pinned)
    (33, 32, 0, 64, 7, 1, "relu", False, 0, True),
    (129, 64, 0, 192, 1, 2, "leaky0.1", True, 0, True),
    (257, 32, 32, 64, 0, 4, "none", False, 36, True),
    (31, 96, 64, 64, 29, 4, "leaky1.5", False, 0, False),
]
for _m, _k1, _k2, _n, _br, _ns, _a, _blk, _ld2, _c3 in _GEMM:
    _add(f"gemm m = {_m}, k = ({_k1}, {_k2}), n = {_n}, bias_rows = {_br or 'none'}, ns = {_ns}, {_a}"
         f"{', a1 column block' if _blk else ''}{f', lda2 = {_ld2}' if _ld2 else ''}, ldc = n{' + 3' if _c3 else ''}",
         gemm_case, m=_m, k1=_k1, k2=_k2, n=_n, bias_rows=_br, ns=_ns, act=_a, a1_block=_blk, a2_ld=_ld2, ldc3=_c3)

# the products of the gemm_multi launches (family "mprod"): m = 1, 129, 300, n = 64, 192; gate relu / leaky with +-0.0,
# strided ldg; accum into a prefilled output
_MPROD = [
    # tag, m, k1, k2, n, bias (1 row), act, gate, accum
    ("plain", 129, 64, 0, 64, 1, "relu", None, False),
    ("one row", 1, 32, 32, 192, 0, "none", None, False),
    ("gate relu", 300, 64, 0, 192, 0, "none", "relu", False),
    ("gate leaky accum", 129, 96, 64, 64, 0, "none", "leaky", True),
    ("accum", 300, 32, 0, 64, 1, "leaky0.1", None, True),
    ("gate relu one row", 1, 64, 0, 64, 0, "none", "relu", True),
]
for _t, _m, _k1, _k2, _n, _br, _a, _g, _acc in _MPROD:
    _add(f"mprod {_t}: m = {_m}, k = ({_k1}, {_k2}), n = {_n}", gemm_case, m=_m, k1=_k1, k2=_k2, n=_n, bias_rows=_br, act=_a,
         gate=_g, accum=_acc, ldc3=True)
# the launches: names of products; None is an m = 0 product (here in the middle of a launch)
MULTI_LAUNCHES = [
    [0], [1, 2], [0, None, 3], [2, 4, None, 5], [3, 1, 0, 4],
]

# dropout: m = 1, 3, 5, 130 (row quads cut by the range end; 130: a second tile, where the absolute row counts), act none
# / relu, gate on / off
for _m in (1, 3, 5, 130):
    for _a, _g in (("none", None), ("relu", None), ("none", "leaky"), ("relu", "relu")):
        _add(f"drop m = {_m}, {_a}, gate {_g or 'off'}", gemm_case, m=_m, k1=32, k2=0, n=64, act=_a, gate=_g, drop=0.3,
             zeros=0.0, ldc3=True)

# dropout with accum and no gate, v * fac + prev: the one pair of epilogue steps a compiler may contract (gated only)
for _m, _a in ((5, "none"), (130, "relu")):
    _add(f"dropacc m = {_m}, {_a}", gemm_case, m=_m, k1=32, k2=0, n=64, act=_a, accum=True, drop=0.3, zeros=0.0, ldc3=True)

# gemm_tn: m = 1, 31, 32, 33, 511, 512, 513 (the first split), 1025; (k, n) = (64, 64), (128, 64), (64, 128)
_TN = [
    (1, 64, 64, False, "plain", False), (31, 128, 64, True, "plain", False), (32, 64, 128, False, "colblock", False),
    (33, 64, 64, False, "rowblock", True), (511, 64, 64, True, "plain", False), (512, 128, 64, False, "colblock", False),
    (513, 64, 64, False, "rowblock", False), (513, 64, 128, True, "colblock", True), (513, 128, 64, False, "plain", False),
    (1025, 64, 64, True, "plain", True), (1025, 128, 64, False, "rowblock", False), (1025, 64, 128, False, "plain", False),
]
for _m, _k, _n, _s, _o, _acc in _TN:
    _add(f"tn m = {_m}, k = {_k}, n = {_n}{', strided a b' if _s else ''}, out {_o}{', accumulate' if _acc else ''}",
         tn_case, m=_m, k=_k, n=_n, strided=_s, out=_o, accumulate=_acc)

# linear_bwd_w: m = 0, 1, 16, 17, 32, 33, 256, 257 (the first split), 300, 1000; want_bias false on both paths
_BWDW = [
    (0, 64, 0, 64, False, True), (0, 128, 64, 128, False, False), (1, 64, 0, 64, False, True), (16, 128, 64, 64, True, True),
    (17, 64, 64, 128, False, False), (32, 64, 0, 128, False, True), (33, 128, 64, 64, True, True),
    (256, 64, 64, 64, False, True), (257, 64, 0, 64, False, True), (257, 128, 64, 128, True, False),
    (300, 64, 64, 64, False, True), (1000, 128, 64, 128, False, True), (1000, 64, 0, 64, True, False),
]
for _m, _k1, _k2, _n, _blk, _wb in _BWDW:
    _add(f"bwdw m = {_m}, k = ({_k1}, {_k2}), n = {_n}{', a1 column block' if _blk else ''}{'' if _wb else ', no bias'}",
         bwdw_case, m=_m, k1=_k1, k2=_k2, n=_n, a1_block=_blk, want_bias=_wb)
# the 16 problems of the multi launch: one-slab and split ones mixed, two with m = 0, some without dbias
BWDW_MULTI = [4, 9, 0, 11, 2, 7, 12, 3, 1, 10, 5, 8, 6, 11, 9, 2]           # positions in family("bwdw")

# colsum: n = 1, 29 (scalar kernel), 64, 100, 256 (partial4), 65; every m; 140 001 rows (512 slabs of 274 rows: the
# four-in-flight loop with a remainder); the same 64 columns aligned / misaligned / ldx % 4 != 0; accumulate
COLSUM_M = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000)
for _n in (1, 29, 64, 65, 100, 256):
    for _m in COLSUM_M:
        _add(f"colsum m = {_m}, n = {_n}", colsum_case, m=_m, n=_n)
for _n in (29, 64):
    _add(f"colsum m = 140001, n = {_n}", colsum_case, m=140001, n=_n)
for _m in (17, 257, 1000):
    _add(f"colsum m = {_m}, n = 64, misaligned parent[:, 1:65]", colsum_case, m=_m, n=64, place="offset1")
    _add(f"colsum m = {_m}, n = 64, ldx = 65", colsum_case, m=_m, n=64, place="ldx_odd")
for _m, _n in ((65, 29), (300, 64), (1000, 1), (257, 100)):
    _add(f"colsum m = {_m}, n = {_n}, accumulate", colsum_case, m=_m, n=_n, accumulate=True)

# rowdot_bwd: n = 16, 64, 256, 1024; R = 1, 255, 256, 257, 1000; 262 145 rows at n = 16 (1024 slabs of 257)
for _n in (16, 64, 256, 1024):
    for _i, _R in enumerate((1, 255, 256, 257, 1000)):
        _add(f"rowdot R = {_R}, n = {_n}{', y strided' if _i % 2 else ''}", rowdot_case, R=_R, n=_n, strided=bool(_i % 2))
_add("rowdot R = 262145, n = 16", rowdot_case, R=262145, n=16)

# smallk_bwd: k = 1, 2, 3, 16; m = 1, 15, 16, 17, 255, 256, 257; 131 073 rows (512 slabs of 257) at k = 2
for _k in (1, 2, 3, 16):
    for _i, _m in enumerate((1, 15, 16, 17, 255, 256, 257)):
        _add(f"smallk m = {_m}, k = {_k}{', views' if (_i + _k) % 2 else ''}", smallk_case, m=_m, k=_k, views=bool((_i + _k) % 2))
_add("smallk m = 131073, k = 2, views", smallk_case, m=131073, k=2, views=True)


@functools.lru_cache(maxsize=None)
def make(name):
    """the named case (built once; callers leave it unchanged)"""
    fn, kw = CASES[name]
    return dict(fn(**kw), name=name)


def family(word):
    return [n for n in CASES if n.split()[0] == word]


@functools.lru_cache(maxsize=None)
def host(name):
    """(case, fp64 reference, mag, ordered float32 evaluation, E_f32 per output) of a named case, computed once; for the
    contractible outputs E_f32 is the larger of the unfused and the fma32 evaluation"""
    case = make(name)
    ref, mg, f32 = evaluate(case), mag(case), evaluate(case, F32)
    ef = {k: scaled_error(f32[k], ref[k], mg[k])[0] for k in ref}
    fu = host_fused(name)
    if fu is not None:
        ef = {k: max(ef[k], scaled_error(fu[k], ref[k], mg[k])[0]) for k in ref}
    return case, ref, mg, f32, ef


@functools.lru_cache(maxsize=None)
def host_fused(name):
    """the float32 evaluation with the contractible products entering by fma32, or None where the case has none"""
    case = make(name)
    if case["kind"] in CONTRACTIBLE or (case["kind"] == "gemm" and (case["s"] is not None or _drop_accum(case))):
        return evaluate(case, F32, fused=True)
    return None
