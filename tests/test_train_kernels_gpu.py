"""The training step's kernels, each against a plain fp64 evaluation of the same operation on the host.

Tolerance rule (per element, never against a tensor's maximum):
  * elementwise kernels with at most one fp32 rounding per element are bit-equal to torch's fp32 evaluation of the same
    expression in the same order;
  * reductions and products satisfy |got - ref| <= tau * mag element by element, where ref is the fp64 reference and mag
    is that reference evaluated on the absolute values of every input and upstream gradient (the sum of |terms| for a
    multilinear output; an upper bound through relu / leaky masks, whose derivative factors become 1).  tau = 1e-5 unless
    a case's longest sequential fp32 chain of n additions needs more: then n * 2^-24 bounds its relative error, and such a
    case takes tau = 1e-4 (``_tau``), never more.
Every test prints its worst error / bound as a ``[parity]`` line."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from desco_amd import _lib, ops  # noqa: E402

DEV = "cuda"
LOG2E = 1.4426950408889634


def _tau(chain):
    """tau for a reduction whose longest sequential fp32 chain has ``chain`` additions (its worst-case relative error is
    chain * 2^-24): 1e-5 while that stays below it, else 1e-4 (up to chains of 1677)."""
    gamma = chain * 2.0 ** -24
    assert gamma <= 1e-4, chain
    return 1e-5 if gamma <= 1e-5 else 1e-4


def _bounded(name, got, ref, mag, tau):
    """|got - ref| <= tau * mag element by element (mag == 0: exact); returns the worst error / bound."""
    got = got.detach().cpu().double().reshape(ref.shape)
    err = (got - ref).abs()
    bound = tau * mag
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)       # (err > 0 at bound 0: inf)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"[parity] {name}: worst error / bound = {worst:.3e} (tau {tau:.0e})")
    if not worst <= 1.0:
        i = int(torch.nan_to_num(ratio, nan=float("inf")).flatten().argmax())
        raise AssertionError(f"{name}: element {i}: got {float(got.flatten()[i])!r}, ref {float(ref.flatten()[i])!r}, "
                             f"bound {float(bound.flatten()[i])!r} (worst error / bound {worst:.3e})")
    return worst


def _bitequal(name, got, want):
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape)
    bad = int((got.view(torch.int32 if got.dtype == torch.float32 else got.dtype) !=
               want.view(torch.int32 if want.dtype == torch.float32 else want.dtype)).sum())
    print(f"[parity] {name}: {bad} of {got.numel()} elements differ in any bit (error / bound = {0.0 if bad == 0 else 'inf'})")
    assert bad == 0, name


def _f32(x):
    return torch.tensor(x, dtype=torch.float32)


# ---- elementwise: act_grad, act_grad_dropout, copy2d_multi, fill, add_rows (bit-equal) ------------------------------
def _act_ref(v, c, act, slope):
    """the kernels' order: v (already dc or dc * factor), then relu / leaky on the sign of the saved output c"""
    if act == ops.ACT_RELU:
        return torch.where(c > 0, v, torch.zeros_like(v))
    if act == ops.ACT_LEAKY:
        return torch.where(c > 0, v, v * _f32(slope))
    return v


def _with_signed_zeros(c):
    c = c.clone().flatten()
    c[::5] = 0.0
    c[1::7] = -0.0
    return c


@pytest.mark.parametrize("act", [ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LEAKY])
@pytest.mark.parametrize("n", [1, 255, 256 * 37 + 77])
def test_act_grad_is_the_fp32_expression(act, n):
    g = torch.Generator().manual_seed(n + act)
    dc = torch.randn(n, generator=g)
    c = _with_signed_zeros(torch.randn(n, generator=g))
    assert (c == 0).any() and (torch.signbit(c) & (c == 0)).any() or n < 8
    got = ops.act_grad(dc.to(DEV), c.to(DEV), act, 0.1)
    _bitequal(f"act_grad act={act} n={n}", got, _act_ref(dc, c, act, 0.1))


@pytest.mark.parametrize("act", [ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LEAKY])
@pytest.mark.parametrize("R,C", [(1, 29), (1001, 29), (258, 64), (131, 256)])
def test_act_grad_dropout_is_the_fp32_expression(act, R, C):
    g = torch.Generator().manual_seed(R * C + act)
    dc = torch.randn(R, C, generator=g)
    c = _with_signed_zeros(torch.randn(R, C, generator=g)).view(R, C)
    key = ops.rng_next(DEV)
    drop = ops.DropSite(key, 7, 0.2)
    f = ops.dropout_mask(drop, R, C).cpu()
    assert R < 8 or ((f == 0).any() and (f != 0).any())
    got = ops.act_grad(dc.to(DEV), c.to(DEV), act, 0.1, drop=drop)
    _bitequal(f"act_grad_dropout act={act} R={R} C={C}", got, _act_ref(dc * f, c, act, 0.1))


def test_copy2d_multi_two_launches_transpose_accumulate_and_strides():
    """27 descriptors (the entry splits them into launches of 24), empty ones interleaved, plain / transposed copies
    with and without accumulate, sizes not multiples of 32, strided source and destination views."""
    g = torch.Generator().manual_seed(27)
    probs, wants = [], []
    for i in range(27):
        if i % 6 == 2:
            rows, cols = (0, 37) if i % 12 == 2 else (45, 0)
        else:
            rows, cols = 1 + (i * 37) % 97, 1 + (i * 53) % 75
        tr, acc = bool(i % 2), bool((i // 2) % 2)
        src_buf = torch.randn(rows + 3, cols + 11, generator=g)
        src = src_buf[2:2 + rows, 5:5 + cols]
        drows, dcols = (cols, rows) if tr else (rows, cols)
        dst_buf = torch.randn(drows + 2, dcols + 9, generator=g)
        want = dst_buf.clone()
        v = src.t() if tr else src
        want[1:1 + drows, 4:4 + dcols] = (want[1:1 + drows, 4:4 + dcols] + v) if acc else v
        sd, dd = src_buf.to(DEV), dst_buf.to(DEV)
        probs.append((sd[2:2 + rows, 5:5 + cols], dd[1:1 + drows, 4:4 + dcols], tr, acc))
        wants.append((dd, want))
    ops.copy2d_multi(probs)
    for i, (dd, want) in enumerate(wants):
        _bitequal(f"copy2d_multi descriptor {i}", dd, want)          # (the bytes around each view untouched)


@pytest.mark.parametrize("n", [1, 255, 256 * 9 + 3])
def test_fill(n):
    t = torch.full((n,), 7.0, device=DEV)
    for v in (0.0, -0.0, 3.25, float("inf")):
        _bitequal(f"fill n={n} value={v}", ops.fill(t, v), torch.full((n,), v))


@pytest.mark.parametrize("rows,cols", [(1, 4), (257, 64), (1001, 192)])
def test_add_rows(rows, cols):
    g = torch.Generator().manual_seed(rows + cols)
    dbuf, sbuf = torch.randn(rows, cols + 8, generator=g), torch.randn(rows, cols + 12, generator=g)
    want = dbuf.clone()
    want[:, 4:4 + cols] = dbuf[:, 4:4 + cols] + sbuf[:, 8:8 + cols]
    dd = dbuf.to(DEV)
    ops.add_rows(dd[:, 4:4 + cols], sbuf.to(DEV)[:, 8:8 + cols])
    _bitequal(f"add_rows {rows}x{cols}", dd, want)


# ---- exact: segment_ids, split_bf16_planes_batch --------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [[1], [0, 3, 0, 0, 17, 1], list(range(40)) * 30])
def test_segment_ids_equal_repeat_interleave(sizes):
    sz = torch.tensor(sizes, dtype=torch.long)
    ptr = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(sz, 0)]).to(torch.int32)
    got = ops.segment_ids(ptr.to(DEV), int(sz.sum()))
    want = torch.repeat_interleave(torch.arange(len(sizes)), sz).to(torch.int32)
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("nb,rows,cols", [(1, 64, 64), (8, 320, 64), (3, 128, 192)])
def test_split_bf16_planes_batch_is_the_per_matrix_split(nb, rows, cols):
    g = torch.Generator().manual_seed(nb * rows + cols)
    w = (torch.randn(nb, rows, cols, generator=g) * torch.rand(nb, rows, 1, generator=g) * 50).to(DEV)
    w[0, 0, :4] = torch.tensor([0.0, -0.0, 1e-30, -3e-39])              # zeros, a denormal
    for tr in (False, True):
        got3 = ops.split_bf16_planes_batch(w, tr, 3)
        got1 = ops.split_bf16_planes_batch(w, tr, 1)
        for i in range(nb):
            want3 = ops.split_bf16_planes_t(w[i]) if tr else ops.split_bf16_planes(w[i])
            want1 = ops.round_bf16(w[i].t().contiguous() if tr else w[i])
            assert torch.equal(got3[i], want3), (i, tr)
            assert torch.equal(got1[i, 0], want1), (i, tr)
    print(f"[parity] split_bf16_planes_batch nb={nb} {rows}x{cols}: bit-equal to the per-matrix splits (error / bound = 0)")


# ---- affine_scalar ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_mul", [False, True])
@pytest.mark.parametrize("use_add", [False, True])
@pytest.mark.parametrize("use_addv", [False, True])
def test_affine_scalar(use_mul, use_add, use_addv):
    """a * mul + add + addv: the multiply-add may contract into an fma, so the reduction rule, not bit-equality"""
    g = torch.Generator().manual_seed(4 * use_mul + 2 * use_add + use_addv)
    n = 256 * 5 + 17
    a = torch.randn(n, generator=g) * 10
    mul, add, addv = torch.randn(1, generator=g), torch.randn(1, generator=g), torch.randn(n, generator=g)
    got = ops.affine_scalar(a.to(DEV), mul.to(DEV) if use_mul else None, add.to(DEV) if use_add else None,
                            addv.to(DEV) if use_addv else None)
    ad = a.double()
    ref, mag = ad.clone(), ad.abs()
    if use_mul:
        ref, mag = ref * mul.double(), mag * mul.double().abs()
    if use_add:
        ref, mag = ref + add.double(), mag + add.double().abs()
    if use_addv:
        ref, mag = ref + addv.double(), mag + addv.double().abs()
    _bounded(f"affine_scalar mul={use_mul} add={use_add} addv={use_addv}", got, ref, mag, 1e-5)


# ---- rowdot2 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncols", [1, 63, 64, 65, 256])
def test_rowdot2(ncols):
    g = torch.Generator().manual_seed(ncols)
    R = 1001
    a, b = torch.randn(R, ncols, generator=g), torch.randn(R, ncols, generator=g)
    got = ops.rowdot2(a.to(DEV), b.to(DEV))
    ref = (a.double() * b.double()).sum(1)
    mag = (a.double().abs() * b.double().abs()).sum(1)
    _bounded(f"rowdot2 ncols={ncols}", got, ref, mag, _tau(ncols // 64 + 1 + 6))    # lane chain + 6 butterfly levels


# ---- loss_fwd --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("count", [1, 255, 2049, 2_100_000])
def test_loss_fwd(mode, count):
    """mode 0: mean smooth_l1(pred - log2(y + 1)); mode 1: sum log2(|pred - y| + 1).  Residuals straddle |d| = 1, y has
    zeros, and mode 1 has exact zeros of d (its gradient there is 0).  Per-element scale of dpred: the rounding of its
    inputs through the formula -- mode 0 (|pred| + |log2(y + 1)| + |d|) / count, mode 1 log2(e) / (|d| + 1) times
    (1 + (|pred| + |y|) / (|d| + 1)).  The loss: the sum of its terms' magnitudes with the same sensitivities."""
    g = torch.Generator().manual_seed(count + mode)
    y = torch.floor(torch.rand(count, generator=g) ** 3 * 40)
    y[::3] = 0.0
    t = torch.log2(y.double() + 1) if mode == 0 else y.double()
    d = torch.randn(count, generator=g, dtype=torch.float64) * 1.5
    d[1::4] = torch.sign(d[1::4]) * (1.0 + (torch.rand(len(d[1::4]), generator=g, dtype=torch.float64) - 0.5) * 1e-3)
    pred = (t + d).float()
    if mode == 1:
        pred[::5] = y[::5]                                   # d == 0 exactly
    loss, dpred = ops.loss_fwd(pred.to(DEV), y.to(DEV), mode)
    p = pred.double()
    dd = p - t
    ad = dd.abs()
    base = p.abs() + t.abs()
    if mode == 0:
        terms = torch.where(ad < 1, 0.5 * dd * dd, ad - 0.5)
        ref_l = terms.sum() / count
        mag_l = (terms + torch.clamp(ad, max=1.0) * base).sum() / count
        ref_d = torch.where(ad < 1, dd, torch.sign(dd)) / count
        mag_d = (base + ad) / count
    else:
        assert (dd == 0).any()
        terms = torch.log2(ad + 1)
        ref_l = terms.sum()
        mag_l = (terms + LOG2E * base / (ad + 1)).sum()
        ref_d = torch.sign(dd) * LOG2E / (ad + 1)
        mag_d = LOG2E / (ad + 1) * (1 + base / (ad + 1))
    blocks = min((count + 2047) // 2048, 1024)
    chain = -(-count // (blocks * 256)) + 8 + blocks          # per thread, the block's tree, the partials in one lane
    _bounded(f"loss mode={mode} count={count}: loss", loss.reshape(1), ref_l.reshape(1), mag_l.reshape(1), _tau(chain))
    _bounded(f"loss mode={mode} count={count}: dpred", dpred, ref_d, mag_d, 1e-5)


# ---- count_head_bwd / count_head_wide ------------------------------------------------------------------------------------
def _head_inputs(B, Q, hid, seed):
    g = torch.Generator().manual_seed(seed)
    tbuf = torch.randn(B + 1, hid + 8, generator=g)
    qbuf = torch.randn(Q + 2, hid + 4, generator=g)
    t, qh = tbuf[1:, 8:], qbuf[2:, 4:]                       # strided views
    if B:
        t[::3, ::2] = -qh[0, ::2]                           # T + Qh == 0 exactly for query 0
        t[1::3, 1::4] = -qh[Q - 1, 1::4]
    w2 = torch.randn(hid, generator=g) / 16
    return tbuf, qbuf, t, qh, w2


@pytest.mark.parametrize("B,Q,hid", [(0, 29, 256), (1, 1, 64), (15, 32, 1024), (17, 29, 256), (512, 29, 256),
                                     (512, 1, 1024), (512, 32, 64), (20000, 29, 64), (20000, 1, 1024)])
def test_count_head_bwd(B, Q, hid):
    """dT, dQh, dw2 of b2 + sum_c w2[c] leaky(T[b, c] + Qh[q, c]) by fp64 autograd (chunks of rows); B = 20000 is past
    the 1024-slab cap.  mag: |w2| sum |dl| for dT / dQh, sum |dl| (|T| + |Qh|) for dw2."""
    slope = 0.01
    tbuf, qbuf, t, qh, w2 = _head_inputs(B, Q, hid, B + Q + hid)
    dl = torch.randn(B, Q, generator=torch.Generator().manual_seed(B)) if B else torch.empty(0, Q)
    tb, qb = tbuf.to(DEV), qbuf.to(DEV)
    dt, dqh, dw2 = ops.count_head_bwd(tb[1:, 8:], qb[2:, 4:], w2.to(DEV), slope, dl.to(DEV))
    Td, Qd, Wd = t.double(), qh.double().requires_grad_(True), w2.double().requires_grad_(True)
    ref_dt = torch.zeros(B, hid, dtype=torch.float64)
    step = max(1, 2_000_000 // max(1, Q * hid))
    for b0 in range(0, B, step):
        Tc = Td[b0:b0 + step].clone().requires_grad_(True)
        out = (Wd * torch.nn.functional.leaky_relu(Tc[:, None, :] + Qd[None], slope)).sum(-1)
        out.backward(dl[b0:b0 + step].double())
        ref_dt[b0:b0 + step] = Tc.grad
    ref_dqh = Qd.grad if Qd.grad is not None else torch.zeros(Q, hid, dtype=torch.float64)
    ref_dw2 = Wd.grad if Wd.grad is not None else torch.zeros(hid, dtype=torch.float64)
    adl, aw = dl.double().abs(), w2.double().abs()
    mag_dt = adl.sum(1, keepdim=True) * aw
    mag_dqh = adl.sum(0)[:, None] * aw
    at, aq = Td.abs(), qh.double().abs()
    mag_dw2 = adl.sum(0) @ aq + adl.sum(1) @ at if B else torch.zeros(hid, dtype=torch.float64)
    splits = min(max((B + 15) // 16, 1), 1024)
    chain_b = -(-B // splits) + splits                      # rows of a slab, then the slabs
    _bounded(f"count_head_bwd B={B} Q={Q} hid={hid}: dT", dt, ref_dt, mag_dt, _tau(Q + 1))
    _bounded(f"count_head_bwd B={B} Q={Q} hid={hid}: dQh", dqh, ref_dqh, mag_dqh, _tau(chain_b + 1))
    _bounded(f"count_head_bwd B={B} Q={Q} hid={hid}: dw2", dw2, ref_dw2, mag_dw2, _tau(Q * -(-B // splits) + splits))


@pytest.mark.parametrize("B,Q,hid", [(1, 1, 64), (255, 8, 320), (257, 9, 1024), (257, 32, 64), (255, 32, 320),
                                     (1_048_577, 1, 64)])
@pytest.mark.parametrize("exp2", [False, True])
def test_count_head_wide(B, Q, hid, exp2):
    """logit = b2 + sum_c w2[c] leaky(T + Qh) (or 2^logit - 1) for hid in {64, 320, 1024}, partial query groups, b2 as a
    float and as a device tensor, ``out`` a column slice; B = 1 048 577 runs the grid-stride loop past 4096 blocks.
    mag of a logit: |b2| + sum |w2| (|T| + |Qh|); of 2^logit - 1: 2^logit (1 + ln 2 mag)."""
    slope = 0.01
    tbuf, qbuf, t, qh, w2 = _head_inputs(B, Q, hid, B * 3 + Q + hid)
    tb, qb, wd = tbuf.to(DEV), qbuf.to(DEV), w2.to(DEV)
    b2 = 0.3
    res = []
    for b2_arg in (b2, torch.tensor([b2], device=DEV)):
        obuf = torch.full((B, Q + 3), 5.0, device=DEV)
        ops.count_head_wide(tb[1:, 8:], qb[2:, 4:], wd, b2_arg, slope, exp2, out=obuf[:, 2:2 + Q])
        assert float((obuf[:, :2] - 5.0).abs().max()) == 0 and float((obuf[:, 2 + Q:] - 5.0).abs().max()) == 0
        res.append(obuf[:, 2:2 + Q].cpu())
    assert torch.equal(res[0], res[1])
    b2d = float(torch.tensor(b2, dtype=torch.float32))
    Qd, aq, Wd, aw = qh.double(), qh.double().abs(), w2.double(), w2.double().abs()
    ref = torch.empty(B, Q, dtype=torch.float64)
    mag = torch.empty(B, Q, dtype=torch.float64)
    step = max(1, 4_000_000 // (Q * hid))
    for b0 in range(0, B, step):
        Tc = t[b0:b0 + step].double()
        ref[b0:b0 + step] = b2d + (Wd * torch.nn.functional.leaky_relu(Tc[:, None, :] + Qd[None], slope)).sum(-1)
        mag[b0:b0 + step] = abs(b2d) + (aw * (Tc.abs()[:, None, :] + aq[None])).sum(-1)
    if exp2:
        e = torch.exp2(ref)
        ref, mag = e - 1, e * (1 + np.log(2.0) * mag)
    _bounded(f"count_head_wide B={B} Q={Q} hid={hid} exp2={exp2}", res[0], ref, mag, _tau(hid + 1))


# ---- affine_rows / affine_rows_bwd ------------------------------------------------------------------------------------------
def _act64(x, act, slope):
    return [x, torch.relu(x), torch.nn.functional.leaky_relu(x, slope)][act]


@pytest.mark.parametrize("ks,qv,R,with_base", [(1, 1, 1, False), (3, 29, 29 * 37 + 5, True), (6, 64, 1001, False),
                                               (8, 29, 3000, True), (3, 29, 262_144 + 29 * 7 + 3, True)])
@pytest.mark.parametrize("act", [ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LEAKY])
def test_affine_rows(ks, qv, R, with_base, act):
    """out[r] = act(base[r] + sum_k c[r, k] v[r % qv, k]) and its dropout form (factor from dropout_mask); R > 262 144
    takes the grid-stride loop a second time.  mag: |base| + sum |c| |v| (times the factor)."""
    g = torch.Generator().manual_seed(ks * 1000 + qv + R)
    c = torch.randn(R, ks, generator=g)
    c[::11] = 0.0
    v = torch.randn(qv, ks, 64, generator=g)
    base = torch.randn(R, 64, generator=g) if with_base else None
    bd = base.double() if with_base else torch.zeros(R, 64, dtype=torch.float64)
    vr = v.double()[torch.arange(R) % qv]                                  # [R, ks, 64]
    z = bd + (c.double()[:, :, None] * vr).sum(1)
    zmag = bd.abs() + (c.double().abs()[:, :, None] * vr.abs()).sum(1)
    ref = _act64(z, act, 0.1)
    got = ops.affine_rows(None if base is None else base.to(DEV), c.to(DEV), v.to(DEV), act, 0.1)
    _bounded(f"affine_rows ks={ks} qv={qv} R={R} base={with_base} act={act}", got, ref, zmag, _tau(ks + 1))
    drop = ops.DropSite(ops.rng_next(DEV), 3, 0.25)
    f = ops.dropout_mask(drop, R, 64).cpu().double()
    got = ops.affine_rows(None if base is None else base.to(DEV), c.to(DEV), v.to(DEV), act, 0.1, drop)
    _bounded(f"affine_rows dropout ks={ks} qv={qv} R={R} act={act}", got, ref * f, zmag * f, _tau(ks + 2))


@pytest.mark.parametrize("ks,qv,num_i", [(1, 1, 0), (3, 29, 0), (8, 64, 1), (1, 29, 1023), (6, 29, 1024), (3, 64, 1025),
                                         (8, 1, 1025), (3, 1, 70001), (8, 1, 70001)])
def test_affine_rows_bwd(ks, qv, num_i):
    """dv[q, k] = sum_i c[i qv + q, k] dz[i qv + q]: one slab up to 1024 nodes, 2..64 slabs beyond, the 64-slab cap at
    70001.  mag: sum |c| |dz|."""
    g = torch.Generator().manual_seed(ks + qv + num_i)
    R = num_i * qv
    cbuf, zbuf = torch.randn(R + 1, ks, generator=g), torch.randn(R + 1, 64, generator=g)
    c, dz = cbuf[:R], zbuf[:R]                                  # (views of a live buffer also when empty)
    c[5::13] = 0.0
    got = ops.affine_rows_bwd(cbuf.to(DEV)[:R], zbuf.to(DEV)[:R], qv)
    cq = c.double().view(num_i, qv, ks)
    zq = dz.double().view(num_i, qv, 64)
    ref = torch.einsum("iqk,iqc->qkc", cq, zq)
    mag = torch.einsum("iqk,iqc->qkc", cq.abs(), zq.abs())
    splits = min(max((num_i + 1023) // 1024, 1), 64)
    slab = -(-num_i // splits) if num_i else 1
    _bounded(f"affine_rows_bwd ks={ks} qv={qv} num_i={num_i} ({splits} slabs)", got, ref, mag,
             _tau(-(-slab // 4) + 4 + splits))                  # a wave's rows, the four waves, the slabs


# ---- gossip_gather ------------------------------------------------------------------------------------------------------------
def _degree_graph():
    """one symmetric CSR with nodes of degree 0, 1, 2, 3, 4 and a hub (300 leaves), lo / hi neighbours on both sides"""
    edges, n = [], 0

    def add(k, es):
        nonlocal n
        edges.extend((a + n, b + n) for a, b in es)
        n += k
    add(1, [])                                                   # degree 0
    add(3, [(0, 1), (1, 2)])                                     # path: 1, 2, 1
    add(4, [(a, b) for a in range(4) for b in range(a + 1, 4)])  # K4: 3
    add(5, [(a, b) for a in range(5) for b in range(a + 1, 5)])  # K5: 4
    add(301, [(150, v) for v in range(301) if v != 150])          # hub in the middle: 300
    e = np.array(edges + [(b, a) for a, b in edges], dtype=np.int64)
    order = np.lexsort((e[:, 1], e[:, 0]))
    e = e[order]
    ptr = np.zeros(n + 1, np.int64)
    np.add.at(ptr, e[:, 0] + 1, 1)
    return n, np.cumsum(ptr), e[:, 0], e[:, 1]


@pytest.mark.parametrize("Q,gated", [(1, False), (29, False), (64, False), (1, True), (64, True)])
def test_gossip_gather(Q, gated):
    """out[i, q] = sum_j w_ijq h[j, q]: signed mode (g = None: +1 for j < i, -1 for j > i, the gate gradients) and gated
    mode (g[q] for j < i, 1 - g[q] for j > i).  mag: sum |w| |h|."""
    n, ptr, r, c = _degree_graph()
    deg = np.diff(ptr)
    assert {0, 1, 2, 3, 4, 300} <= set(deg.tolist())
    g = torch.Generator().manual_seed(Q + gated)
    h = torch.randn(n * Q, 64, generator=g)
    gv = torch.rand(Q, generator=g) if gated else None
    got = ops.gossip_gather(h.to(DEV), torch.from_numpy(ptr).int().to(DEV), torch.from_numpy(c).int().to(DEV), n, Q,
                            None if gv is None else gv.to(DEV))
    lo = torch.from_numpy(c < r)[:, None].double()
    if gated:
        w = lo * gv.double() + (1 - lo) * (1 - gv.double())                # [E, Q]
    else:
        w = (2 * lo - 1).expand(-1, Q)
    hd = h.double().view(n, Q, 64)
    rr, cc = torch.from_numpy(r), torch.from_numpy(c)
    ref = torch.zeros(n, Q, 64, dtype=torch.float64).index_add_(0, rr, hd[cc] * w[..., None])
    mag = torch.zeros(n, Q, 64, dtype=torch.float64).index_add_(0, rr, hd[cc].abs() * w.abs()[..., None])
    _bounded(f"gossip_gather Q={Q} {'gated' if gated else 'signed'}", got, ref.view(n * Q, 64), mag.view(n * Q, 64),
             _tau(int(deg.max()) + 1))


# ---- segment_sum_layers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lx,with_extra", [(1, False), (8, True)])
def test_segment_sum_layers(Lx, with_extra):
    g = torch.Generator().manual_seed(Lx)
    sizes = torch.randint(0, 40, (300,), generator=g)
    sizes[[0, 7, 299]] = 0
    sizes[5] = 700
    ptr = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(sizes, 0)])
    num_rows = int(ptr[-1])
    xall = torch.randn(Lx, num_rows + 13, 64, generator=g)               # N > num_rows: rows past them unused
    extra = torch.randn(300, 64 * Lx + 32, generator=g) if with_extra else None
    out = torch.full((300, 64 * Lx + 64), 3.0, device=DEV)
    ops.segment_sum_layers(xall.to(DEV), num_rows, ptr.int().to(DEV), 300,
                           None if extra is None else extra.to(DEV)[:, 32:], out[:, 64:])
    seg = torch.repeat_interleave(torch.arange(300), sizes)
    ref = torch.zeros(300, Lx, 64, dtype=torch.float64).index_add_(0, seg, xall[:, :num_rows].double().transpose(0, 1))
    mag = torch.zeros(300, Lx, 64, dtype=torch.float64).index_add_(0, seg, xall[:, :num_rows].double().abs().transpose(0, 1))
    if with_extra:
        ref += extra[:, 32:].double().view(300, Lx, 64)
        mag += extra[:, 32:].double().abs().view(300, Lx, 64)
    assert float((out[:, :64] - 3.0).abs().max()) == 0
    _bounded(f"segment_sum_layers Lx={Lx} extra={with_extra}", out[:, 64:], ref.view(300, Lx * 64),
             mag.view(300, Lx * 64), _tau(int(sizes.max()) + 1))


# ---- shmp_bwd_dx (and vcsr_transpose_sym) --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def train_batch():
    from helpers import golden_graphs, random_family_graphs
    from desco_amd.batch import NeighborhoodBatch
    from desco_amd.graphs import GraphSet
    from desco_amd.partition import build_partition
    stars = [(k + 1, [(0, v) for v in range(1, k + 1)]) for k in (8, 12, 30)]          # centre rows of 8, 12, 30 entries
    graphs = golden_graphs(max_n=60)[:20] + random_family_graphs(5, 22) + stars
    part = build_partition(GraphSet.from_edge_lists(graphs), 4)
    return NeighborhoodBatch(part, DEV)


def _adjoint_index(batch):
    """(dst row of each forward edge's virtual row, its slot, its source row) from the FORWARD index"""
    vrowptr = batch.vrowptr.cpu().long()
    vcol = batch.vcol.cpu().long()
    S = batch.slots
    vrow = torch.repeat_interleave(torch.arange(batch.num_rows * S), vrowptr[1:] - vrowptr[:-1])
    return vrow // S, vrow % S, vcol


def test_vcsr_transpose_sym_is_the_transpose_of_the_forward_index(train_batch):
    b = train_batch
    ti = b.train_index()
    k, s, src = _adjoint_index(b)
    S, N = b.slots, b.num_rows
    t_rowptr, t_col = ti["t_rowptr"].cpu().long(), ti["t_col"].cpu().long()
    cnt = torch.bincount(src, minlength=N)
    assert torch.equal(t_rowptr, torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(cnt, 0)]))
    # row j's entries: exactly the virtual rows k S + s that gather j, ascending
    order = torch.from_numpy(np.lexsort(((k * S + s).numpy(), src.numpy())))
    assert torch.equal(t_col, (k * S + s)[order])
    assert torch.equal(ti["t_col_s1"].cpu().long(), t_col + t_col // S)
    rp2, tc2 = ops.vcsr_transpose_sym(b.vrowptr, b.vcol, N, S, b.num_count)       # the entry point itself, once more
    assert torch.equal(rp2, ti["t_rowptr"]) and torch.equal(tc2, ti["t_col"])
    print(f"[parity] vcsr_transpose_sym: {t_col.numel()} entries equal the transposed forward index (error / bound = 0)")


@pytest.mark.parametrize("with_dcanon", [False, True])
@pytest.mark.parametrize("with_relu", [False, True])
@pytest.mark.parametrize("mask_scale", [1.0, 1.0 / (1.0 - 0.2)])
def test_shmp_bwd_dx(train_batch, with_dcanon, with_relu, mask_scale):
    """out[i] = mask_i (seed_i + D[i, self block] + sum over the virtual rows k S + s that gathered i of D[k, slot s]),
    the reference built as the adjoint of the forward gather (vrowptr / vcol), then the last-layer call form of
    autograd.ShmpTrunk (a stride-0 zero D, an all-zero t_rowptr).  mag: the same sums of absolute values."""
    b = train_batch
    ti = b.train_index()
    N, Nc, S, B = b.num_rows, b.num_count, b.slots, b.num_graphs
    t_rowptr = ti["t_rowptr"].cpu().long()
    tdeg = t_rowptr[1:] - t_rowptr[:-1]
    assert N % 16 != 0 and Nc < N
    for lo, hi in ((1, 7), (8, 8), (9, 16), (17, 10 ** 9)):           # (every row of a real batch has an entry: rows
        assert ((tdeg >= lo) & (tdeg <= hi)).any(), (lo, hi)           #  without one, below, with an all-zero t_rowptr)
    g = torch.Generator().manual_seed(int(with_dcanon) * 4 + int(with_relu) * 2 + int(mask_scale != 1.0))
    H = 64
    off_count, off_canon = 4 * H, 2 * H
    D = torch.randn(N, (S + 1) * H, generator=g)
    dpool = torch.randn(B, 3 * H, generator=g)[:, H:2 * H]
    dcanon = torch.randn(B, 2 * H, generator=g)[:, :H] if with_dcanon else None
    relu_src = torch.relu(torch.randn(N, H, generator=g)) if with_relu else None
    if with_relu:
        relu_src[::9, ::3] = 0.0
    seg = torch.repeat_interleave(torch.arange(B), torch.from_numpy(np.diff(b._seg_ptr_host())))
    assert torch.equal(ti["seg_id"].cpu().long(), seg)

    def reference(Dd, with_edges):
        seed = torch.zeros(N, H, dtype=torch.float64)
        seed[:Nc] = dpool.double()[seg]
        if with_dcanon:
            seed[Nc:] = dcanon.double()
        sb = torch.cat([Dd[:Nc, off_count:off_count + H], Dd[Nc:, off_canon:off_canon + H]])
        ref, mag = seed + sb, seed.abs() + sb.abs()
        if with_edges:
            k, s, src = _adjoint_index(b)
            blk = Dd.view(N, S + 1, H)[k, s]
            ref = ref.index_add(0, src, blk)
            mag = mag.index_add(0, src, blk.abs())
        if with_relu:
            m = (relu_src.double() > 0) * float(torch.tensor(mask_scale, dtype=torch.float32))
            ref, mag = ref * m, mag * m
        return ref, mag

    args = (ti["seg_id"],)
    kw = dict(dcanon=None if dcanon is None else dcanon.to(DEV), relu_src=None if relu_src is None else relu_src.to(DEV),
              mask_scale=mask_scale)
    dp = torch.randn(B, 3 * H, generator=torch.Generator()).to(DEV)
    dp[:, H:2 * H] = dpool.to(DEV)
    got = ops.shmp_bwd_dx(D.to(DEV), ti["t_rowptr"], ti["t_col_s1"], Nc, off_count, off_canon, dp[:, H:2 * H], *args,
                          **kw)
    ref, mag = reference(D.double(), True)
    name = f"shmp_bwd_dx dcanon={with_dcanon} relu={with_relu} scale={mask_scale:g}"
    _bounded(name, got, ref, mag, _tau(int(tdeg.max()) + 2))
    # rows without transposed entries: the same D with an all-zero t_rowptr (seed + self block alone) ...
    empty_ptr = torch.zeros(N + 1, device=DEV, dtype=torch.int32)
    got = ops.shmp_bwd_dx(D.to(DEV), empty_ptr, ti["t_col_s1"], Nc, off_count, off_canon, dp[:, H:2 * H], *args, **kw)
    ref, mag = reference(D.double(), False)
    _bounded(name + " (no transposed entries)", got, ref, mag, 1e-5)
    # ... and the last layer's form: one zero row for D (row stride 0), no transposed entries
    zero_d = torch.zeros((1, (S + 1) * H), device=DEV).expand(N, -1)
    got = ops.shmp_bwd_dx(zero_d, empty_ptr, ti["t_col_s1"], Nc, off_count, off_canon, dp[:, H:2 * H], *args, **kw)
    ref, mag = reference(torch.zeros(N, (S + 1) * H, dtype=torch.float64), False)
    _bounded(name + " (last layer form)", got, ref, mag, 1e-5)


# ---- gemm_split_multi -----------------------------------------------------------------------------------------------------------
def _split_problems(g, drop):
    """four problems: a2 + bias + relu; leaky gate; relu gate + dropout; an empty one"""
    probs, refs = [], []
    for i, (m, k1, k2, n) in enumerate(((1001, 64, 64, 64), (300, 128, 0, 128), (777, 64, 32, 64), (0, 64, 0, 64))):
        a1 = torch.randn(m, k1, generator=g) * 3
        a2 = torch.randn(m, k2, generator=g) if k2 else None
        w = torch.randn(n, k1 + k2, generator=g) / np.sqrt(k1 + k2)        # [out, in]
        bias = torch.randn(n, generator=g) if i == 0 else None
        gate = torch.randn(m, n, generator=g) if i in (1, 2) else None
        if gate is not None:
            gate[::4, ::3] = 0.0
        kw = [dict(act=ops.ACT_RELU), dict(gate_act=ops.ACT_LEAKY, gate_slope=0.1), dict(gate_act=ops.ACT_RELU, drop=drop),
              dict()][i]
        probs.append((a1, a2, w, bias, gate, kw))
    return probs


def _split_ref(a1, a2, w, bias, gate, kw, f, rnd=None):
    A = a1 if a2 is None else torch.cat([a1, a2], 1)
    if rnd is not None:
        A, w = rnd(A), rnd(w)
    A, w = A.double(), w.double()
    z, mag = A @ w.T, A.abs() @ w.abs().T
    if bias is not None:
        z, mag = z + bias.double(), mag + bias.double().abs()
    if kw.get("act") == ops.ACT_RELU:
        z = torch.relu(z)
    if "drop" in kw:
        z, mag = z * f, mag * f
    if gate is not None:
        d = torch.where(gate.double() > 0, 1.0, kw.get("gate_slope", 0.0) if kw["gate_act"] == ops.ACT_LEAKY else 0.0)
        z, mag = z * d, mag * d
    return z, mag


def _bf16_rne(x):
    return x.to(torch.bfloat16).float()


@pytest.mark.parametrize("planes_per_weight", [3, 1])
def test_gemm_split_multi(planes_per_weight):
    """desco_gemm_bf16x6_multi_f32 (three planes: fp32-accurate, against fp64 and against gemm_multi with the same
    descriptors) and desco_gemm_bf16_multi_f32 (one plane: the fp64 product of round-to-nearest bf16 operands), with a2,
    bias, relu / leaky gates, dropout and an empty problem.  mag: |A| |W| (+ |bias|) times the gate / dropout factor."""
    g = torch.Generator().manual_seed(planes_per_weight)
    drop = ops.DropSite(ops.rng_next(DEV), 9, 0.3)
    probs = _split_problems(g, drop)
    dprobs, planes, outs = [], [], []
    for a1, a2, w, bias, gate, kw in probs:
        m, n = a1.shape[0], w.shape[0]
        out = torch.empty(m, n, device=DEV)
        pr = dict(a1=a1.to(DEV), a2=None if a2 is None else a2.to(DEV), out=out,
                  bias=None if bias is None else bias.to(DEV), gate=None if gate is None else gate.to(DEV), **kw)
        dprobs.append(pr)
        planes.append(ops.split_bf16_planes_batch(w.to(DEV)[None], False, planes_per_weight)[0])
        outs.append(out)
    ops.gemm_split_multi(dprobs, planes)
    for i, ((a1, a2, w, bias, gate, kw), out) in enumerate(zip(probs, outs)):
        m, n = out.shape
        if m == 0:
            continue
        f = ops.dropout_mask(drop, m, n).cpu().double() if "drop" in kw else None
        k = w.shape[1]
        if planes_per_weight == 3:
            ref, mag = _split_ref(a1, a2, w, bias, gate, kw, f)
            _bounded(f"gemm_split_multi bf16x6 problem {i} (k={k}) vs fp64", out, ref, mag, _tau(k + 2))
            want = torch.empty(m, n, device=DEV)
            pr = dict(dprobs[i], out=want, wt=w.t().contiguous().to(DEV))
            ops.gemm_multi([pr])
            _bounded(f"gemm_split_multi bf16x6 problem {i} vs gemm_multi", out, want.cpu().double(), 2 * mag, _tau(k + 2))
            assert torch.equal(out == 0, want == 0) or "drop" not in kw
        else:
            ref, mag = _split_ref(a1, a2, w, bias, gate, kw, f, rnd=_bf16_rne)
            _bounded(f"gemm_split_multi bf16 problem {i} (k={k}) vs fp64 of bf16 operands", out, ref, mag, _tau(k + 2))


def test_gemm_split_entry_points_refuse_dropout_site_256():
    """The kernels build the dropout counter as col | site << 24 in 32 bits: site 256 would draw site 0's mask.  Every
    entry point that takes a descriptor rejects it (DropSite refuses it in Python; this goes through ctypes)."""
    L = _lib.lib()
    g = torch.Generator().manual_seed(256)
    m, k, n = 64, 64, 64
    a1 = torch.randn(m, k, generator=g).to(DEV)
    w = torch.randn(n, k, generator=g).to(DEV)
    out = torch.zeros(m, n, device=DEV)
    key = ops.rng_next(DEV)
    d = _lib.GemmDesc()
    d.a1, d.lda1, d.k1, d.n, d.m = a1.data_ptr(), k, k, n, m
    d.c, d.ldc = out.data_ptr(), n
    d.drop = ops.DropSite(key, 5, 0.5).desc()
    d.drop.site = 256
    p3 = ops.split_bf16_planes(w)
    p1 = ops.round_bf16(w)[None].contiguous()
    rc = L.desco_gemm_bf16x6_desc_f32(ctypes.byref(d), p3.data_ptr(), 1, ops._stream())
    assert rc == -1 and b"desco_gemm_bf16x6_desc_f32" in L.desco_last_error() and b"site" in L.desco_last_error()
    descs = (_lib.GemmDesc * 1)(d)
    for fn, pl in ((L.desco_gemm_bf16x6_multi_f32, p3), (L.desco_gemm_bf16_multi_f32, p1)):
        ptrs = (ctypes.c_void_p * 1)(pl.data_ptr())
        rc = fn(1, descs, ptrs, ops._stream())
        assert rc == -1 and b"site must be < 256" in L.desco_last_error(), L.desco_last_error()
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0                         # nothing launched
    d.drop.site = 255                                            # the last valid site runs
    assert L.desco_gemm_bf16x6_desc_f32(ctypes.byref(d), p3.data_ptr(), 1, ops._stream()) == 0
    torch.cuda.synchronize()
    print("[parity] dropout site 256: refused by desco_gemm_bf16x6_desc_f32 / _multi_f32 / bf16_multi_f32")


# ---- fold_shmp_fwd / fold_shmp_bwd ----------------------------------------------------------------------------------------------
def _neigh_model(tconv, L):
    from desco_amd.lightning_model import NeighborhoodCountingModel
    from helpers import neigh_args
    torch.manual_seed(11 + L + 2 * tconv)
    nm = NeighborhoodCountingModel(1, 64, neigh_args(use_tconv=tconv, layer_num=L)).to_hetero_old(tconv, tconv)
    with torch.no_grad():
        for p in nm.parameters():
            p.add_(0.05 * torch.randn(p.shape))
    return nm


@pytest.mark.parametrize("tconv", [True, False])
@pytest.mark.parametrize("L", [8, 1])
def test_fold_shmp_native(tconv, L):
    """(Wt, fb) of every row type by desco_fold_shmp_fwd against gnn_model.pack_shmp_stacked on a float64 copy, and the
    gradient of every raw parameter (desco_fold_shmp_bwd: ops.fold_shmp_bwd in FoldShmp.backward) for random (dWt, dfb)
    against fp64 autograd.  use_tconv=False
    ties two slots to one weight (their gradients sum).  mag: the same folding / backward on absolute values."""
    import copy
    from desco_amd import gnn_model as GM
    nm = _neigh_model(tconv, L)
    nm64 = copy.deepcopy(nm).double()
    nmabs = copy.deepcopy(nm).double()
    with torch.no_grad():
        for p in nmabs.parameters():
            p.abs_()
    nm = nm.to(DEV)
    for attr in ("emb_model", "emb_model_query"):
        gnn, g64, gabs = getattr(nm, attr), getattr(nm64, attr), getattr(nmabs, attr)
        ref_all, mag_all = GM.pack_shmp_stacked(g64), GM.pack_shmp_stacked(gabs)
        for t in gnn.gnn_core.node_types:
            wt, fb = GM.fold_shmp_native(gnn, t)
            sp = gnn._fold_specs[t]
            wt2, fb2 = ops.fold_shmp_fwd(sp.table, sp.L, sp.S, sp.NU)          # (what FoldShmp.forward launches)
            assert torch.equal(wt2, wt) and torch.equal(fb2, fb)
            rwt, rfb = ref_all[t]
            mwt, mfb = mag_all[t]
            name = f"fold_shmp tconv={tconv} L={L} {attr}/{t}"
            _bounded(name + ": Wt", wt, rwt.detach(), mwt.detach(), 1e-5)
            _bounded(name + ": fb", fb, rfb.detach(), mfb.detach(), 1e-5)
            g = torch.Generator().manual_seed(L)
            dwt, dfb = torch.randn(wt.shape, generator=g), torch.randn(fb.shape, generator=g)
            params = dict(gnn.named_parameters())
            p64 = dict(g64.named_parameters())
            pabs = dict(gabs.named_parameters())
            for p in list(params.values()) + list(p64.values()) + list(pabs.values()):
                p.grad = None
            ((wt * dwt.to(DEV)).sum() + (fb * dfb.to(DEV)).sum()).backward()
            ((rwt * dwt.double()).sum() + (rfb * dfb.double()).sum()).backward()
            ((mwt * dwt.double().abs()).sum() + (mfb * dfb.double().abs()).sum()).backward()
            n = 0
            for pn, p in params.items():
                if p64[pn].grad is None:
                    assert p.grad is None or float(p.grad.abs().max()) == 0.0, pn
                    continue
                assert p.grad is not None, pn
                _bounded(f"{name}: d {pn}", p.grad, p64[pn].grad, pabs[pn].grad, _tau(64 * (L + 1)))
                n += 1
            assert n >= 4 * L, (name, n)


# ---- gossip_fold_fwd / gossip_fold_bwd ------------------------------------------------------------------------------------------
def _fold_gossip_reference(gm, E, w_pre, b_pre):
    """the operands of the more-than-64-queries branch of gnn_model.gossip_forward_train (torch ops, differentiable), in
    FoldGossip's output order"""
    from desco_amd import gnn_model as GM
    core = gm.emb_model.gnn_core
    H = 64
    Q = E.shape[0]
    c1 = core.convs[1]
    C1, cb1, D1, db1 = c1.lin_com.weight, c1.lin_com.bias, c1.lin_update.weight, c1.lin_update.bias
    (g0, g1), p, r, t, z, tp, zp = GM._gossip_layer0_terms(core, gm.emb_model.post_mp[0], E, w_pre, b_pre)
    r, t = r.expand(Q, H), t.expand(Q, H)
    V0 = torch.stack([p, g0[:, None] * p, r, g0[:, None] * r, t, z], 1)
    D1a, D1b = D1[:, :H], D1[:, H:]
    wt1 = torch.cat([(D1a @ C1).t(), D1b.t()], 0)
    u = GM._mv(D1a, cb1).expand(Q, H)
    V1 = torch.stack([u, g1[:, None] * u, db1.expand(Q, H)], 1)
    P0 = gm.emb_model.post_mp[0].weight
    He = H
    wtp = torch.cat([P0[:, He + H:He + 2 * H].t(), P0[:, He + 2 * H:He + 3 * H].t()], 0)
    Vp = torch.stack([tp.expand(Q, H), zp], 1)
    post = gm.emb_model.post_mp
    return dict(V0=V0, g1=g1, g1c=1 - g1, wt1=wt1, V1=V1, wtp=wtp, Vp=Vp, w3t=post[3].weight.t(), w5t=post[5].weight.t())


_FG_OUT = ("V0", "g1", "g1c", "wt1", "V1", "wtp", "Vp", "w3t", "w5t")


def _fold_gossip_args(gm, E, w_pre, b_pre):
    core = gm.emb_model.gnn_core
    c0, c1 = core.convs[0], core.convs[1]
    gl = [c.lin_gate for c in (c0, c1)]
    post = gm.emb_model.post_mp
    return (E, w_pre, b_pre, c0.lin_com.weight, c0.lin_com.bias, c0.lin_update.weight, c0.lin_update.bias,
            c1.lin_com.weight, c1.lin_com.bias, c1.lin_update.weight, c1.lin_update.bias,
            gl[0][0].weight, gl[0][0].bias, gl[0][2].weight, gl[0][2].bias, gl[1][0].weight, gl[1][0].bias,
            gl[1][2].weight, gl[1][2].bias, post[0].weight, post[0].bias, post[3].weight, post[5].weight)


@pytest.mark.parametrize("Q", [1, 29, 64])
@pytest.mark.parametrize("with_dg1", [False, True])
def test_fold_gossip(Q, with_dg1):
    """autograd.FoldGossip (desco_gossip_fold_fwd / _bwd: ops.gossip_fold_fwd, and ops.gossip_fold_bwd in its backward) against the fp64 torch-op construction of the same operands
    (the Q > 64 branch of the gossip training pass) differentiated by autograd: every operand and every parameter
    gradient, with the gate gradient dg1 absent and present.  mag: the same construction on absolute values of the
    parameters, E and the upstream gradients -- through the sigmoids of the gates a magnitude, not a bound."""
    import copy
    from desco_amd import autograd as AG
    from helpers import make_models
    _, gm = make_models(seed=Q)
    gm64 = copy.deepcopy(gm).double()
    gabs = copy.deepcopy(gm).double()
    with torch.no_grad():
        for p in gabs.parameters():
            p.abs_()
    gm = gm.to(DEV)
    g = torch.Generator().manual_seed(Q + 100 * with_dg1)
    E = torch.randn(Q, 64, generator=g)
    core = gm.emb_model.gnn_core
    w_pre, b_pre = core.pre_mp[0].weight[:, 0].detach(), core.pre_mp[0].bias.detach()
    outs = AG.FoldGossip.apply(*_fold_gossip_args(gm, E.to(DEV), w_pre.contiguous(), b_pre.contiguous()))
    got = dict(zip(_FG_OUT, outs))
    O = ops.gossip_fold_fwd(AG.FoldGossip._pack(*_fold_gossip_args(gm, E.to(DEV), w_pre.contiguous(), b_pre.contiguous())[:3],
                                                _fold_gossip_args(gm, E.to(DEV), w_pre, b_pre)[3:]))
    assert all(torch.equal(O[k], got[k]) for k in _FG_OUT)
    wp64, bp64 = w_pre.double().cpu(), b_pre.double().cpu()
    ref = _fold_gossip_reference(gm64, E.double(), wp64, bp64)
    mag = _fold_gossip_reference(gabs, E.double().abs(), wp64.abs(), bp64.abs())
    mag["g1c"] = 1 + mag["g1"]                                   # (1 - g1: the magnitudes of its two terms)
    for k in _FG_OUT:
        _bounded(f"fold_gossip Q={Q}: {k}", got[k], ref[k].detach(), mag[k].detach(), 1e-5)
    ups = {k: torch.randn(tuple(ref[k].shape), generator=g, dtype=torch.float64) for k in _FG_OUT if k != "g1c"}
    if not with_dg1:
        del ups["g1"]
    sum(((got[k] * ups[k].float().to(DEV)).sum() for k in ups)).backward()
    sum(((ref[k] * ups[k]).sum() for k in ups)).backward()
    sum(((mag[k] * ups[k].abs()).sum() for k in ups)).backward()
    n = 0
    params, p64, pabs = (dict(m.named_parameters()) for m in (gm, gm64, gabs))
    for pn, p in params.items():
        r = p64[pn].grad
        if r is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, pn
            continue
        assert p.grad is not None, pn
        # the gates' own parameters: their gradient passes through sigma' = sigma (1 - sigma) of both sigmoids, formed
        # in fp32 -- 1 - sigma near sigma = 1 carries sigma's rounding relative to 1 - sigma, which the magnitude of the
        # absolute values does not see (measured up to 5x tau = 1e-5 on lin_gate.0.weight): tau = 1e-4 for them
        tau = 1e-4 if ".lin_gate." in pn else _tau(64 + Q + 64)
        _bounded(f"fold_gossip Q={Q} dg1={with_dg1}: d {pn}", p.grad, r, pabs[pn].grad, tau)
        n += 1
    assert n >= 20, n
