"""Host reference of the fused-pooling family (the producers' partial rows -- csrc/shmp_layer16.hip's POOL epilogue and
degree_affine_pool_kernel -- and their consumers: pool_reduce_kernel / pool_reduce_multi_kernel in csrc/graph_ops.hip, the
POOLA instantiation of csrc/gemm_split.hip, csrc/anchor_post.hip), written from the documented contract alone: numpy +
torch on the CPU, no call into ``desco_amd.ops`` or ``desco_amd.batch``.  Used by tests/test_pool_kernels_gpu.py (the
kernels against it) and by tests/test_pool_reference_host.py (the reference against a dense incidence-matrix formula,
known wrong slot decodes against the ceiling, and the gate against the kernels' restated arithmetic and a second fp32
summation order).

    slot layout   every (16-row tile t, segment b) pair in which segment b has a row in tile t, ordered by (t, b); the
                  position in that order is the pair's slot, one partial row [64] per slot and pooled layer
    reduce        out[b] = sum of segment b's partial rows + extra[b]
    pooled        block 0 = anch block 0 + rows(b) x0;  block l >= 1 = anch block l + sum of segment b's rows of parts[l-1]
    post          act(pooled W0^T + b0)                                     W0 [64, 64 (L + 1)]
    anchor_post   post with anch = act(a Wa^T + ba)                         Wa [64 (L + 1), k], k = 64 L or 64 (L + 1)

A *case* is a dict (``make(name)``): kind ("reduce", "post", "anchor"), layout, seg_ptr [B + 1] (int64 tensor; the post
kernels' cases end in one empty segment), seg_slots / num_slots / bits / slot (``slots_of``), parts (L tensors
[num_slots, 64]) and, by kind, extra | anch, x0, W0, b0, act, slope | a, Wa, ba, row_scale.  ``evaluate`` returns all B
rows in the dtype asked for: float64 is the reference, float32 the *fp32 evaluation* the kernels are held to (documented
orders: a segment's partial rows added in tile order from 0, one rounding per add; pooled = (((p0 + p1) + p2) + rows x0)
+ anchor; one matmul over K).  ``mag`` is the same evaluation on absolute operands without the activations: for the
anchor kernel the composed scale |W0| (|a| |Wa| + |ba| + sum |partials| + rows |x0|) + |b0| -- leaky and relu are
1-Lipschitz, so an error of the first stage enters the second at that scale.  ``emulate`` restates the kernels'
arithmetic (fp16 hi / lo anchor product with per-row power-of-two scales; the pooled operand and W0 split into three
truncated bf16 planes, the six retained products summed in fp32)."""
import functools

import numpy as np
import torch

from shmp_reference import scaled_error  # noqa: F401  (the figure every pool test reports)
from wide_reference import _pow2_scale, _split

TILE = 16
ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2          # the values of desco_amd.ops.ACT_*
SLOPE = 0.1


# ---- the slot layout --------------------------------------------------------------------------------------------------
def pairs_of(seg_ptr, num_rows, tile=TILE):
    """[(t, b, lo, hi)] in slot order: segment b owns rows [lo, hi) of tile t, hi > lo"""
    sp = [int(v) for v in seg_ptr]
    assert sp[0] == 0 and sp[-1] == num_rows and all(a <= b for a, b in zip(sp, sp[1:]))
    pairs = []
    for b in range(len(sp) - 1):
        r0, r1 = sp[b], sp[b + 1]
        for t in range(r0 // tile, (r1 - 1) // tile + 1) if r1 > r0 else ():
            pairs.append((t, b, max(r0, t * tile), min(r1, (t + 1) * tile)))
    pairs.sort(key=lambda p: (p[0], p[1]))
    return pairs


def slots_of(seg_ptr, num_rows, tile=TILE):
    """(per-segment list of slots in tile order, number of slots, (pool_bits uint32 [tiles], pool_slot int32 [tiles])):
    pool_bits has bit r of tile t set iff row t tile + r is the last row of a segment, pool_slot[t] is the tile's first
    slot -- read off the enumeration of the pairs, not through popcounts"""
    pairs = pairs_of(seg_ptr, num_rows, tile)
    B, nt = len(seg_ptr) - 1, (num_rows + tile - 1) // tile
    seg_slots = [[] for _ in range(B)]
    bits, slot = np.zeros(nt, np.uint32), np.full(nt, -1, np.int64)
    for s, (t, b, lo, hi) in enumerate(pairs):
        seg_slots[b].append(s)                                   # (t, b) order visits a segment's tiles in tile order
        if slot[t] < 0:
            slot[t] = s
        if hi == int(seg_ptr[b + 1]):
            bits[t] |= np.uint32(1) << np.uint32(hi - 1 - t * tile)
    assert (slot >= 0).all()                                     # every tile of [0, num_rows) holds a row of a segment
    return seg_slots, len(pairs), (bits, slot.astype(np.int32))


def slot_table(seg_slots):
    """[B, longest list] int64, -1 beyond a segment's slots"""
    width = max([len(s) for s in seg_slots] + [1])
    tab = np.full((len(seg_slots), width), -1, np.int64)
    for b, s in enumerate(seg_slots):
        tab[b, :len(s)] = s
    return torch.from_numpy(tab)


def tile_partials(rows, seg_ptr, dtype=torch.float64, absolute=False):
    """what a producer leaves: [num_slots, W], slot s = the sum of the rows of its (tile, segment) pair; float32: a
    running sum in row order from 0, one rounding per add"""
    pairs = pairs_of(seg_ptr, rows.shape[0])
    rows = rows.to(dtype).abs() if absolute else rows.to(dtype)
    lo, hi = torch.tensor([p[2] for p in pairs]), torch.tensor([p[3] for p in pairs])
    out = torch.zeros(len(pairs), rows.shape[1], dtype=dtype)
    for p in range(TILE):
        live = (lo + p < hi).nonzero().flatten()
        out[live] = out[live] + rows[lo[live] + p]
    return out


# ---- the formulas -----------------------------------------------------------------------------------------------------
def _conv(dtype, absolute):
    return (lambda t: t.to(dtype).abs()) if absolute else (lambda t: t.to(dtype))


def _act(z, act, slope):
    if act == ACT_RELU:
        return torch.relu(z)
    if act == ACT_LEAKY:
        return torch.where(z > 0, z, z * slope)
    assert act == ACT_NONE
    return z


def reduce(part, seg_slots, extra=None, dtype=torch.float64, absolute=False):
    """out[b] = sum of segment b's partial rows (tile order, from 0; float32: one rounding per add) + extra[b]"""
    conv = _conv(dtype, absolute)
    part, tab = conv(part), slot_table(seg_slots)
    out = torch.zeros(len(seg_slots), part.shape[1], dtype=dtype)
    for p in range(tab.shape[1]):
        live = (tab[:, p] >= 0).nonzero().flatten()
        out[live] = out[live] + part[tab[live, p]]
    return out if extra is None else out + conv(extra)


def _rows_of(case):
    return case["seg_ptr"][1:] - case["seg_ptr"][:-1]


def anchor(case, dtype=torch.float64, absolute=False):
    """the anchor rows [B, 64 (L + 1)]: given (kind "post") or act(a Wa^T + ba); ``absolute``: |a| |Wa|^T + |ba|"""
    conv = _conv(dtype, absolute)
    if case["kind"] == "post":
        return conv(case["anch"])
    z = conv(case["a"]) @ conv(case["Wa"]).t() + conv(case["ba"])
    return z if absolute else _act(z, case["act"], case["slope"])


def pooled(case, dtype=torch.float64, absolute=False, seg_slots=None, x0_term="block 0", anch=None):
    """[B, 64 (L + 1)]: (((p0 + p1) + p2) + rows x0) + anchor per 64-column block (x0 in block 0 only, partial rows in
    the blocks l >= 1 only).  ``seg_slots`` / ``x0_term`` ("none", "block 1") express known wrong forms."""
    conv = _conv(dtype, absolute)
    anch = anchor(case, dtype, absolute) if anch is None else anch
    if "draws" in case:                                          # the draws' rows one after the other
        ends = np.cumsum([len(d["seg_slots"]) for d in case["draws"]]).tolist()
        return torch.cat([pooled(d, dtype, absolute, None, x0_term, anch[e - len(d["seg_slots"]):e])
                          for d, e in zip(case["draws"], ends)])
    seg_slots = case["seg_slots"] if seg_slots is None else seg_slots
    B, L = anch.shape[0], len(case["parts"])
    rx = _rows_of(case).to(dtype)[:, None] * conv(case["x0"])[None, :]           # rounded on its own in float32
    zero = torch.zeros(B, 64, dtype=dtype)
    out = []
    for l in range(L + 1):
        s = reduce(case["parts"][l - 1], seg_slots, None, dtype, absolute) if l else zero
        s = s + (rx if x0_term == f"block {l}" else zero)
        out.append(s + anch[:, 64 * l:64 * (l + 1)])
    return torch.cat(out, 1)


def post(case, dtype=torch.float64, absolute=False, order="whole", **kw):
    """act(pooled W0^T + b0) [B, 64].  ``order``: "whole" (one matmul over K) or "blocks_reversed" (one matmul per
    64-column block, accumulated from the last block to the first)"""
    conv = _conv(dtype, absolute)
    p, W0 = pooled(case, dtype, absolute, **kw), conv(case["W0"])
    if order == "whole":
        z = p @ W0.t()
    else:
        assert order == "blocks_reversed"
        z = None
        for l in range(p.shape[1] // 64 - 1, -1, -1):
            t = p[:, 64 * l:64 * (l + 1)] @ W0[:, 64 * l:64 * (l + 1)].t()
            z = t if z is None else z + t
    if case["b0"] is not None:
        z = z + conv(case["b0"])
    return z if absolute else _act(z, case["act"], case["slope"])


anchor_post = post          # the anchor kernel's contract: ``post`` of a case whose anchor rows are act(a Wa^T + ba)


def evaluate(case, dtype=torch.float64, absolute=False, order="whole", layer=0, **kw):
    """all B rows of a case (of every draw of it, one after the other): ``reduce`` of its partial array ``layer`` (kind
    "reduce"), ``post`` otherwise"""
    if case["kind"] == "reduce":
        return reduce(case["parts"][layer], kw.get("seg_slots", case["seg_slots"]), case["extra"], dtype, absolute)
    return post(case, dtype, absolute, order, **kw)


def mag(case, layer=0):
    return evaluate(case, torch.float64, absolute=True, layer=layer)


# ---- the kernels' arithmetic, restated ----------------------------------------------------------------------------------
def _trunc_bf16x3(v):
    """v (float32) = hi + mid + lo + (less than 2^-24 of it): three bf16 values by truncation, as float32 arrays"""
    def top(a):
        return (a.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    v = np.ascontiguousarray(v, np.float32)
    hi = top(v)
    r1 = v - hi
    mid = top(r1)
    return hi, mid, top(r1 - mid)


def emulate_anchor_f16x3(case):
    """gemm_f16x3's arithmetic on the host -> [B, 64 (L + 1)] float32: every row of ``a`` scaled by the power of two of
    its ``row_scale`` and split into fp16 hi / lo, Wa by one power of two per matrix; lo hi, hi lo, hi hi accumulated
    in fp32 per 32-wide K step; the scales undone, bias, activation.  (The sum inside a step is numpy's.)"""
    f32 = np.float32
    a, Wa, ba = (case[k].numpy().astype(f32) for k in ("a", "Wa", "ba"))
    ws = _pow2_scale(np.abs(Wa).max().astype(f32))
    wh, wl = _split(Wa * ws)
    sc = _pow2_scale(case["row_scale"].numpy().astype(f32))
    ah, al = _split(a * sc[:, None])
    acc = np.zeros((a.shape[0], Wa.shape[0]), f32)
    for k in range(0, a.shape[1], 32):
        acc = acc + al[:, k:k + 32] @ wh[:, k:k + 32].T
        acc = acc + ah[:, k:k + 32] @ wl[:, k:k + 32].T
        acc = acc + ah[:, k:k + 32] @ wh[:, k:k + 32].T
    z = acc * ((f32(1) / sc) * (f32(1) / ws))[:, None] + ba
    return _act(torch.from_numpy(z), case["act"], case["slope"])


def emulate_post_bf16x6(case, anch=None):
    """the POOLA product on the host -> [B, 64] float32: the pooled operand formed in float32 in the documented order,
    it and W0 split into three truncated bf16 planes, per 16-wide K step lo hi, hi lo, mid mid, mid hi, hi mid, hi hi
    added to an fp32 accumulator; bias, activation"""
    f32 = np.float32
    p = pooled(case, torch.float32, anch=anch).numpy()
    ph, pm, pl = _trunc_bf16x3(p)
    wh, wm, wl = _trunc_bf16x3(case["W0"].numpy())
    acc = np.zeros((p.shape[0], 64), f32)
    for k in range(0, p.shape[1], 16):
        s = slice(k, k + 16)
        for x, w in ((pl, wh), (ph, wl), (pm, wm), (pm, wh), (ph, wm), (ph, wh)):
            acc = acc + x[:, s] @ w[:, s].T
    if case["b0"] is not None:
        acc = acc + case["b0"].numpy().astype(f32)
    return _act(torch.from_numpy(acc), case["act"], case["slope"])


def emulate(case):
    if case["kind"] == "reduce":
        return evaluate(case, torch.float32)
    return emulate_post_bf16x6(case, emulate_anchor_f16x3(case) if case["kind"] == "anchor" else None)


# ---- the segment layouts ------------------------------------------------------------------------------------------------
SWEEP_MAX = 33
LONG = [1, 1000, 16, 17, 3000, 5, 48]
LAYOUTS = ("sweep33", "ones", "ragged", "single33", "single1", "long")
POST_LAYOUTS = LAYOUTS[:-1]                      # the post kernels read at most three tiles per segment


def layout(name):
    """segment lengths (all >= 1) -> int64 array.
      sweep33   for every length n in 1..33 and start offset f in 0..15 one segment of n rows that begins at a row = f
                (mod 16), each reached by a filler segment of 1..16 rows before it; the (n, f) pairs in random order
      ones      300 one-row segments: full tiles have all 16 bits set
      ragged    lengths 1..33 at random; the last segment starts at offset 9 of a tile and has 12 rows: the last tile
                is partial (5 rows) and all of it belongs to a segment carried in from the tile before
      single33, single1   one segment
      long      LONG: segments of up to 3000 rows (189 tiles)"""
    rng = np.random.default_rng(LAYOUTS.index(name))
    if name == "sweep33":
        lens, cur = [], 0
        pairs = [(n, f) for n in range(1, SWEEP_MAX + 1) for f in range(TILE)]
        for i in rng.permutation(len(pairs)):
            n, f = pairs[i]
            fill = (f - cur) % TILE or TILE
            lens += [fill, n]
            cur += fill + n
    elif name == "ones":
        lens = [1] * 300
    elif name == "ragged":
        lens = rng.integers(1, SWEEP_MAX + 1, 60).tolist()
        lens += [(9 - sum(lens)) % TILE or TILE, 12]
    elif name == "long":
        lens = list(LONG)
    else:
        lens = [{"single33": 33, "single1": 1}[name]]
    return np.asarray(lens, np.int64)


def seg_ptr_of(lens, trailing_empty=False):
    sp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return np.concatenate([sp, sp[-1:]]) if trailing_empty else sp


# ---- the cases ----------------------------------------------------------------------------------------------------------
REGIMES = ("o1", "rows_pm16", "zeros", "cancel")
POST_L, ANCHOR_L = (1, 3, 8), (2, 5, 8)
M_VALUES = (1, 127, 128, 129)                    # launches on prefixes of a case, and on all B rows
MULTI_LAYERS = (1, 8, 11)


@functools.lru_cache(maxsize=None)
def _layout_index(layout_name, trailing_empty):
    """(seg_ptr, slots_of(seg_ptr)) of a layout, computed once and shared by its cases (which leave it unchanged)"""
    sp = seg_ptr_of(layout(layout_name), trailing_empty)
    return sp, slots_of(sp, int(sp[-1]))


def _base(layout_name, L, seed, trailing_empty):
    g = torch.Generator().manual_seed(7000 + seed)
    sp, (seg_slots, ns, (bits, slot)) = _layout_index(layout_name, trailing_empty)
    case = dict(layout=layout_name, seg_ptr=torch.from_numpy(sp), seg_slots=seg_slots, num_slots=ns, bits=bits, slot=slot,
                parts=[torch.randn(ns, 64, generator=g) for _ in range(L)])
    return case, g


def reduce_case(layout_name, extra, layers=1, seed=0):
    """pool_reduce / pool_reduce_multi: ``layers`` random partial arrays (``evaluate`` is layer 0's), extra [B, 64]"""
    case, g = _base(layout_name, layers, seed, False)
    B = len(case["seg_slots"])
    case.update(kind="reduce", extra=torch.randn(B, 64, generator=g) if extra else None)
    return case


SINGLE_DRAWS = 32


def draws_of(case):
    return case.get("draws", [case])


def post_case(kind, layout_name, L, regime="o1", act=ACT_LEAKY, bias=True, k_blocks=None, seed=0):
    """``_post_draw``; on the single-segment layouts SINGLE_DRAWS draws of it under "draws": problems of their own with
    B = 1 (+ the empty segment), each launched on its own by the GPU test, with the weights, biases and x0 in common.
    The case itself holds the draws' ``a`` (``anch``) rows one after the other, so that its float32 evaluation is one
    matmul over K on all of them, like every other case's.  Why: E_f32 is a maximum over the elements of the case, and
    the float32 evaluation has to be the same arithmetic on every case.  Over the 128 elements of one draw the maximum
    scatters by a factor of 5 between seeds, and torch's CPU matmul (MKL) of 4 rows and fewer takes a path of its own
    that is 2.3 times as accurate as the one all larger products take (measured mean |error| / mag 6.3e-9 against
    1.5e-8 at K = 576, the same from 8 rows to 1 057): held to one draw's figure the kernels' documented arithmetic
    (``emulate``) itself misses 4 E_f32 on a quarter of the seeds."""
    if not layout_name.startswith("single"):
        return _post_draw(kind, layout_name, L, regime, act, bias, k_blocks, seed, seed)
    draws = [_post_draw(kind, layout_name, L, regime, act, bias, k_blocks, 1000 * (seed + 1) + i, seed)
             for i in range(SINGLE_DRAWS)]
    case = {k: v for k, v in draws[0].items() if k in ("kind", "layout", "regime", "act", "slope", "x0", "W0", "b0", "Wa", "ba")}
    for k in ("a", "anch", "row_scale"):
        if k in draws[0]:
            case[k] = torch.cat([d[k] for d in draws])
    return dict(case, draws=draws)


def _post_draw(kind, layout_name, L, regime, act, bias, k_blocks, seed, wseed):
    """One case of pool_post (kind "post": anch [B, 64 (L + 1)] given) or anchor_pool_post (kind "anchor": a [B, 64
    k_blocks], k_blocks = L or L + 1).  ``regime``:
      o1         operands of order 1, partial rows of mixed sign
      rows_pm16  the rows of a (of anch) scaled by 2^randint(-16, 16); row_scale is their true absmax
      zeros      30 % of the rows of a (of anch) all zero with row_scale 0, their segments' partial rows 0, x0 = 0,
                 ba = 0, no b0: mag == 0 on those rows
      cancel     the partial rows of every segment of two or three tiles cancel to 2^-12 of their size"""
    assert regime in REGIMES and kind in ("post", "anchor")
    case, g = _base(layout_name, L, seed, True)
    B, n = len(case["seg_slots"]), 64 * (L + 1)
    k = n if kind == "post" else 64 * k_blocks
    a = torch.randn(B, k, generator=g)
    gw = torch.Generator().manual_seed(9000 + wseed)             # (the draws of a case have these in common)
    x0 = torch.randn(64, generator=gw) / 2
    W0 = torch.randn(64, n, generator=gw) / np.sqrt(n)
    b0 = torch.randn(64, generator=gw) / 4 if bias else None
    Wa = torch.randn(n, k, generator=gw) / np.sqrt(k)
    ba = torch.randn(n, generator=gw) / 4
    zero_rows = []
    if regime == "rows_pm16":
        a = a * 2.0 ** torch.randint(-16, 17, (B, 1), generator=g).float()
    elif regime == "zeros":
        z = torch.rand(B, generator=g) < 0.3
        z[0], z[-1] = True, False                                # (the one-row launch and the B = 2 cases see both kinds)
        a[z] = 0
        for b in z.nonzero().flatten().tolist():
            for p in case["parts"]:
                p[case["seg_slots"][b]] = 0
        x0, ba, b0 = torch.zeros(64), torch.zeros(n), None
        zero_rows = z.nonzero().flatten().tolist()
    elif regime == "cancel":
        for s in case["seg_slots"]:
            if len(s) > 1:
                for p in case["parts"]:
                    size = p[s[:-1]].abs().sum(0)
                    p[s[-1]] = -p[s[:-1]].sum(0) + 2.0 ** -12 * size * (1 - 2 * torch.randint(0, 2, (64,), generator=g))
    case.update(kind=kind, regime=regime, act=act, slope=SLOPE if act == ACT_LEAKY else 0.0, x0=x0, W0=W0, b0=b0,
                zero_rows=zero_rows)
    if kind == "post":
        case.update(anch=a)
    else:
        case.update(a=a, Wa=Wa, ba=ba, row_scale=a.abs().amax(1))
    return case


# name -> (builder, arguments); tests/test_pool_kernels_gpu.py runs every one, tests/test_pool_reference_host.py proves each
# one's gate reachable.  Per kernel and L: sweep33 with every regime and every (activation, bias) setting, the other
# layouts with every regime (the activation and bias settings going round).
CASES = {}
_ACT_NAME = {ACT_NONE: "none", ACT_RELU: "relu", ACT_LEAKY: "leaky"}
_SETTINGS = [(ACT_LEAKY, True), (ACT_RELU, False), (ACT_NONE, False), (ACT_NONE, True), (ACT_RELU, True), (ACT_LEAKY, False)]


def _add(name, fn, **kw):
    assert name not in CASES
    CASES[name] = (fn, dict(kw, seed=len(CASES)))


for _lay in LAYOUTS:
    for _ex in (False, True):
        _add(f"reduce {_lay}{' extra' if _ex else ''}", reduce_case, layout_name=_lay, extra=_ex)
for _n in MULTI_LAYERS:
    _add(f"multi {_n} layers sweep33", reduce_case, layout_name="sweep33", extra=True, layers=_n)


def _add_post(kind, L, k_blocks=None):
    tag = f"{kind} L {L}" + (f" k {64 * k_blocks}" if k_blocks else "")
    plan = list(zip(["sweep33"] * 6, ("o1", "rows_pm16", "zeros", "cancel", "o1", "o1"), _SETTINGS))
    i = 0
    for lay in POST_LAYOUTS[1:]:
        for reg in REGIMES:
            plan.append((lay, reg, _SETTINGS[i % 6]))
            i += 5                                               # (5 and 6 are coprime: every setting comes round)
    for lay, reg, (act, bias) in plan:
        bias = bias and reg != "zeros"
        _add(f"{tag} {lay} {reg} {_ACT_NAME[act]}{' bias' if bias else ''}", post_case, kind=kind, layout_name=lay, L=L,
             regime=reg, act=act, bias=bias, k_blocks=k_blocks)


for _L in POST_L:
    _add_post("post", _L)
for _L in ANCHOR_L:
    for _kb in (_L, _L + 1):
        _add_post("anchor", _L, _kb)


for _n in MULTI_LAYERS:                          # (added last: a case's seed is its position)
    _add(f"multi {_n} layers sweep33 no extra", reduce_case, layout_name="sweep33", extra=False, layers=_n)


def make(name):
    fn, kw = CASES[name]
    return fn(**kw)


def family(word):
    return [n for n in CASES if n.split()[0] == word]
