"""The fused-pooling family -- the consumers pool_reduce / pool_reduce_multi (csrc/graph_ops.hip), pool_post (the POOLA
instantiation of csrc/gemm_split.hip) and anchor_pool_post (csrc/anchor_post.hip), and the partial rows the producers
leave (shmp_layer(pool=...) in its bf16x6 and f16x3 forms, degree_affine_pool) -- per element against the fp64 host
reference tests/pool_reference.py.

Gate (that of tests/test_wide_kernels_gpu.py; no number of its own): per launch E_kernel = max |got - ref| / mag over ALL
elements the launch computes, mag = the reference evaluated on absolute values (the sum of |terms| of the element).
E_kernel <= 4 E_f32, where E_f32 is the same figure of the reference evaluated in float32 on the host over all rows of
the case (a launch on a prefix of the case, or on one draw of a single-segment case, is held to the figure of the whole
case), and E_kernel <= 1e-4.  An element with mag == 0 must be exactly 0.  tests/test_pool_reference_host.py proves the
gate reachable on every case below.  Every launch prints E_kernel, E_f32 and their ratio as ``[parity]`` lines; the worst
ratio per family is printed once more when the module ends.

The consumers read random partial arrays [num_slots, 64]: the slot layout (pool_reference.slots_of, which the host test
holds against NeighborhoodBatch.pool_index), not a producer, is what they are tested on.  Every launch runs twice
(bit-identical); outputs live in NaN-filled parents and nothing outside the rows and columns a launch owns is written."""
import collections
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pool_reference as P  # noqa: E402
from desco_amd import ops  # noqa: E402

DEV = "cuda"
CEILING = 1e-4
NAN = float("nan")
WORST = collections.defaultdict(float)          # family -> worst E_kernel / E_f32 seen
PLACEMENTS = ("contiguous", "ldo 68", "one float in")


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    for k in sorted(WORST):
        print(f"[parity] pool worst E_kernel / E_f32 over the module, {k}: {WORST[k]:.2f} (gate 4)")


def _gate(name, family, got, ref, mag, ef):
    """E_kernel <= 4 E_f32 (``ef``: the figure of the whole case) and <= CEILING; zero where mag is zero"""
    g = got.detach().cpu().double().reshape(ref.shape)
    ek, i = P.scaled_error(g, ref, mag)
    ratio = ek / ef if ef > 0 else (0.0 if ek == 0 else float("inf"))
    WORST[family] = max(WORST[family], ratio)
    print(f"[parity] {family}, {name}: E_kernel {ek:.3e}, E_f32 {ef:.3e}, ratio {ratio:.2f} (gate 4, ceiling {CEILING:.0e})")
    exact = bool((g[mag == 0] == 0).all())
    assert ek <= 4 * ef and ek <= CEILING and exact, (
        f"{family}, {name}: E_kernel {ek:.3e} E_f32 {ef:.3e} ratio {ratio:.2f}; element {i} (row {i // 64}, column {i % 64}): "
        f"got {float(g.flatten()[i])!r}, ref {float(ref.flatten()[i])!r}, mag {float(mag.flatten()[i])!r}"
        f"{'' if exact else '; nonzero where mag == 0'}")


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _all_nan(t):
    return bool(torch.isnan(t).all())


@functools.lru_cache(maxsize=None)
def _host(name):
    """(case, fp64 reference, mag, fp32 evaluation, E_f32) of a named case, computed once for the module"""
    case = P.make(name)
    ref, m, f32 = P.evaluate(case), P.mag(case), P.evaluate(case, torch.float32)
    return case, ref, m, f32, P.scaled_error(f32, ref, m)[0]


def _index(case):
    """(pool_bits, pool_slot, seg_ptr) of a case on the device"""
    return (torch.from_numpy(case["bits"].view(np.int32)).to(DEV), torch.from_numpy(case["slot"]).to(DEV),
            case["seg_ptr"].to(torch.int32).to(DEV))


def _column_block(t, lead, tail=4):
    """``t`` as a column block of a NaN-filled parent [rows, lead + width + tail] (lead a multiple of 4: 16-byte rows)"""
    parent = torch.full((t.shape[0], lead + t.shape[1] + tail), NAN)
    parent[:, lead:lead + t.shape[1]] = t
    parent = parent.to(DEV)
    view = parent[:, lead:lead + t.shape[1]]
    assert view.data_ptr() % 16 == 0 and view.stride(0) % 4 == 0
    return view, parent


# ---- pool_reduce, pool_reduce_multi -------------------------------------------------------------------------------------
def _reduce_once(case, layer_ids, multi):
    B = len(case["seg_slots"])
    bits, slot, seg = _index(case)
    n = len(layer_ids)
    parts = [case["parts"][l].to(DEV) for l in layer_ids]
    extras = [None] * n
    if case["extra"] is not None:
        ext, _ = _column_block(case["extra"].repeat(1, n), 68)
        extras = [ext[:, 64 * i:64 * (i + 1)] for i in range(n)]
    parent = torch.full((B + 2, 64 * n + 72), NAN, device=DEV)
    outs = [parent[1:B + 1, 4 + 64 * i:68 + 64 * i] for i in range(n)]
    if multi:
        ops.pool_reduce_multi(parts, bits, slot, seg, B, extras, outs)
    else:
        got = ops.pool_reduce(parts[0], bits, slot, seg, B, extra=extras[0], out=outs[0])
        assert got.data_ptr() == outs[0].data_ptr()
    assert _all_nan(parent[0]) and _all_nan(parent[-1]) and _all_nan(parent[:, :4]) and _all_nan(parent[:, 4 + 64 * n:])
    return torch.stack([o.clone() for o in outs])


@pytest.mark.parametrize("name", P.family("reduce"))
def test_pool_reduce_is_the_fp32_sum_in_tile_order(name):
    """every layout (sweep33: every length 1..33 at every start offset; ones: 16 ends per tile; ragged: a partial last
    tile; one segment of 33 rows and of 1 row; segments of up to 189 tiles), with and without ``extra``; ``out`` and
    ``extra`` column blocks of NaN-filled parents: bit-identical to the float32 sum in tile order, within the gate of
    the fp64 sum, nothing else written"""
    case, ref, m, f32, ef = _host(name)
    got = _reduce_once(case, [0], False)[0]
    assert _same_bits(got, _reduce_once(case, [0], False)[0]), f"{name}: two launches on the same inputs differ"
    _gate(name, "pool_reduce", got, ref, m, ef)
    assert _same_bits(got.cpu(), f32), f"{name}: not the float32 sum in tile order"


@pytest.mark.parametrize("name", P.family("multi"))
def test_pool_reduce_multi_is_the_fp32_sum_per_layer(name):
    """1, 8 and 11 layers (one group, a full group, two groups) on sweep33, with and without ``extra``: every layer
    bit-identical to the float32 sum in tile order and within the gate"""
    case = _host(name)[0]
    ids = list(range(len(case["parts"])))
    got = _reduce_once(case, ids, True)
    assert _same_bits(got, _reduce_once(case, ids, True)), f"{name}: two launches on the same inputs differ"
    for l in ids:
        ref, m, f32 = P.evaluate(case, layer=l), P.mag(case, layer=l), P.evaluate(case, torch.float32, layer=l)
        _gate(f"{name}, layer {l}", "pool_reduce_multi", got[l], ref, m, P.scaled_error(f32, ref, m)[0])
        assert _same_bits(got[l].cpu(), f32), f"{name}, layer {l}: not the float32 sum in tile order"


# ---- pool_post, anchor_pool_post ------------------------------------------------------------------------------------------
def _weights(case):
    w = dict(w0=ops.split_bf16_planes(case["W0"].to(DEV)), b0=None if case["b0"] is None else case["b0"].to(DEV),
             x0=case["x0"].to(DEV))
    if case["kind"] == "anchor":
        w.update(wa=ops.split_f16_planes(case["Wa"].to(DEV)), ba=case["ba"].to(DEV))
    return w


def _operands(d):
    """one draw's operands on the device: the index, the partial arrays, ``anch`` as a strided view (lda = n + 8) or
    ``a`` as the column view parent[:, 64:] the model passes, and its row bounds"""
    o = dict(index=_index(d), parts=[p.to(DEV) for p in d["parts"]])
    if d["kind"] == "post":
        o["anch"], o["parent"] = _column_block(d["anch"], 4)
        assert o["anch"].stride(0) > d["anch"].shape[1]
    else:
        o["a"], o["parent"] = _column_block(d["a"], 64, 0)
        o["row_scale"] = d["row_scale"].to(DEV)
    return o


def _call(case, w, o, m, out=None):
    bits, slot, seg = o["index"]
    if case["kind"] == "post":
        return ops.pool_post(o["anch"][:m], o["parts"], bits, slot, seg, w["x0"], w["w0"], w["b0"], case["act"],
                             case["slope"], out=out)
    return ops.anchor_pool_post(o["a"][:m], w["wa"], w["ba"], o["row_scale"][:m], o["parts"], bits, slot, seg, w["x0"],
                                w["w0"], w["b0"], case["act"], case["slope"], out=out)


def _placed(case, w, o, m, placement):
    """one launch on rows [0, m) into ``out`` placed as asked -> its rows; nothing but them was written"""
    if placement == "contiguous":
        parent = out = torch.full((m, 64), NAN, device=DEV)
    else:
        parent = torch.full((m + 2, 68), NAN, device=DEV)
        c = 0 if placement == "ldo 68" else 1
        out = parent[1:m + 1, c:c + 64]
        assert out.data_ptr() % 16 == 4 * c
    got = _call(case, w, o, m, out)
    assert got.data_ptr() == out.data_ptr()
    rows = out.clone()
    assert not torch.isnan(rows).any(), f"{placement}: an element was not written (or is NaN)"
    if parent is not out:
        out.fill_(NAN)
        assert _all_nan(parent), f"{placement}: written outside rows [0, {m}) x 64 columns"
    return rows


def _run_post(name, family):
    case, ref, mg, _, ef = _host(name)
    w = _weights(case)
    row = 0
    for di, d in enumerate(P.draws_of(case)):
        B = len(d["seg_slots"])
        o = _operands(d)
        for m in sorted({min(v, B) for v in P.M_VALUES} | {B}):
            tag = f"{name}, m {m}" + (f", draw {di}" if "draws" in case else "")
            got = _placed(d, w, o, m, "contiguous")
            assert _same_bits(got, _placed(d, w, o, m, "contiguous")), f"{tag}: two launches on the same inputs differ"
            for placement in PLACEMENTS[1:] if di == 0 else ():
                assert _same_bits(got, _placed(d, w, o, m, placement)), f"{tag}: ``out`` {placement} changes bits"
            _gate(tag, family, got, ref[row:row + m], mg[row:row + m], ef)
            if d["kind"] == "anchor":
                bits, slot, seg = o["index"]
                anch = ops.gemm_f16x3(o["a"][:m], w["wa"], w["ba"], act=d["act"], slope=d["slope"], row_scale=o["row_scale"][:m])
                two = ops.pool_post(anch, o["parts"], bits, slot, seg, w["x0"], w["w0"], w["b0"], d["act"], d["slope"])
                assert _same_bits(got, two), f"{tag}: not the bits of gemm_f16x3 + pool_post"
        if d["kind"] == "anchor":
            assert _all_nan(o["parent"][:, :64])
        row += B


@pytest.mark.parametrize("name", P.family("post"))
def test_pool_post_matches_the_reference(name):
    """L in {1, 3, 8}; every layout with every magnitude regime; NONE / RELU / LEAKY 0.1, with and without a bias;
    ``anch`` a strided view; m in {1, 127, 128, 129, B} as prefixes of one case (the single-segment cases: every draw on
    its own, m in {1, 2}); ``out`` contiguous, with ldo = 68 and one float into a NaN-filled parent: the same bits"""
    _run_post(name, "pool_post")


@pytest.mark.parametrize("name", P.family("anchor"))
def test_anchor_pool_post_matches_the_reference(name):
    """L in {2, 5, 8} with k = 64 L and k = 64 (L + 1); ``a`` the column view parent[:, 64:]; the layouts, regimes,
    activations, bias settings, m values and ``out`` placements of pool_post; every launch bit-identical to
    gemm_f16x3 + pool_post on the same arguments"""
    _run_post(name, "anchor_pool_post")


# ---- the producers' partial rows ------------------------------------------------------------------------------------------
def _random_vcsr(num_rows, slots, max_deg, n_src, g):
    cnt = torch.randint(0, max_deg + 1, (num_rows * slots,), generator=g)
    cnt[::7] = 0
    ptr = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(cnt, 0)])
    col = torch.randint(0, n_src, (int(ptr[-1]),), generator=g)
    return ptr.to(torch.int32), col.to(torch.int32), cnt


def _layer_launches(form, N, g):
    """(plain launch -> rows, pooled launch (out, part) -> None) of one producer on N rows"""
    S = 4
    if form == "degree_affine":
        ptr = _random_vcsr(N, S, 3, N, g)[0].to(DEV)
        coef = (torch.randn(S + 1, 64, generator=g) / 4).to(DEV)
        return (lambda out: ops.degree_affine(ptr, 0, N, S, coef, ops.ACT_RELU, 0.0, out),
                lambda out, pool: ops.degree_affine_pool(ptr, N, S, coef, ops.ACT_RELU, 0.0, out, pool))
    sm, n_tab = 2, 50
    x = torch.randn(N + n_tab, 64, generator=g)
    ptr, col, cnt = _random_vcsr(N + n_tab, S, 3, N, g)
    vrow = torch.repeat_interleave(torch.arange((N + n_tab) * S), cnt)
    col = torch.where((vrow % S) >= sm, N + col % n_tab, col % N).to(torch.int32)      # table slots read the table rows
    wt = torch.randn(3 * 64, 64, generator=g) / 12
    bias = torch.randn(64, generator=g).to(DEV)
    split = ops.split_bf16_planes if form == "bf16x6" else ops.split_f16_planes
    planes = split(wt.t().contiguous().to(DEV))
    ytab = torch.randn(n_tab, 128, generator=g).to(DEV)
    xd, ptrd, cold = x.to(DEV), ptr.to(DEV), col.to(DEV)

    def run(out, pool=None):
        ops.shmp_layer(xd, ptrd, cold, 0, N, S, sm, planes, bias, out, ytab=ytab, ytab_row0=N, pool=pool)
    return run, run


@pytest.mark.parametrize("layout", ["sweep33", "ones", "ragged"])
@pytest.mark.parametrize("form", ["bf16x6", "f16x3", "degree_affine"])
def test_producers_leave_the_tile_sums_of_their_rows(form, layout):
    """shmp_layer(pool=...) in its bf16x6 and f16x3 forms and degree_affine_pool on a small random virtual CSR: with
    ``out`` stored the rows are those of the plain launch bit for bit, every slot of the NaN-filled partial array (and
    nothing behind it) is written, and each partial row is the fp64 sum of the stored rows of its (tile, segment) pair
    within the gate (E_f32: their float32 sum in row order); with ``out`` None the partial rows have the same bits"""
    sp = P.seg_ptr_of(P.layout(layout))
    N = int(sp[-1])
    _, ns, (bits, slot) = P.slots_of(sp, N)
    bits, slot = torch.from_numpy(bits.view(np.int32)).to(DEV), torch.from_numpy(slot).to(DEV)
    plain_fn, pool_fn = _layer_launches(form, N, torch.Generator().manual_seed(len(form) + len(layout)))
    plain = torch.full((N, 64), NAN, device=DEV)
    plain_fn(plain)
    assert not torch.isnan(plain).any()
    parts = []
    for store in (True, False, True):
        buf = torch.full((ns + 1, 64), NAN, device=DEV)
        out = torch.full((N, 64), -7.0, device=DEV) if store else None
        pool_fn(out, (bits, slot, buf[:ns]))
        assert not torch.isnan(buf[:ns]).any(), f"{form}, {layout}: a slot was not written"
        assert _all_nan(buf[ns:]), f"{form}, {layout}: written behind the last slot"
        assert out is None or _same_bits(out, plain), f"{form}, {layout}: the stored rows are not the plain launch's"
        parts.append(buf[:ns].clone())
    assert _same_bits(parts[0], parts[1]), f"{form}, {layout}: the partial rows depend on ``out``"
    assert _same_bits(parts[0], parts[2]), f"{form}, {layout}: two launches on the same inputs differ"
    rows = plain.cpu()
    ref, m, f32 = P.tile_partials(rows, sp), P.tile_partials(rows, sp, absolute=True), P.tile_partials(rows, sp, torch.float32)
    _gate(f"{form}, {layout}", f"producer {form}", parts[0], ref, m, P.scaled_error(f32, ref, m)[0])
