"""The fused plain-layer kernel (csrc/plain_layer.hip, desco_plain_layer_f16x3_f32 through ops.plain_layer) per element
against the fp64 host reference tests/plain_kernel_reference.py.

Gate (that of tests/test_wide_kernels_gpu.py; no number of its own): per launch E_kernel = max |got - ref| / mag over ALL
elements the launch computes, mag = the reference evaluated on absolute values (|z| |W1| + |b1|, pushed without the relu
through |W2|, |b2| for two products).  E_kernel <= 4 E_f32, where E_f32 is the same figure of the reference evaluated
in float32 on the host, and E_kernel <= 1e-4.  An element with mag == 0 must be exactly 0.  Every test prints E_kernel,
E_f32 and their ratio as ``[parity]`` lines; the worst ratio per family is printed once more when the module ends.

Every case runs the kernel twice (bit-identical) and checks that nothing outside the rows and columns it owns was written
(NaN-filled parents of out, out2 and x).  Against the un-fused composition (csr_gather_sum_wide with slots = 1, the
eps x term, gemm_f16x3 once or twice): both forms scale a row by the power of two of its maximum over the whole width,
but they do NOT coincide by construction -- gemm_f16x3 accumulates 16-wide K steps on v_mfma_f32_32x32x16_f16, the fused
kernel 32-wide K steps on v_mfma_f32_16x16x32_f16, so the fp32 sums are formed in another order -- and the composition
is therefore held to the same reference within the same gate, not bit for bit."""
import collections
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import plain_kernel_reference as P  # noqa: E402
from desco_amd import _lib, ops  # noqa: E402

DEV = "cuda"
CEILING = 1e-4
NAN = float("nan")
WORST = collections.defaultdict(float)


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    for k in sorted(WORST):
        print(f"[parity] plain worst E_kernel / E_f32 over the module, {k}: {WORST[k]:.2f} (gate 4)")


def _gate(name, family, got, ref, mag, f32):
    g = got.detach().cpu().double().reshape(ref.shape)
    ek, i = P.scaled_error(g, ref, mag)
    ef, _ = P.scaled_error(f32, ref, mag)
    ratio = ek / ef if ef > 0 else (0.0 if ek == 0 else float("inf"))
    WORST[family] = max(WORST[family], ratio)
    print(f"[parity] {family}, {name}: E_kernel {ek:.3e}, E_f32 {ef:.3e}, ratio {ratio:.2f} (gate 4, ceiling {CEILING:.0e})")
    exact = bool((g[mag == 0] == 0).all())
    nc = max(ref.shape[-1], 1)
    assert ek <= 4 * ef and ek <= CEILING and exact, (
        f"{family}, {name}: E_kernel {ek:.3e} E_f32 {ef:.3e} ratio {ratio:.2f}; element {i} (row {i // nc}, column "
        f"{i % nc}): got {float(g.flatten()[i])!r}, ref {float(ref.flatten()[i])!r}, mag {float(mag.flatten()[i])!r}"
        f"{'' if exact else '; nonzero where mag == 0'}")


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _all_nan(t):
    return bool(torch.isnan(t).all())


def _i32(t):
    return t.to(torch.int32).to(DEV)


@functools.lru_cache(maxsize=None)
def _host(name):
    """(case, fp64 reference, mag, fp32 evaluation) of a named case, computed once for the module"""
    case = P.make(name)
    return case, P.evaluate(case), P.mag(case), P.evaluate(case, torch.float32)


@functools.lru_cache(maxsize=None)
def _device(name):
    """x (a 16-byte-aligned column view of a NaN-filled parent with ldx = Wp + 12, or contiguous), its parent, the index,
    the weight planes of W1.T / W2.T, the biases, the self scale as a device scalar"""
    case = _host(name)[0]
    x = case["x"]
    N, wp = x.shape
    if case["x_strided"]:
        parent = torch.full((N, wp + 12), NAN)
        parent[:, 8:8 + wp] = x
        parent = parent.to(DEV)
        xd = parent[:, 8:8 + wp]
        assert xd.stride(0) > wp and xd.data_ptr() % 16 == 0
    else:
        parent = xd = x.to(DEV)
    w1 = ops.split_f16_planes(case["W1"].t().contiguous().to(DEV))
    w2 = None if case["W2"] is None else ops.split_f16_planes(case["W2"].t().contiguous().to(DEV))
    b2 = None if case["b2"] is None else case["b2"].to(DEV)
    s = None if case["s"] is None else torch.tensor([case["s"]], device=DEV)
    return xd, parent, _i32(case["rowptr"]), _i32(case["col"]), w1, case["b1"].to(DEV), w2, b2, s


def _fused(name, row0, num_rows, mode, out=None, out2_row0=None):
    """one launch on rows [row0, row0 + num_rows) -> the rows it produced [num_rows, Wp] (taken from ``out`` where it is
    given, else from out2, whose range then has to cover the launch's)"""
    case = _host(name)[0]
    xd, parent, rowptr, col, w1, b1, w2, b2, s = _device(name)
    N, wp = xd.shape
    o2r0 = row0 if out2_row0 is None else out2_row0
    assert row0 <= o2r0 < row0 + num_rows or num_rows == 0
    fresh = out is None
    if fresh:
        out = torch.full((N, wp), NAN, device=DEV)
    n2 = row0 + num_rows - o2r0
    buf2 = torch.full((n2, 3 * wp + 7), NAN, device=DEV)
    out2 = buf2[:, wp + 5:2 * wp + 5]                            # a column block that starts at no multiple of 4
    ops.plain_layer(xd, rowptr, col, row0, num_rows, w1, b1, w2, b2, self_scale=s,
                    out=out if mode in ("out", "both") else None, out2=out2 if mode in ("out2", "both") else None,
                    out2_row0=o2r0)
    rows = out[row0:row0 + num_rows]
    if mode == "out2":
        assert _all_nan(out), f"{name}: out was not given and was written"
    elif fresh:
        assert _all_nan(out[:row0]) and _all_nan(out[row0 + num_rows:]), f"{name}: rows outside the range were written"
    if mode == "out":
        assert _all_nan(buf2), f"{name}: out2 was not given and was written"
    else:
        assert _all_nan(buf2[:, :wp + 5]) and _all_nan(buf2[:, 2 * wp + 5:]), f"{name}: out2 written outside its block"
        assert not torch.isnan(out2).any(), f"{name}: a row of out2 was not written"
        if mode == "both":
            assert _same_bits(rows[o2r0 - row0:], out2), f"{name}: out and out2 differ"
    if mode != "out2":
        assert not torch.isnan(rows).any(), f"{name}: an element of the range was not written (or is NaN)"
    if case["x_strided"]:
        assert _all_nan(parent[:, :8]) and _all_nan(parent[:, 8 + wp:]) and _same_bits(xd, case["x"].to(DEV))
    return (out2 if mode == "out2" else rows).clone()


def _unfused(name, row0, num_rows):
    """the PLAIN_FUSED = False form: csr_gather_sum_wide (slots = 1) over all rows, the eps x term, gemm_f16x3"""
    xd, _, rowptr, col, w1, b1, w2, b2, s = _device(name)
    N, wp = xd.shape
    z = ops.csr_gather_sum_wide(xd, rowptr, col, N, 1)[row0:row0 + num_rows]
    if s is not None:
        z = z + s * xd[row0:row0 + num_rows]
    h = ops.gemm_f16x3(z.contiguous(), w1, b1, act=ops.ACT_RELU)
    return h if w2 is None else ops.gemm_f16x3(h, w2, b2, act=ops.ACT_RELU)


def _run(name):
    case, ref, m, f32 = _host(name)
    r0, n, o2 = case["row0"], case["num_rows"], case["out2_row0"]
    mode = case["out_mode"]
    got = _fused(name, r0, n, mode, out2_row0=o2)
    assert _same_bits(got, _fused(name, r0, n, mode, out2_row0=o2)), f"{name}: two launches on the same inputs differ"
    r = slice(o2 if mode == "out2" else r0, r0 + n)
    _gate(name, "layer fused", got, ref[r], m[r], f32[r])
    full = slice(r0, r0 + n)
    un = _unfused(name, r0, n)
    _gate(name, "layer un-fused", un, ref[full], m[full], f32[full])
    base = r.start
    if case["mats"] == 1:
        want = torch.relu(case["b1"]).to(DEV)
        for i in case["bare"]:                                   # z == 0: the row's scale must be 1
            if i >= base:
                assert _same_bits(got[i - base], want), f"{name}: bare row {i}"
    else:
        want = torch.relu(case["b2"]).to(DEV)
        for i in case["dead"]:                                   # relu(h) == 0: the second scale must be 1
            assert float(torch.relu(ref[i]).sub(torch.relu(case["b2"]).double()).abs().max()) == 0.0
            if i >= base:
                assert _same_bits(got[i - base], want), f"{name}: dead row {i} is not relu(b2) bit for bit"
                assert _same_bits(un[i - r0], want), f"{name}: dead row {i} of the un-fused form"
    if case["H"] is not None:                                    # the padded channels stay exactly 0
        assert not got[:, case["H"]:].any() and not un[:, case["H"]:].any() and got[:, :case["H"]].any()
    return got


def _family(word):
    return [n for n in P.CASES if n.split()[0] == word]


@pytest.mark.parametrize("name", _family("instantiation"))
def test_every_instantiation_matches_the_reference(name):
    """Wp in {64, 128, 192, 256} x num_mats in {1, 2} on O(1) inputs of both signs, rows (37, 203): every degree 0..9, a
    third of the rows empty, hubs of 301, 203 and 77 sources; self_scale 0.25 with two products, none with one."""
    assert {(P.CASES[n]["wp"], P.CASES[n]["mats"]) for n in _family("instantiation")} == {(w, m) for w in P.WIDTHS
                                                                                           for m in P.MATS}
    _run(name)


@pytest.mark.parametrize("name", _family("range"))
def test_row_ranges_match_the_reference(name):
    """(row0, num_rows) in {(0, 1), (0, 63), (0, 64), (5, 65), (37, 203)} with source-only rows on both sides; the rows
    of the NaN-filled ``out`` outside the range stay NaN."""
    _run(name)


@pytest.mark.parametrize("name", _family("arguments") + _family("outputs") + _family("degrees"))
def test_self_scale_outputs_and_strides_match_the_reference(name):
    """self_scale NULL, 0 and 0.25 for one and two products; ``out`` only, ``out2`` only (a column block of a
    [rows, 3 Wp + 7] buffer starting at column Wp + 5, from out2_row0 = 40 > row0 = 5 on) and both; x a column view with
    ldx = Wp + 12 and contiguous; an empty ``col``."""
    _run(name)


def test_self_scale_zero_equals_no_self_scale():
    a = _fused("arguments self_scale None Wp 64 mats 2", 5, 65, "out")
    case = P.make("arguments self_scale None Wp 64 mats 2")
    xd, _, rowptr, col, w1, b1, w2, b2, _ = _device("arguments self_scale None Wp 64 mats 2")
    out = torch.full(tuple(case["x"].shape), NAN, device=DEV)
    ops.plain_layer(xd, rowptr, col, 5, 65, w1, b1, w2, b2, self_scale=torch.zeros(1, device=DEV), out=out)
    assert _same_bits(a, out[5:70])


@pytest.mark.parametrize("name", _family("regime") + _family("padding"))
def test_value_ranges_dead_rows_and_padding_match_the_reference(name):
    """Rows at 2^-16 .. 2^16 mixed inside the 64-row tiles, everything x 1e5 and x 1e-4, 30 % all-zero rows (a zero row
    without sources gives relu(b1) bit for bit with one product), b1 strongly negative with three rows whose relu(h) is
    all zero (relu(b2) bit for bit with two products); H = 100 in Wp = 128 and H = 32 in Wp = 64 with zero padding: the
    columns >= H are exactly 0."""
    _run(name)


@pytest.mark.parametrize("name", _family("instantiation"))
def test_a_result_does_not_depend_on_the_tiling_or_on_row0(name):
    """rows (37, 203) launched once, and as (37, 50) + (87, 153) give the same bits"""
    case = _host(name)[0]
    assert (case["row0"], case["num_rows"]) == (37, 203)
    once = _fused(name, 37, 203, "out")
    out = torch.full(tuple(case["x"].shape), NAN, device=DEV)
    _fused(name, 37, 50, "out", out=out)
    assert _all_nan(out[:37]) and _all_nan(out[87:])
    _fused(name, 87, 153, "out", out=out)
    assert _all_nan(out[:37]) and _all_nan(out[240:])
    assert _same_bits(once, out[37:240]), f"{name}: the rows depend on the launch's tiling"


def test_each_bad_argument_is_refused_before_any_launch():
    """every argument valid but one -> -1 (DESCO_EINVAL) and a message naming the entry point; the NaN-filled outputs stay
    untouched"""
    L = _lib.lib()
    wp, n = 64, 8
    x = torch.randn(n + 1, wp + 4, device=DEV)
    rp = torch.arange(n + 2, dtype=torch.int32, device=DEV)
    col = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    w = ops.split_f16_planes(torch.randn(wp, wp, device=DEV))
    b = torch.zeros(wp, device=DEV)
    out = torch.full((n, wp), NAN, device=DEV)
    out2 = torch.full((n, wp), NAN, device=DEV)
    good = dict(x=x.data_ptr(), ldx=wp + 4, rowptr=rp.data_ptr(), col=col.data_ptr(), s=None, row0=0, num_rows=n, width=wp,
                mats=2, w1=w.planes.data_ptr(), s1=w.scale.data_ptr(), b1=b.data_ptr(), w2=w.planes.data_ptr(),
                s2=w.scale.data_ptr(), b2=b.data_ptr(), out=out.data_ptr(), ldo=wp, out2=out2.data_ptr(), ld2=wp,
                out2_row0=0)

    def call(**over):
        a = dict(good, **over)
        return L.desco_plain_layer_f16x3_f32(a["x"], a["ldx"], a["rowptr"], a["col"], a["s"], a["row0"], a["num_rows"],
                                             a["width"], a["mats"], a["w1"], a["s1"], a["b1"], a["w2"], a["s2"], a["b2"],
                                             a["out"], a["ldo"], a["out2"], a["ld2"], a["out2_row0"], None)
    bad = [dict(x=None), dict(rowptr=None), dict(col=None), dict(w1=None), dict(s1=None), dict(b1=None), dict(w2=None),
           dict(s2=None), dict(b2=None), dict(out=None, out2=None), dict(x=x.data_ptr() + 4), dict(w1=w.planes.data_ptr() + 2),
           dict(w2=w.planes.data_ptr() + 2), dict(ldx=wp + 2), dict(ldx=wp - 4), dict(ldo=wp - 1), dict(ld2=wp - 1),
           dict(width=96), dict(width=320), dict(width=0), dict(mats=0), dict(mats=3), dict(out=x.data_ptr()),
           dict(out2=x.data_ptr()), dict(row0=-1), dict(num_rows=-1), dict(out2_row0=-1), dict(num_rows=64 * 2 ** 31 + 1)]
    for over in bad:
        L.desco_gemm_f32_multi(5, None, None)                   # (another entry point's message in between)
        assert call(**over) == -1, over
        assert b"desco_plain_layer_f16x3_f32" in L.desco_last_error(), over
    torch.cuda.synchronize()
    assert _all_nan(out) and _all_nan(out2)
    assert call() == 0 and call(num_rows=0) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(out).any() and _same_bits(out, out2)


def test_torch_op_is_registered_and_runs_the_kernel():
    import desco_amd.torch_ops  # noqa: F401
    name = "arguments self_scale 0.25 Wp 64 mats 2"
    want = _fused(name, 5, 65, "out")
    xd, _, rowptr, col, w1, b1, w2, b2, s = _device(name)
    out = torch.full((xd.shape[0], 64), NAN, device=DEV)
    torch.ops.desco.plain_layer_f16x3(xd, rowptr, col, 5, 65, w1.planes, w1.scale, b1, w2.planes, w2.scale, b2, s, out)
    assert _same_bits(out[5:70], want)
