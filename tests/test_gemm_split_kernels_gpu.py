"""The single-problem split-precision GEMMs (csrc/gemm_split.hip, csrc/gemm_f16x3.hip) -- ops.gemm_split (bf16x6),
ops.gemm_bf16, ops.gemm_f16x3, the descriptor entry ops.gemm_split_desc with its backward epilogue and per-row-class
scalar tail, the streaming projection ops.linear64 and the plane / scale makers -- per element against the fp64 host
reference tests/gemm_split_reference.py.

Gate (that of tests/test_wide_kernels_gpu.py; no number of its own): E_kernel = max |got - ref| / mag over ALL elements a
launch computes, mag = the reference evaluated on absolute values (the sum of |terms| of the element, times the dropout
factor and |act'(gate)|).  E_kernel <= 4 E_f32, where E_f32 is the same figure of the reference evaluated in float32 on
the host over the case's parent of max(m, 257) rows (never a kernel's figure), and E_kernel <= 1e-4.  An element with
mag == 0 must be exactly 0.  tests/test_gemm_split_reference_host.py proves the gate reachable on every case below.
Every test prints E_kernel, E_f32 and their ratio as ``[parity]`` lines; the worst ratio per family (bf16x6, bf16, f16x3,
desc epilogue, linear64) is printed once more when the module ends.

Every case is launched twice (bit-identical), with a1, a2 and out as blocks of NaN-filled parents: a1 / a2 column views
with different leading dimensions (nothing outside [m, k] may reach a result, and a NaN would), out a column block at a
multiple of 4 (16-byte stores), at column 5 (misaligned pointer) or in rows of 3 n + 7 floats (ldc % 4 != 0: both take
the narrow stores); everything of out's parent outside the [m, n] block must still be NaN."""
import collections
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_split_reference as G  # noqa: E402
from desco_amd import _lib, ops  # noqa: E402

DEV = "cuda"
CEILING = 1e-4
NAN = float("nan")
ACT = {"none": ops.ACT_NONE, "relu": ops.ACT_RELU, "leaky": ops.ACT_LEAKY}
WORST = collections.defaultdict(lambda: (0.0, ""))      # family -> (worst E_kernel / E_f32 seen, its case)


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    for k in sorted(WORST):
        print(f"[parity] gemm_split worst E_kernel / E_f32 over the module, {k}: {WORST[k][0]:.2f} (gate 4) at {WORST[k][1]}")


def _gate(name, family, got, ref, mag, ef):
    """E_kernel <= 4 E_f32 and <= CEILING; zero where mag is zero"""
    g = got.detach().cpu().double().reshape(ref.shape)
    ek, i = G.scaled_error(g, ref, mag)
    ratio = ek / ef if ef > 0 else (0.0 if ek == 0 else float("inf"))
    WORST[family] = max(WORST[family], (ratio, name))
    print(f"[parity] {family}, {name}: E_kernel {ek:.3e}, E_f32 {ef:.3e}, ratio {ratio:.2f} (gate 4, ceiling {CEILING:.0e})")
    exact = bool((g[mag == 0] == 0).all())
    n = max(ref.shape[-1], 1)
    assert ek <= 4 * ef and ek <= CEILING and exact, (
        f"{family}, {name}: E_kernel {ek:.3e} E_f32 {ef:.3e} ratio {ratio:.2f}; element {i} (row {i // n}, column {i % n}): "
        f"got {float(g.flatten()[i])!r}, ref {float(ref.flatten()[i])!r}, mag {float(mag.flatten()[i])!r}"
        f"{'' if exact else '; nonzero where mag == 0'}")


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _all_nan(t):
    return bool(torch.isnan(t).all())


def _block(t, lead, off):
    """t [m, k] as rows 1 .. m, columns off .. off + k of a NaN-filled device parent [m + 2, lead] -> (view, parent)"""
    m, k = t.shape
    parent = torch.full((m + 2, lead), NAN)
    parent[1:m + 1, off:off + k] = t
    parent = parent.to(DEV)
    return parent[1:m + 1, off:off + k], parent


def _intact(view, parent, t, off):
    """the parent is NaN outside the block and holds t's bits inside"""
    m, k = t.shape
    return (_all_nan(parent[0]) and _all_nan(parent[m + 1]) and _all_nan(parent[:, :off]) and _all_nan(parent[:, off + k:])
            and _same_bits(view.cpu(), t))


@functools.lru_cache(maxsize=None)
def _host(name):
    """(case, fp64 reference, mag, E_f32 over the parent, fp64 pre-activation, its mag) of a named case, computed once"""
    case = G.make(name)
    ref, mag = G.evaluate(case), G.mag(case)
    ef = G.scaled_error(G.evaluate(case, torch.float32), ref, mag)[0]
    return case, ref, mag, ef, G.evaluate(case, pre=True), G.evaluate(case, absolute=True, pre=True)


def _out_block(case):
    """out [m, n] inside its NaN-filled parent, by the case's ``store`` -> (view, parent, column offset)"""
    m, n = case["m"], case["n"]
    lead, off = {"wide": (n + 12, 8), "offset5": (n + 12, 5), "ldc": (3 * n + 7, n + 4)}[case["store"]]
    parent = torch.full((m + 2, lead), NAN, device=DEV)
    out = parent[1:m + 1, off:off + n]
    narrow = out.data_ptr() % 16 != 0 or lead % 4 != 0
    assert narrow == (case["store"] != "wide")
    return out, parent, off


def _launch(case, a1, a2, weights, out):
    """one launch of the case's entry point on device operands"""
    m, n = case["m"], case["n"]
    dev = lambda t: None if t is None else t.to(DEV)                     # noqa: E731
    bias, act, slope = dev(case["bias"]), ACT[case["act"]], case["slope"]
    s = None if case["s"] is None else case["s"][:m].contiguous().to(DEV)
    ws = dev(case["ws"])
    if case["entry"] == "linear64":
        return ops.linear64(a1, weights, bias, act=act, slope=slope, out=out)
    if case["entry"] == "desc":
        pr = dict(a1=a1, a2=a2, bias=bias, act=act, slope=slope, out=out, s=s, ws=ws)
        if case["gate"] is not None:
            gate = case["gate"][:m]
            pr.update(gate=_block(gate, n + 4, 4)[0] if case["gate_act"] == "leaky" else gate.to(DEV),
                      gate_act=ACT[case["gate_act"]], gate_slope=case["gate_slope"])
        if case["drop"] is not None:
            d = case["drop"]
            key = torch.tensor([d["seed"], d["step"]], dtype=torch.int64, device=DEV)      # (seed, step): a pass's key
            pr["drop"] = ops.DropSite(key, d["site"], d["p"])
        return ops.gemm_split_desc(pr, weights)
    if s is None:
        fn = {"bf16x6": ops.gemm_split, "bf16": ops.gemm_bf16, "f16x3": ops.gemm_f16x3}[case["mode"]]
        return fn(a1, weights, bias, a2=a2, act=act, slope=slope, out=out)
    # the scalar tail of the plain entry points, which ops does not expose: the C ABI
    L = _lib.lib()
    a1p, lda1 = ops._rows(a1, "a1")
    a2p, lda2 = (None, 0) if a2 is None else ops._rows(a2, "a2")
    op, ldo = ops._rows(out, "out")
    k1, k2 = case["k1"], case["k2"]
    bp, br = (None, 1) if bias is None else (bias.data_ptr(), 1 if bias.dim() == 1 else bias.shape[0])
    assert ws.shape[0] == 1 and ws.is_contiguous() and tuple(s.shape) == (m, ws.shape[1])
    tail = (bp, br, s.data_ptr(), s.shape[1], ws.data_ptr(), act, slope, op, ldo, m)
    if case["mode"] == "f16x3":
        rs = ops.row_scale_f16(a1, a2)
        rc = L.desco_gemm_f16x3_f32(a1p, lda1, k1, a2p, lda2, k2, weights.planes.data_ptr(), weights.scale.data_ptr(), n,
                                    *tail, rs.data_ptr(), ops._stream())
    else:
        fn = L.desco_gemm_bf16x6_f32 if case["mode"] == "bf16x6" else L.desco_gemm_bf16_f32
        rc = fn(a1p, lda1, k1, a2p, lda2, k2, weights.data_ptr(), n, *tail, ops._stream())
    _lib.check(rc, "gemm with a scalar tail")
    torch.cuda.synchronize()                                             # (s, ws, rs stay alive until the launch is done)


def _weights(case):
    w = case["w"].to(DEV)
    if case["entry"] == "linear64":
        return ops.linear64_planes(w)
    if case["entry"] == "desc":                                          # from a weight kept as [in, out]
        return ops.split_bf16_planes_t(w.t().contiguous())
    return {"bf16x6": ops.split_bf16_planes, "bf16": ops.round_bf16, "f16x3": ops.split_f16_planes}[case["mode"]](w)


def _run(name):
    case, ref, mag, ef, pre, pre_mag = _host(name)
    m, n, k1, k2 = case["m"], case["n"], case["k1"], case["k2"]
    r = slice(0, m)
    h1, h2 = case["a1"][:m], None if case["a2"] is None else case["a2"][:m]
    if case["a1_contig"]:
        a1 = p1 = h1.to(DEV)
    else:
        a1, p1 = _block(h1, k1 + 8, 4)
    a2, p2 = (None, None) if h2 is None else _block(h2, k2 + 12, 8)
    assert a1.data_ptr() % 16 == 0 and (a2 is None or (a2.data_ptr() % 16 == 0 and a2.stride(0) != a1.stride(0)))
    weights = _weights(case)
    got = []
    for _ in range(2):
        out, parent, off = _out_block(case)
        _launch(case, a1, a2, weights, out)
        assert _all_nan(parent[0]) and _all_nan(parent[m + 1]) and _all_nan(parent[:, :off]) and _all_nan(parent[:, off + n:]), \
            f"{name}: out's parent was written outside the [m, n] block"
        assert not torch.isnan(out).any(), f"{name}: an element of out was not written (or is NaN)"
        got.append(out.clone())
    assert _same_bits(got[0], got[1]), f"{name}: two launches on the same inputs differ"
    assert case["a1_contig"] or _intact(a1, p1, h1, 4), f"{name}: a1 or its parent changed"
    assert a2 is None or _intact(a2, p2, h2, 8), f"{name}: a2 or its parent changed"
    _gate(name, G.family(case), got[0], ref[r], mag[r], ef)
    g = got[0].cpu()
    if case["regime"] == "zero":                                         # a zero row: act(bias) bit for bit, 0 without a bias
        z = ~case["a1"][:m].any(1) if h2 is None else ~(h1.any(1) | h2.any(1))
        want = torch.zeros(n) if case["bias"] is None else case["bias"]
        assert bool(z.any()) and torch.equal(g[z], want.expand(int(z.sum()), -1)), f"{name}: a zero row is not act(bias)"
    if case["entry"] == "desc":
        # the exactly-zero outputs are those whose dropout factor or gate derivative is 0 -- and, behind a relu, those the
        # relu clamps (decided by the fp64 pre-activation; left open where that lies within the gate's ceiling of 0)
        dead = mag[r] == 0
        clamp = (pre[r] <= 0) if case["act"] == "relu" else torch.zeros_like(dead)
        open_ = (pre[r].abs() <= CEILING * pre_mag[r]) if case["act"] == "relu" else torch.zeros_like(dead)
        assert bool(dead.any()) == (case["drop"] is not None or case["gate_act"] == "relu")
        bad = ((g == 0) != (dead | clamp)) & ~(open_ & ~dead)
        assert not bad.any(), (f"{name}: the zero pattern differs at (row, column) {bad.nonzero()[0].tolist()}: got "
                               f"{float(g[tuple(bad.nonzero()[0])])!r}, factor x act' zero: {bool(dead[tuple(bad.nonzero()[0])])}")
    return got[0]


def _family(word):
    return [n for n in G.CASES if n.split()[0] == word]


@pytest.mark.parametrize("name", _family("instantiation"))
def test_every_instantiation_matches_the_reference(name):
    """bf16x6, bf16 and f16x3 at n in {64, 128, 192} (WN = 1, 2, 3 column tiles per block) and n in {256, 320, 384} (ny =
    2, 5, 2 blocks along n), m = 129 (a second row tile of one row), K = 96"""
    _run(name)


@pytest.mark.parametrize("name", _family("rows"))
def test_row_edges_match_the_reference(name):
    """m in {1, 31, 32, 33, 63, 64, 65, 127, 128, 129}: the 32-row half tiles, the 64-row wave tiles and the 128-row
    block, clamped rows everywhere else; m = 1025 (nine row tiles: the second XCD round of the block map) and m = 1153 at
    n = 384 (local / ny and local % ny both above 0); the operand in two halves (k1 = k2 = 32)"""
    _run(name)


@pytest.mark.parametrize("name", _family("seam"))
def test_k_extents_and_the_operand_seam_match_the_reference(name):
    """K = 32 (one chunk: the ``nchunks > 1 ? 1 : 0`` prologue), 64, 96 (the ``ch + 2 < nchunks`` clamp), 160; the seam
    between a1 and a2 after one and two chunks and before three; the anchor GEMM's 300 x 576 x 576; a1 and a2 are column
    views of NaN-filled parents with leading dimensions k1 + 8 and k2 + 12 (in one case a1 is contiguous)"""
    _run(name)


@pytest.mark.parametrize("name", _family("regime"))
def test_value_ranges_match_the_reference(name):
    """O(1) rows, rows at 2^-16 .. 2^16, everything x 1e5 and x 1e-4, even K columns at 2^-20 of the odd ones, 30 %
    all-zero rows (act(bias) bit for bit; exactly 0 without a bias), at (m, n, K) = (129, 64, 128) and (257, 192, 192)"""
    _run(name)


@pytest.mark.parametrize("name", _family("store"))
def test_wide_and_narrow_stores_match_the_reference(name):
    """out at a 16-byte-aligned column block (nontemporal 16-byte stores), at column 5 (misaligned pointer) and in rows of
    3 n + 7 floats (ldc % 4 != 0): the last two take the scalar stores.  (Every other case of this module cycles through
    the three as well.)"""
    _run(name)


@pytest.mark.parametrize("name", _family("epilogue"))
def test_epilogues_match_the_reference(name):
    """m = 333 on the 64-, 128- and 192-column tiles.  Through ops.gemm_split_desc: bias per row class (29), the scalar
    tail with ns in {1, 3, 4} and ws_rows in {1, 29, 37} (classes that wrap inside and across the tiles), relu and leaky,
    the activation-derivative gate alone (relu, leaky; the gate holds +0.0, -0.0 and negative values), the dropout factor
    alone (p = 0.3 and 1.0, against oracle/dropout.py), and all of them together; the set of exactly-zero outputs is the
    set the factor and the gate derivative zero.  bf16 and f16x3: bias per row class and the ws_rows = 1 tail (C ABI)."""
    _run(name)


@pytest.mark.parametrize("name", _family("linear64"))
def test_linear64_matches_the_reference(name):
    """the streaming bf16x6 projection (K = 64): m in {1, 63, 64, 65, 257}, n in {64, 128, 192} (one launch of two column
    blocks, and one of two plus one of one), x a column view with ldx = 72, the three activations, with and without bias"""
    _run(name)


@pytest.mark.parametrize("mode", G.MODES)
def test_every_product_lands_at_its_own_element(mode):
    """the transposed-map check: row i of A is 2^(i % 5) at column (5 i + 3) % K, W holds distinct small integers, so
    out[i, j] = 2^(i % 5) W[j, perm(i)] EXACTLY (hi + mid + lo summed small to large is exact; so are small integers in
    fp16 and bf16) -- a wrong row, column or K index of any fragment shows as a wrong integer"""
    fn = {"bf16x6": ops.gemm_split, "bf16": ops.gemm_bf16, "f16x3": ops.gemm_f16x3}[mode]
    for n in (64, 192):
        for K in (32, 96):
            A, W, want = G.routing_case(mode, n, K)
            got = fn(A.to(DEV), W.to(DEV)).cpu()
            bad = (got != want).nonzero()
            assert not len(bad), (f"{mode} n {n} K {K}: {len(bad)} wrong elements, first (row, column) {bad[0].tolist()}: got "
                                  f"{float(got[tuple(bad[0])])!r}, want {float(want[tuple(bad[0])])!r}")
    print(f"[parity] {mode} routing probe: exact at n in (64, 192), K in (32, 96), m = 129")


# ---- the exact operations ---------------------------------------------------------------------------------------------
def _specimens(count):
    g = torch.Generator().manual_seed(count)
    x = torch.randn(count, generator=g) * 2.0 ** torch.randint(-60, 60, (count,), generator=g).float()
    x[:8] = torch.tensor([0.0, 1.0, -1.0, 2.0 ** -100, -1.0 - 2.0 ** -23, 1.0 + 2.0 ** -8, 2.0 - 2.0 ** -23, 3.0e38])
    return x


def test_bf16_plane_makers_are_bit_exact():
    """ops.split_bf16_planes, ops.split_bf16_planes_t on a strided [k, n] view and ops.round_bf16 against the host's
    truncation split and nearest-even rounding, bit for bit (ties, carries into the exponent, both signs, 2^-100 .. 3e38)"""
    x = _specimens(96 * 70).view(96, 70)                                 # [k, n]
    x[1, :4] = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -1.0 - 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -23])   # ties
    assert torch.equal(ops.split_bf16_planes(x.to(DEV)).cpu(), torch.from_numpy(G.split_bf16x3(x.numpy())))
    assert torch.equal(ops.round_bf16(x.to(DEV)).cpu(), torch.from_numpy(G.round_bf16(x.numpy())))
    view, parent = _block(x, 80, 4)
    got = ops.split_bf16_planes_t(view)
    assert tuple(got.shape) == (3, 70, 96)
    assert torch.equal(got.cpu(), torch.from_numpy(G.split_bf16x3(x.t().contiguous().numpy())))
    assert _intact(view, parent, x, 4)
    one = torch.tensor([[3.0]])
    assert torch.equal(ops.split_bf16_planes_t(one.to(DEV)).cpu(), torch.from_numpy(G.split_bf16x3(one.numpy())))


def test_f16_plane_maker_is_bit_exact():
    """ops.split_f16_planes: the planes and the {scale, 1 / scale} pair against the host split -- O(1) weights, a matrix of
    zeros (scale 1), elements so far below the maximum that hi or lo is an fp16 subnormal or 0, one huge element (scale
    2^-113), a tiny matrix (scale 2^126), more elements than one block's threads reduce in one pass"""
    g = torch.Generator().manual_seed(3)
    sub = torch.randn(64, 96, generator=g) * 2.0 ** torch.randint(-45, 1, (64, 96), generator=g).float()
    huge = torch.randn(64, 32, generator=g)
    huge[17, 5] = -3.0e38
    tiny = (1 + torch.rand(64, 32, generator=g)) * torch.sign(torch.randn(64, 32, generator=g)) * 2.0 ** -120
    for tag, w in (("o1", torch.randn(192, 96, generator=g)), ("zeros", torch.zeros(64, 32)), ("subnormal planes", sub),
                   ("huge", huge), ("tiny", tiny), ("3 x 5", torch.randn(3, 5, generator=g))):
        got = ops.split_f16_planes(w.to(DEV))
        planes, scale = G.split_f16x2(w.numpy())
        assert torch.equal(got.scale.cpu(), torch.from_numpy(scale)), f"{tag}: scale pair {got.scale.tolist()} != {scale.tolist()}"
        bad = (got.planes.cpu() != torch.from_numpy(planes)).nonzero()
        assert not len(bad), f"{tag}: {len(bad)} plane elements differ, first (plane, row, column) {bad[0].tolist()}"
    hi, lo = (torch.from_numpy(p) for p in G.split_f16x2(sub.numpy())[0].view(np.float16))
    normal = 2.0 ** -14
    assert ((hi != 0) & (hi.abs() < normal)).any() and ((lo != 0) & (lo.abs() < normal)).any() and (hi == 0).any()


@pytest.mark.parametrize("m", [1, 15, 16, 17, 257])
def test_row_scale_f16_is_the_row_maximum(m):
    """ops.row_scale_f16 (desco_row_absmax_f32: 16 lanes per row, 16 rows per block): exactly max_k |[a1 | a2][i, k]| for
    k in {4, 36, 68, 100} (fewer than 16 float4, a partial second pass), with and without a second operand, on strided
    views inside NaN parents, with a row of zeros and a row whose maximum is a negative element in its last column"""
    for k1 in (4, 36, 68, 100):
        for k2 in (0, 4, 36):
            g = torch.Generator().manual_seed(1000 * m + 10 * k1 + k2)
            a1, a2 = torch.randn(m, k1, generator=g), torch.randn(m, k2, generator=g) if k2 else None
            a1[m // 2] = 0
            if a2 is not None:
                a2[m // 2] = 0
            (a1 if a2 is None else a2)[m - 1, -1] = -7.5
            if m > 2:
                a1[0, 0] = -9.25
            v1, p1 = _block(a1, k1 + 8, 4)
            v2, p2 = (None, None) if a2 is None else _block(a2, k2 + 12, 8)
            got = ops.row_scale_f16(v1, v2).cpu()
            want = torch.from_numpy(G.row_absmax(a1.numpy(), None if a2 is None else a2.numpy()))
            assert want[m - 1] == 7.5 and (m == 1 or want[m // 2] == 0 or m // 2 in (0, m - 1))
            assert torch.equal(got, want), f"m {m}, k ({k1}, {k2}): rows {(got != want).nonzero().flatten().tolist()} differ"
            assert _intact(v1, p1, a1, 4) and (a2 is None or _intact(v2, p2, a2, 8))
