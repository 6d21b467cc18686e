"""The exact-fp32 GEMM family -- gemm / gemm_multi (csrc/gemm_f32.hip) and the split-M reductions gemm_tn, linear_bwd_w,
linear_bwd_w_multi, colsum, linear_smallk_bwd, rowdot_bwd (csrc/train_ops.hip) -- against tests/gemm_f32_reference.py.

Bit-equality, the main assertion: gemm_f32.hip states that v_mfma_f32_32x32x2_f32 is an fmaf chain per output element
in k order, train_ops.hip that partial sums are reduced in a fixed order, so the result of these kernels is defined bit
for bit and must have the bits of the reference's ordered float32 evaluation (``fma32`` chains, every other operation
one float32 operation).  It applies to gemm / gemm_multi without the ``s`` / ``ws`` tail (chain, bias add, activation,
dropout factor, gate, accum), gemm_tn, linear_bwd_w(_multi) (weights and bias row, both paths), colsum (both kernels)
and dz of rowdot_bwd.  A dropped, duplicated, misplaced or reordered term fails it; there is no tolerance to argue about.

The per-element gate (that of tests/test_pool_kernels_gpu.py / test_wide_kernels_gpu.py, no number of its own), on every
case of every kernel: E_kernel = max |got - ref64| / mag over all elements of the launch, E_kernel <= 4 E_f32 and
E_kernel <= 1e-4, an element with mag == 0 exactly 0.  E_f32 is the same figure of the ordered float32 evaluation of the
whole case.  It is the only assertion for the terms a compiler may or may not contract into an fma (the ``s`` / ``ws``
tail, dw / db of rowdot_bwd, smallk_bwd); for these E_f32 is the larger of the unfused and the fma32 evaluation.
tests/test_gemm_f32_reference_host.py proves the gate reachable on every case.

Every launch runs twice (bit-identical); outputs live in NaN-filled parents and nothing outside the rows and columns a
launch owns is written.  Every launch prints a ``[parity]`` line; the worst ratio per entry point and the number of
bit-pinned launches are printed once more when the module ends."""
import collections

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_f32_reference as G  # noqa: E402
from desco_amd import ops  # noqa: E402

DEV = "cuda"
NAN = float("nan")
F32 = np.float32
WORST = collections.defaultdict(float)          # entry point -> worst E_kernel / E_f32 seen
PINNED = collections.Counter()                  # entry point -> launches held bit for bit


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print(f"[parity] gemm_f32 worst E_kernel / E_f32 over the module, {k}: {WORST[k]:.2f} (gate 4); "
              f"{PINNED[k]} outputs bit-identical to the ordered float32 evaluation")
    print(f"[parity] gemm_f32 bit-pinned outputs in all: {sum(PINNED.values())}")


def T(x):
    if x.size == 0:                              # (an empty numpy array's strides are not those of a row-major tensor)
        return torch.empty(x.shape, device=DEV)
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


def _gate(name, entry, got, ref, mag, ef):
    """E_kernel <= 4 E_f32 (``ef``: the figure of the whole case) and <= the ceiling; zero where mag is zero"""
    got = np.asarray(got, np.float64).reshape(ref.shape)
    ek, i = G.scaled_error(got, ref, mag)
    ratio = ek / ef if ef > 0 else (0.0 if ek == 0 else float("inf"))
    WORST[entry] = max(WORST[entry], ratio)
    print(f"[parity] {entry}, {name}: E_kernel {ek:.3e}, E_f32 {ef:.3e}, ratio {ratio:.2f} (gate 4, ceiling {G.CEILING:.0e})")
    exact = bool((got[mag == 0] == 0).all())
    assert ek <= 4 * ef and ek <= G.CEILING and exact, (
        f"{entry}, {name}: E_kernel {ek:.3e} E_f32 {ef:.3e} ratio {ratio:.2f}; element {i}: got "
        f"{float(got.ravel()[i])!r}, ref {float(ref.ravel()[i])!r}, mag {float(mag.ravel()[i])!r}"
        f"{'' if exact else '; nonzero where mag == 0'}")


def _bits(name, entry, got, want):
    """the bits of the ordered float32 evaluation; on failure the element, both values, the number of differing elements"""
    got, want = np.ascontiguousarray(got, F32).reshape(want.shape), np.ascontiguousarray(want, F32)
    diff = got.view(np.int32) != want.view(np.int32)
    if diff.any():
        i = int(np.flatnonzero(diff.ravel())[0])
        ulps = G.ulp_distance(got, want)
        raise AssertionError(
            f"{entry}, {name}: {int(diff.sum())} of {diff.size} elements differ from the ordered float32 evaluation, "
            f"largest distance {int(ulps.max())} ulps; first at {np.unravel_index(i, want.shape)}: got "
            f"{float(got.ravel()[i])!r}, want {float(want.ravel()[i])!r}")
    PINNED[entry] += 1


def _check(name, entry, case, key, got, ref, mg, f32, ef):
    _gate(f"{name}, {key}", entry, got, ref[key], mg[key], ef[key])
    if G.is_pinned(case, key):
        _bits(f"{name}, {key}", entry, got, f32[key])
    else:                                        # (not asserted: which way the compiler went is its own business)
        fu = G.host_fused(case["name"])[key]
        print(f"[parity] {entry}, {name}, {key}: the bits of the fma32 evaluation: {G.same_bits(got, fu)}, of the unfused "
              f"one: {G.same_bits(got, f32[key])}")


def _block(x, lead, tail=4, above=0, below=0):
    """``x`` as a block of a NaN-filled parent [above + rows + below, lead + cols + tail] -> (view, parent)"""
    r, c = x.shape
    parent = torch.full((above + r + below, lead + c + tail), NAN)
    parent[above:above + r, lead:lead + c] = torch.from_numpy(np.ascontiguousarray(x))
    parent = parent.to(DEV)
    return parent[above:above + r, lead:lead + c], parent


def _only_block_written(parent, above, rows, lead, cols):
    rest = parent.clone()
    rest[above:above + rows, lead:lead + cols] = NAN
    return bool(torch.isnan(rest).all())


def _guarded(numel):
    """a [numel] float32 device vector between two NaN guards of 4 floats (16-byte aligned) -> (view, parent)"""
    parent = torch.full((numel + 8,), NAN, device=DEV)
    return parent[4:4 + numel], parent


def _guards_intact(parent):
    return bool(torch.isnan(parent[:4]).all() and torch.isnan(parent[-4:]).all())


def _same(a, b):
    return G.same_bits(a, b)


# ---- gemm, gemm_multi -----------------------------------------------------------------------------------------------------------
def _gemm_operands(case):
    a1 = _block(case["a1"], 4)[0] if case["a1_block"] else T(case["a1"])
    a2 = None
    if case["a2"] is not None:
        ld2, k2 = case["a2_ld"], case["a2"].shape[1]
        a2 = _block(case["a2"], 0, ld2 - k2)[0] if ld2 > k2 else T(case["a2"])
    return a1, a2


def _gemm_out(case):
    """the output block of a NaN-filled parent (ldc = n + 3: rows of the parent are not 16-byte aligned), holding the
    previous output where the product accumulates -> (view, check)"""
    m, n = case["m"], case["n"]
    lead, tail = (2, 1) if case["ldc"] == n + 3 else (0, 0)
    init = case["prev"] if case["prev"] is not None else np.full((m, n), NAN, F32)
    out, parent = _block(init, lead, tail, 1, 1)
    return out, (lambda: _only_block_written(parent, 1, m, lead, n))


def _drop_of(case, site):
    if case["drop"] is None:
        return None
    return ops.DropSite(torch.tensor([20240 + site, 7], dtype=torch.int64).to(DEV), site, case["drop"])


def _problem(case, site=0):
    """the gemm_multi descriptor of a case, with an output of its own -> (dict, out view, check)"""
    a1, a2 = _gemm_operands(case)
    out, check = _gemm_out(case)
    pr = dict(a1=a1, a2=a2, wt=T(case["wt"]), out=out, act=case["act"], slope=case["slope"])
    if case["bias"] is not None:
        assert case["bias"].shape[0] == 1
        pr["bias"] = T(case["bias"][0])
    if case["gate"] is not None:
        pr.update(gate=_block(case["gate"], 0, case["ldg"] - case["n"])[0], gate_act=case["gate_act"],
                  gate_slope=case["gate_slope"])
    if case["prev"] is not None:
        pr["accum"] = True
    if case["drop"] is not None:
        pr["drop"] = _drop_of(case, site)
    return pr, out, check


def _empty_problem():
    return dict(a1=torch.empty(0, 64, device=DEV), wt=torch.zeros(64, 64, device=DEV), out=torch.empty(0, 64, device=DEV))


def _gemm_once(case):
    a1, a2 = _gemm_operands(case)
    out, check = _gemm_out(case)
    got = ops.gemm(a1, T(case["wt"]), None if case["bias"] is None else T(case["bias"]), a2, case["act"], case["slope"],
                   None if case["s"] is None else T(case["s"]), None if case["ws"] is None else T(case["ws"]), out=out)
    assert got.data_ptr() == out.data_ptr() and check(), "written outside the output block"
    return N(out)


@pytest.mark.parametrize("name", G.family("gemm"))
def test_gemm_is_the_fmaf_chain_in_k_order(name):
    """m = 1 .. 257 around the 32-row waves and the 128-row tile, one to twenty K chunks with the a1 / a2 switch inside,
    n = 64 and 192, bias_rows none / 1 / 7 / 29, every activation, a1 as a column block, a2 with another ld, the output
    a block of a NaN-filled parent with ldc = n + 3, operands with exact zeros: the bits of the ordered float32
    evaluation (without the s / ws tail) and within the gate (always)"""
    case, ref, mg, f32, ef = G.host(name)
    got = _gemm_once(case)
    assert _same(got, _gemm_once(case)), f"{name}: two launches on the same inputs differ"
    _check(name, "gemm", case, "c", got, ref, mg, f32, ef)


def _multi_once(cases, sites):
    """one gemm_multi launch of the cases (None: an m = 0 product) -> the outputs, in order"""
    built = [None if c is None else _problem(c, s) for c, s in zip(cases, sites)]
    ops.gemm_multi([_empty_problem() if b is None else b[0] for b in built])
    for b in built:
        assert b is None or b[2](), "written outside the output block"
    return [None if b is None else N(b[1]) for b in built]


def _expect_drop(case, site):
    """(ref64, mag, ordered float32, E_f32, factors) of a dropout case under the factors ops.dropout_mask regenerates"""
    fac = N(ops.dropout_mask(_drop_of(case, site), case["m"], case["n"]))
    ref, mg, f32 = (fn(case, fac=fac)["c"] for fn in (G.evaluate, G.mag, lambda c, fac: G.evaluate(c, F32, fac=fac)))
    return ref, mg, f32, G.scaled_error(f32, ref, mg)[0], fac


@pytest.mark.parametrize("name", G.family("mprod"))
def test_gemm_multi_product_alone(name):
    """gate relu / leaky on a saved output that holds +0.0 and -0.0 (neither is > 0) with a strided ldg, accum into a
    prefilled output, m = 1, 129, 300, n = 64, 192: bits and gate"""
    case, ref, mg, f32, ef = G.host(name)
    got = _multi_once([case], [0])[0]
    assert _same(got, _multi_once([case], [0])[0]), f"{name}: two launches on the same inputs differ"
    _check(name, "gemm_multi", case, "c", got, ref, mg, f32, ef)


_EXTRA_LAUNCH = ["drop m = 130, none, gate leaky", "mprod plain: m = 129, k = (64, 0), n = 64", None, "drop m = 5, relu, gate relu"]


def _launch_names(i):
    if i == len(G.MULTI_LAUNCHES):
        return _EXTRA_LAUNCH
    fam = G.family("mprod")
    return [None if j is None else fam[j] for j in G.MULTI_LAUNCHES[i]]


@pytest.mark.parametrize("launch", range(len(G.MULTI_LAUNCHES) + 1))
def test_gemm_multi_slots_are_bit_identical_to_the_product_alone(launch):
    """1 to 4 products of different m and n in one launch, an m = 0 product in the middle, two with dropout: every
    rotation of the launch -- every slot a product can take -- gives each product the bits it has launched alone,
    its dropout mask included (the site and key stay with the product)"""
    names = _launch_names(launch)
    cases = [None if n is None else G.make(n) for n in names]
    sites = list(range(len(cases)))
    alone = [None if c is None else _multi_once([c], [s])[0] for c, s in zip(cases, sites)]
    for rot in range(len(cases)):
        order = [(i + rot) % len(cases) for i in range(len(cases))]
        got = _multi_once([cases[i] for i in order], [sites[i] for i in order])
        for i, g in zip(order, got):
            assert (g is None) == (alone[i] is None)
            assert g is None or _same(g, alone[i]), f"{names[i]} in slot {order.index(i)} of launch {names} differs from alone"
    print(f"[parity] gemm_multi, launch {names}: every slot bit-identical to the product alone")


@pytest.mark.parametrize("name", G.family("drop"))
def test_gemm_multi_dropout_is_the_mask_of_dropout_mask(name):
    """m = 1, 3, 5 (row quads cut by the range end) and 130 (a second tile: the quad is that of the absolute row), act
    none / relu, gate on / off: the factor of every element is the one ops.dropout_mask regenerates -- every element it
    drops is 0, with act none and no gate no other is; the kept elements are float32(v * scale) (the bits of the ordered
    evaluation under those factors)"""
    case = G.make(name)
    ref, mg, f32, ef, fac = _expect_drop(case, 3)
    assert (fac == 0).any() or case["m"] == 1
    assert set(np.unique(fac)) <= {F32(0), F32(1.0 / (1.0 - case["drop"]))}
    got = _multi_once([case], [3])[0]
    assert _same(got, _multi_once([case], [3])[0]), f"{name}: two launches on the same inputs differ"
    assert (got[fac == 0] == 0).all(), f"{name}: an element ops.dropout_mask drops is not 0"
    if case["act"] == G.ACT_NONE and case["gate"] is None:
        assert ((got == 0) == (fac == 0)).all(), f"{name}: the zeroed elements are not those of ops.dropout_mask"
    _gate(name, "gemm_multi dropout", got, ref, mg, ef)
    _bits(name, "gemm_multi dropout", got, f32)


@pytest.mark.parametrize("name", G.family("dropacc"))
def test_gemm_multi_dropout_with_accum_is_within_the_gate(name):
    """v * fac + prev with no gate between them is the one pair of epilogue steps a compiler may contract into an fma:
    held to the gate of the larger of the two float32 evaluations under the factors of ops.dropout_mask, not to bits;
    a dropped element keeps the previous output bit for bit"""
    case = G.make(name)
    fac = N(ops.dropout_mask(_drop_of(case, 3), case["m"], case["n"]))
    ref, mg = G.evaluate(case, fac=fac)["c"], G.mag(case, fac=fac)["c"]
    evals = [G.evaluate(case, F32, fused=fused, fac=fac)["c"] for fused in (False, True)]
    ef = max(G.scaled_error(e, ref, mg)[0] for e in evals)
    got = _multi_once([case], [3])[0]
    assert _same(got, _multi_once([case], [3])[0]), f"{name}: two launches on the same inputs differ"
    assert _same(got[fac == 0], case["prev"][fac == 0]), f"{name}: a dropped element changed the previous output"
    _gate(name, "gemm_multi dropout + accum", got, ref, mg, ef)
    print(f"[parity] gemm_multi dropout + accum, {name}: the bits of the fma32 evaluation: {_same(got, evals[1])}, of the "
          f"unfused one: {_same(got, evals[0])}")


def test_gemm_multi_refuses_five_products_and_a_2d_bias():
    case = G.make(G.family("mprod")[0])
    with pytest.raises(RuntimeError, match="desco_gemm_f32_multi"):
        ops.gemm_multi([_problem(case)[0] for _ in range(5)])
    pr = _problem(case)[0]
    pr["bias"] = torch.zeros(7, case["n"], device=DEV)
    with pytest.raises(AssertionError):
        ops.gemm_multi([pr])


# ---- gemm_tn --------------------------------------------------------------------------------------------------------------------
def _tn_once(case):
    a = _block(case["a"], 4)[0] if case["strided"] else T(case["a"])
    b = _block(case["b"], 4)[0] if case["strided"] else T(case["b"])
    k, n = case["a"].shape[1], case["b"].shape[1]
    init = case["prev"] if case["prev"] is not None else np.full((k, n), NAN, F32)
    lead, tail, above, below = {"plain": (0, 0, 0, 0), "rowblock": (0, 0, 0, k), "colblock": (0, 4, 1, 1)}[case["out"]]
    out, parent = _block(init, lead, tail, above, below)
    got = ops.gemm_tn(a, b, out=out, accumulate=case["prev"] is not None)
    assert got.data_ptr() == out.data_ptr() and _only_block_written(parent, above, k, lead, n)
    return N(out)


@pytest.mark.parametrize("name", G.family("tn"))
def test_gemm_tn_is_one_chain_per_slab_folded_in_order(name):
    """m = 1 .. 1025 around the 32-row chunk and the first split at m = 513, (k, n) = (64, 64), (128, 64), (64, 128),
    strided a and b, out as the row block dwt[:k] of a taller tensor and as a column block with ldo = n + 4, accumulate
    on a prefilled output: bits and gate"""
    case, ref, mg, f32, ef = G.host(name)
    got = _tn_once(case)
    assert _same(got, _tn_once(case)), f"{name}: two launches on the same inputs differ"
    _check(name, "gemm_tn", case, "out", got, ref, mg, f32, ef)


# ---- linear_bwd_w, linear_bwd_w_multi -------------------------------------------------------------------------------------------
def _bwdw_operands(case):
    m = case["m"]
    a1 = _block(case["a1"], 4)[0] if case["a1_block"] and m else T(case["a1"])
    a2 = None if case["a2"] is None else T(case["a2"])
    return a1, a2, T(case["dz"])


def _bwdw_wrapper(case, want_bias):
    a1, a2, dz = _bwdw_operands(case)
    dwt, dbias = ops.linear_bwd_w(a1, a2, dz, want_bias)
    assert (dbias is None) == (not want_bias)
    return N(dwt), None if dbias is None else N(dbias)


def _bwdw_ctypes(case, want_bias):
    """desco_linear_bwd_w_f32 with lddw = n + 4 (ops.linear_bwd_w always passes n), dwt a block of a NaN-filled parent,
    dbias between guards (or NULL), the workspace NaN-filled with a guard behind it"""
    a1, a2, dz = _bwdw_operands(case)
    m, k1 = case["a1"].shape
    k2 = 0 if a2 is None else a2.shape[1]
    k, n = k1 + k2, dz.shape[1]
    dwt, parent = _block(np.full((k, n), NAN, F32), 0, 4, 1, 1)
    dbias, bparent = _guarded(n)
    L = ops._lib.lib()
    nws = L.desco_linear_bwd_w_workspace(m, k, n) // 4
    ws, wparent = _guarded(nws)
    a1p, lda1 = ops._rows(a1, "a1")
    a2p, lda2 = (None, 0) if a2 is None else ops._rows(a2, "a2")
    zp, ldz = ops._rows(dz, "dz")
    ops._lib.check(L.desco_linear_bwd_w_f32(a1p, lda1, k1, a2p, lda2, k2, zp, ldz, m, n, dwt.data_ptr(), n + 4,
                                            dbias.data_ptr() if want_bias else None, ws.data_ptr(), ops._stream()),
                   "linear_bwd_w")
    torch.cuda.synchronize()
    assert _only_block_written(parent, 1, k, 0, n) and _guards_intact(bparent) and _guards_intact(wparent)
    if not want_bias:
        assert bool(torch.isnan(bparent).all()), "dbias is NULL and something was written for it"
    if G.bwdw_splits(m, k, n)[0] == 1:
        assert bool(torch.isnan(wparent).all()), "the one-slab path writes its results in place, not to the workspace"
    return N(dwt), N(dbias) if want_bias else None


@pytest.mark.parametrize("name", G.family("bwdw"))
def test_linear_bwd_w_is_the_chain_and_the_16_bias_groups(name):
    """m = 0 .. 1000 around the 16 bias groups, the 32-row chunk and the first split at m = 257, (k1, k2) = (64, 0),
    (128, 64), (64, 64), n = 64, 128, a1 as a column block, with and without the bias row on both paths, lddw = n and
    (through ctypes) n + 4: weights and bias row have the bits of the ordered float32 evaluation; m = 0 gives zeros"""
    case, ref, mg, f32, ef = G.host(name)
    for how, run in (("lddw = n", _bwdw_wrapper), ("lddw = n + 4", _bwdw_ctypes)):
        dwt, db = run(case, case["want_bias"])
        dwt2, db2 = run(case, case["want_bias"])
        assert _same(dwt, dwt2) and (db is None or _same(db, db2)), f"{name}: two launches on the same inputs differ"
        _check(f"{name}, {how}", "linear_bwd_w", case, "dwt", dwt, ref, mg, f32, ef)
        if case["want_bias"]:
            _check(f"{name}, {how}", "linear_bwd_w", case, "dbias", db, ref, mg, f32, ef)
        if case["m"] == 0:
            assert (dwt == 0).all() and (db is None or (db == 0).all())


def _bwdw_multi_problems():
    fam = G.family("bwdw")
    out = []
    for slot, j in enumerate(G.BWDW_MULTI):
        case = G.make(fam[j])
        want_bias = case["want_bias"] != (slot >= 13)            # the repeated problems: with and without dbias
        a1, a2, dz = _bwdw_operands(case)
        k, n = case["a1"].shape[1] + (0 if a2 is None else a2.shape[1]), dz.shape[1]
        out.append((fam[j], case, want_bias, dict(a1=a1, a2=a2, dz=dz, dwt=torch.full((k, n), NAN, device=DEV),
                                                  dbias=torch.full((n,), NAN, device=DEV) if want_bias else None)))
    return out


def test_linear_bwd_w_multi_is_bit_identical_to_the_single_problem_calls():
    """16 problems in one call, one-slab and split ones mixed, two with m = 0, some without dbias: every problem has the
    bits of its single-problem call and of the ordered float32 evaluation"""
    probs = _bwdw_multi_problems()
    assert len(probs) == 16
    ops.linear_bwd_w_multi([p[3] for p in probs])
    first = [(N(p[3]["dwt"]), None if p[3]["dbias"] is None else N(p[3]["dbias"])) for p in probs]
    again = _bwdw_multi_problems()
    ops.linear_bwd_w_multi([p[3] for p in again])
    for slot, ((name, case, want_bias, pr), (dwt, db)) in enumerate(zip(again, first)):
        assert _same(N(pr["dwt"]), dwt) and (db is None or _same(N(pr["dbias"]), db)), f"slot {slot}: two calls differ"
        sdwt, sdb = _bwdw_wrapper(case, want_bias)
        assert _same(dwt, sdwt), f"slot {slot}, {name}: dwt differs from the single-problem call"
        assert db is None or _same(db, sdb), f"slot {slot}, {name}: dbias differs from the single-problem call"
        _, ref, mg, f32, ef = G.host(name)
        _check(f"slot {slot}, {name}", "linear_bwd_w_multi", case, "dwt", dwt, ref, mg, f32, ef)
        if want_bias:
            _check(f"slot {slot}, {name}", "linear_bwd_w_multi", case, "dbias", db, ref, mg, f32, ef)


def test_linear_bwd_w_multi_keeps_to_each_problem_s_workspace_range():
    """the call through ctypes on a NaN-filled workspace: the ranges of the one-slab problems (results written in place),
    the bias rows of the split problems without dbias and the guard behind the workspace still hold NaN, every other
    float of a split problem's range is written, and the results are those of the wrapper's call"""
    probs = _bwdw_multi_problems()
    descs = (ops._lib.BwdWDesc * len(probs))()
    ranges = []
    off = 0
    for d, (name, case, want_bias, pr) in zip(descs, probs):
        d.a1, d.lda1 = ops._rows(pr["a1"], "a1")
        d.k1, d.k2 = pr["a1"].shape[1], 0 if pr["a2"] is None else pr["a2"].shape[1]
        if pr["a2"] is not None:
            d.a2, d.lda2 = ops._rows(pr["a2"], "a2")
        d.dz, d.lddz = ops._rows(pr["dz"], "dz")
        d.m, d.n = case["m"], pr["dz"].shape[1]
        d.dwt, d.dbias = pr["dwt"].data_ptr(), None if pr["dbias"] is None else pr["dbias"].data_ptr()
        k = d.k1 + d.k2
        splits = G.bwdw_splits(d.m, k, d.n)[0]
        ranges.append((off, splits, k, d.n, want_bias))
        off += splits * (k + 1) * d.n
    L = ops._lib.lib()
    assert L.desco_linear_bwd_w_multi_workspace(len(probs), descs) == 4 * off
    ws, wparent = _guarded(off)
    ops._lib.check(L.desco_linear_bwd_w_multi_f32(len(probs), descs, ws.data_ptr(), ops._stream()), "linear_bwd_w_multi")
    torch.cuda.synchronize()
    assert _guards_intact(wparent)
    w = N(ws)
    for slot, (o, splits, k, n, want_bias) in enumerate(ranges):
        mine = w[o:o + splits * (k + 1) * n].reshape(splits, k + 1, n)
        if splits == 1:
            assert np.isnan(mine).all(), f"slot {slot}: a one-slab problem wrote to the workspace"
        else:
            assert not np.isnan(mine[:, :k]).any(), f"slot {slot}: a partial was not written"
            assert np.isnan(mine[:, k]).all() != want_bias, f"slot {slot}: the bias row of the partials"
    ref = _bwdw_multi_problems()
    ops.linear_bwd_w_multi([p[3] for p in ref])
    for slot, (a, b) in enumerate(zip(probs, ref)):
        assert _same(N(a[3]["dwt"]), N(b[3]["dwt"])), slot
        assert a[3]["dbias"] is None or _same(N(a[3]["dbias"]), N(b[3]["dbias"])), slot
    print(f"[parity] linear_bwd_w_multi, workspace: {sum(r[1] == 1 for r in ranges)} one-slab ranges and the guard untouched")


def test_linear_bwd_w_multi_refuses_17_problems():
    probs = [p[3] for p in _bwdw_multi_problems()]
    with pytest.raises(RuntimeError, match="desco_linear_bwd_w_multi_f32"):
        ops.linear_bwd_w_multi(probs + probs[:1])


# ---- colsum ---------------------------------------------------------------------------------------------------------------------
def _colsum_once(case):
    m, n = case["x"].shape
    if case["place"] == "aligned":
        x = T(case["x"])
    else:
        x = _block(case["x"], case["lead"], case["ldx"] - n - case["lead"])[0]
    assert ((x.data_ptr() % 16 == 0 and n % 4 == 0 and (m == 1 or x.stride(0) % 4 == 0)) == (G.colsum_kernel(case) == "partial4"))
    out, parent = _guarded(n)
    if case["prev"] is not None:
        out.copy_(T(case["prev"]))
    got = ops.colsum(x, out=out, accumulate=case["prev"] is not None)
    assert got.data_ptr() == out.data_ptr() and _guards_intact(parent)
    return N(out)


@pytest.mark.parametrize("name", G.family("colsum"))
def test_colsum_is_the_documented_sum_in_both_kernels(name):
    """n = 1, 29, 65 (scalar kernel), 64, 100, 256 (colsum_partial4_kernel), m = 1 .. 1000 around the 4- and 16-row
    groups, the 64-row step and the 256-row slab, 140 001 rows (slabs of 274: the four-in-flight loop with a remainder),
    the same 64 columns aligned, as parent[:, 1:65] and with ldx = 65, accumulate: bits and gate"""
    case, ref, mg, f32, ef = G.host(name)
    got = _colsum_once(case)
    assert _same(got, _colsum_once(case)), f"{name}: two launches on the same inputs differ"
    _check(f"{name} [{G.colsum_kernel(case)}]", "colsum", case, "out", got, ref, mg, f32, ef)


# ---- rowdot_bwd, smallk_bwd -----------------------------------------------------------------------------------------------------
def _rowdot_once(case):
    """desco_rowdot_bwd_f32 through ctypes: dz a block of a NaN-filled parent (lddz = n + 4), dwb between guards"""
    R, n = case["y"].shape
    y = _block(case["y"], 4)[0] if case["strided"] else T(case["y"])
    dz, parent = _block(np.full((R, n), NAN, F32), 0, 4, 1, 1)
    dwb, bparent = _guarded(n + 1)
    ws, wparent = _guarded(1024 * (n + 1))
    w, d = T(case["w"]), T(case["dout"])
    yp, ldy = ops._rows(y, "y")
    ops._lib.check(ops._lib.lib().desco_rowdot_bwd_f32(yp, ldy, n, w.data_ptr(), d.data_ptr(), R, dz.data_ptr(), n + 4,
                                                       dwb.data_ptr(), ws.data_ptr(), ops._stream()), "rowdot_bwd")
    torch.cuda.synchronize()
    assert _only_block_written(parent, 1, R, 0, n) and _guards_intact(bparent) and _guards_intact(wparent)
    return N(dz), N(dwb)


@pytest.mark.parametrize("name", G.family("rowdot"))
def test_rowdot_bwd_dz_bits_and_dwb_gate(name):
    """n = 16, 64, 256, 1024 (64, 16, 4, 1 row groups), R = 1 .. 1000 around the 256-row slab, 262 145 rows at n = 16
    (1024 slabs of 257), y strided with signed zeros (neither is > 0): dz has the bits of d * w; dw and db, whose
    products a compiler may contract, are within the gate of the larger of the two float32 evaluations"""
    case, ref, mg, f32, ef = G.host(name)
    dz, dwb = _rowdot_once(case)
    dz2, dwb2 = _rowdot_once(case)
    assert _same(dz, dz2) and _same(dwb, dwb2), f"{name}: two launches on the same inputs differ"
    _check(name, "rowdot_bwd", case, "dz", dz, ref, mg, f32, ef)
    _check(name, "rowdot_bwd", case, "dwb", dwb, ref, mg, f32, ef)


def _smallk_operands(case):
    if case["views"]:
        return (_block(case["feat"], 2, 3)[0],                   # a column pair (block) of a wider tensor
                _block(case["dout"], 0, 0, 3, 2)[0])             # a row-offset view
    return T(case["feat"]), T(case["dout"])


def _smallk_once(case):
    """desco_linear_smallk_bwd_f32 through ctypes: dwb and the 512 (k + 1) 64 float workspace between NaN guards"""
    m, k = case["feat"].shape
    feat, dout = _smallk_operands(case)
    dwb, bparent = _guarded((k + 1) * 64)
    ws, wparent = _guarded(512 * (k + 1) * 64)
    fp, ldf = ops._rows(feat, "feat")
    dp, ldd = ops._rows(dout, "dout")
    ops._lib.check(ops._lib.lib().desco_linear_smallk_bwd_f32(fp, ldf, k, dp, ldd, m, dwb.data_ptr(), ws.data_ptr(),
                                                              ops._stream()), "linear_smallk_bwd")
    torch.cuda.synchronize()
    assert _guards_intact(bparent) and _guards_intact(wparent), "written outside dwb or the workspace"
    splits = G.rows_splits(m, 512)[0]
    assert bool(torch.isnan(ws[splits * (k + 1) * 64:]).all()), "written behind the slabs' partials"
    return N(dwb).reshape(k + 1, 64)


@pytest.mark.parametrize("name", G.family("smallk"))
def test_smallk_bwd_is_within_the_gate(name):
    """k = 1, 2, 3, 16, m = 1 .. 257 around the 16 row groups and the 256-row slab, 131 073 rows (512 slabs of 257),
    feat as a column block of a wider tensor, dout as a row-offset view: weight rows and bias row within the gate of the
    larger of the unfused and the fma32 evaluation (the products may be contracted: not bit-pinned); dwb and the
    workspace sit between NaN guards and nothing behind the slabs' partials is written"""
    case, ref, mg, f32, ef = G.host(name)
    got = _smallk_once(case)
    assert _same(got, _smallk_once(case)), f"{name}: two launches on the same inputs differ"
    dwt, db = ops.linear_smallk_bwd(*_smallk_operands(case))
    assert _same(got, np.concatenate([N(dwt), N(db)[None, :]])), f"{name}: ops.linear_smallk_bwd differs from the entry point"
    _check(name, "smallk_bwd", case, "dwb", got, ref, mg, f32, ef)


# ---- empty batches and bad arguments --------------------------------------------------------------------------------------------
def test_empty_batches():
    """m = 0: gemm_tn and colsum write zeros (autograd.py's unfused weight-gradient path reaches both with an empty
    batch; they used to refuse the NULL operands torch hands over), with accumulate the output stays as it is;
    rowdot_bwd, which the gossip trunks' backward reaches with an empty batch, writes dwb = 0 and leaves dz alone;
    linear_smallk_bwd, which autograd.py guards on both call sites, refuses by name"""
    e64 = torch.empty(0, 64, device=DEV)
    out = torch.full((64, 128), NAN, device=DEV)
    ops.gemm_tn(e64, torch.empty(0, 128, device=DEV), out=out)
    assert bool((out == 0).all())
    prev = torch.randn(64, 64).to(DEV)
    out = prev.clone()
    ops.gemm_tn(e64, e64, out=out, accumulate=True)
    assert torch.equal(out, prev)
    for n in (29, 64):
        assert bool((ops.colsum(torch.empty(0, n, device=DEV)) == 0).all())
    prev = torch.randn(64).to(DEV)
    assert torch.equal(ops.colsum(e64, out=prev.clone(), accumulate=True), prev)
    for n in (16, 64, 256, 1024):
        dz, dwb = ops.rowdot_bwd(torch.empty(0, n, device=DEV), torch.randn(n).to(DEV), torch.empty(0, device=DEV))
        assert tuple(dz.shape) == (0, n) and tuple(dwb.shape) == (n + 1,) and bool((dwb == 0).all())
    with pytest.raises(RuntimeError, match="desco_linear_smallk_bwd_f32"):
        ops.linear_smallk_bwd(torch.empty(0, 2, device=DEV), e64)


def _empty_gossip_operands(Q=5):
    """the operands of the gossip trunks for a batch without nodes: (constants, parameters by name)"""
    g = torch.Generator().manual_seed(11)
    rnd = lambda *shape: (torch.randn(*shape, generator=g) / 4).to(DEV)                # noqa: E731
    const = [torch.zeros(1, dtype=torch.int32, device=DEV), torch.empty(0, dtype=torch.int32, device=DEV), 0, Q,
             torch.empty(0, 6, device=DEV), torch.empty(0, 3, device=DEV), torch.empty(0, 2, device=DEV),
             torch.empty(0, device=DEV)]
    par = dict(V0=rnd(Q, 6, 64), g1=torch.rand(Q, generator=g).to(DEV), wt1=rnd(128, 64), V1=rnd(Q, 3, 64), wtp=rnd(128, 64),
               Vp=rnd(Q, 2, 64), w3t=rnd(64, 64), b3=rnd(64), w5t=rnd(64, 256), b5=rnd(256), w7=rnd(256), b7=rnd(1))
    return const, {k: v.requires_grad_() for k, v in par.items()}


@pytest.mark.parametrize("form", ("bf16x6", "fp32", "deep"))
def test_an_empty_batch_through_the_gossip_trunks_gives_zero_gradients(form, monkeypatch):
    """a gossip batch without nodes passes the forward of GossipTrunk (input-gradient products on the bf16x6 pipe and in
    exact fp32) and of GossipTrunkDeep (L = 2); the backward then hands rowdot_bwd the NULL pointers of empty tensors:
    every parameter gradient is zeros of the parameter's shape"""
    from desco_amd import autograd as AG
    monkeypatch.setattr(AG, "TRAIN_GEMM_BF16X6", form == "bf16x6")
    const, p = _empty_gossip_operands()
    w3, w5 = p["w3t"].detach().t().contiguous(), p["w5t"].detach().t().contiguous()
    if form == "deep":
        order = ("V0", "w3t", "b3", "w5t", "b5", "w7", "b7", "wtp", "Vp", "g1", "wt1", "V1")
        pred = AG.GossipTrunkDeep.apply(*const, w3, w5, None, 2, *[p[k] for k in order])
    else:
        order = ("V0", "g1", "wt1", "V1", "wtp", "Vp", "w3t", "b3", "w5t", "b5", "w7", "b7")
        pred = AG.GossipTrunk.apply(*const, (1.0 - p["g1"]).detach().contiguous(), w3, w5, None, *[p[k] for k in order])
    assert tuple(pred.shape) == (0,)
    pred.backward(torch.empty(0, device=DEV))
    for k in order:
        assert p[k].grad is not None and p[k].grad.shape == p[k].shape and bool((p[k].grad == 0).all()), k


def test_an_empty_batch_through_autograd_linear_gives_zero_gradients():
    """autograd.Linear.backward sends an empty batch down its unfused path, gemm_tn + colsum on NULL operands: the
    gradients of the weight and the bias are zeros (the entry points refused this before)"""
    from desco_amd import autograd as AG
    wt = torch.randn(64, 64).to(DEV).requires_grad_()
    bias = torch.randn(64).to(DEV).requires_grad_()
    a1 = torch.empty(0, 64, device=DEV, requires_grad=True)
    c = AG.Linear.apply(a1, None, wt, bias, ops.ACT_RELU, 0.0)
    assert tuple(c.shape) == (0, 64)
    c.backward(torch.empty(0, 64, device=DEV))
    assert tuple(wt.grad.shape) == (64, 64) and bool((wt.grad == 0).all())
    assert tuple(bias.grad.shape) == (64,) and bool((bias.grad == 0).all())
    assert tuple(a1.grad.shape) == (0, 64)


@pytest.mark.parametrize("n", (8, 48, 2048))
def test_rowdot_bwd_refuses_other_widths(n):
    with pytest.raises(RuntimeError, match="desco_rowdot_bwd_f32"):
        ops.rowdot_bwd(torch.zeros(4, n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(4, device=DEV))


def test_smallk_bwd_refuses_k_17():
    with pytest.raises(RuntimeError, match="desco_linear_smallk_bwd_f32"):
        ops.linear_smallk_bwd(torch.zeros(4, 17, device=DEV), torch.zeros(4, 64, device=DEV))
