"""tests/gemm_split_reference.py on the host, before any GPU is involved, on every case
tests/test_gemm_split_kernels_gpu.py runs:
  * the fp64 reference against an independent formula (a python loop over K, torch.nn.functional for the activations and
    their derivatives, the row classes by explicit row loops), so that it is not its own only witness; known wrong forms
    -- the row class taken modulo ws_rows + 1, a gate of +-0.0 counted as positive -- must differ;
  * ``mag`` bounds |ref| and is 0 exactly where the dropout factor or the gate derivative is;
  * the plane splits against their defining properties: hi + mid + lo reproduces the float bit for bit, the fp16 hi + lo
    is within 2^-22 of the scaled value, the nearest-even bf16 is torch's;
  * the gate of the GPU test (E_kernel <= 4 E_f32 and <= 1e-4 on the scale ``mag``, E_kernel over the m rows a launch
    computes, E_f32 over the case's parent) is reachable by the documented arithmetic: each mode's restated form
    (``emulate``) and a second fp32 summation order (one matmul per 32-wide K block, accumulated from the last block to
    the first) both stay within it;
  * the cases hold what they promise."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gemm_split_reference as G

CEILING = 1e-4


@pytest.mark.parametrize("name", ["epilogue desc n 64 gate drop tail", "epilogue desc n 128 gate relu drop tail relu",
                                  "epilogue f16x3 n 64 tail ns 3", "epilogue bf16 n 64 bias_rows 29",
                                  "epilogue desc n 192 gate slope -0.25 drop relu", "seam bf16x6 k (32, 96)",
                                  "linear64 m 63 n 128"])
def test_reference_equals_a_plain_loop_over_k(name):
    case = G.make(name)
    rows = 41                                                            # > 37: every row class wraps
    A = (case["a1"] if case["a2"] is None else torch.cat([case["a1"], case["a2"]], 1))[:rows]
    W = case["w"]
    if case["mode"] == "bf16":
        A, W = A.bfloat16().float(), W.bfloat16().float()                 # torch's nearest-even rounding
    A, W = A.double(), W.double()
    z = torch.zeros(rows, W.shape[0], dtype=torch.float64)
    for k in range(A.shape[1]):
        z += A[:, k:k + 1] * W[:, k][None, :]
    for r in range(rows):
        if case["bias"] is not None:
            b = case["bias"].double()
            z[r] += b if b.dim() == 1 else b[r % b.shape[0]]
        if case["s"] is not None:
            ws = case["ws"].double()
            for j in range(case["s"].shape[1]):
                z[r] += float(case["s"][r, j]) * ws[r % ws.shape[0], j]
    act = {"none": lambda t: t, "relu": F.relu, "leaky": lambda t: F.leaky_relu(t, case["slope"])}[case["act"]]
    f = G.factor(case)[:rows].double()
    d = torch.ones_like(z)
    if case["gate"] is not None:
        g = case["gate"][:rows].double().requires_grad_()
        {"relu": F.relu, "leaky": lambda t: F.leaky_relu(t, case["gate_slope"])}[case["gate_act"]](g).sum().backward()
        d = g.grad                                                       # torch's own derivative: 0 / slope at +-0.0
    want = act(z) * f * d
    ref, m = G.evaluate(case)[:rows], G.mag(case)[:rows]
    e, _ = G.scaled_error(ref, want, m)
    print(f"[parity] gemm_split reference vs loop over K, {name}: max |d| / mag = {e:.2e}")
    assert e <= 1e-12
    assert bool((m >= ref.abs() * (1 - 1e-12)).all()) and bool(((m == 0) == ((f == 0) | (d == 0))).all())
    # known wrong forms must show
    if case["s"] is not None and case["ws"].shape[0] > 1:
        wrong = dict(case, ws=torch.cat([case["ws"], case["ws"][:1]]))   # r % (ws_rows + 1)
        assert G.scaled_error(G.evaluate(wrong)[:rows], ref, m)[0] > CEILING
    if case["gate"] is not None:                                         # +-0.0 counted as positive
        low = 0.0 if case["gate_act"] == "relu" else case["gate_slope"]
        d0 = torch.where(case["gate"][:rows].double() >= 0, 1.0, low)
        assert G.scaled_error(act(z) * f * d0, ref, torch.maximum(m, G.mag(dict(case, gate=None))[:rows]))[0] > CEILING


def test_mag_bounds_the_reference_on_every_case():
    for name in G.CASES:
        case = G.make(name)
        ref, m = G.evaluate(case), G.mag(case)
        assert ref.shape == (max(case["m"], G.PARENT_ROWS), case["n"]) and torch.isfinite(m).all(), name
        assert bool((m >= ref.abs() * (1 - 1e-12)).all()), name
        dead = (G.factor(case) == 0) | (G.gate_derivative(case) == 0)
        if case["regime"] == "zero" and case["bias"] is None:
            dead = dead | ~case["a1"].any(1)[:, None]
        assert bool(((m == 0) == dead).all()) and not ref[dead].any(), name


def _specimens():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4096, generator=g) * 2.0 ** torch.randint(-60, 60, (4096,), generator=g).float()
    x[:8] = torch.tensor([0.0, 1.0, -1.0, 2.0 ** -100, -1.0 - 2.0 ** -23, 1.0 + 2.0 ** -8, 2.0 - 2.0 ** -23, 3.0e38])
    return x.numpy()                        # (no residual of the truncation split is an fp32 subnormal: those lose bits)


def test_the_plane_splits_hold_their_defining_properties():
    x = _specimens()
    hi, mid, lo = (G.bf16_value(p) for p in G.split_bf16x3(x))
    assert np.array_equal(((lo + mid) + hi).view(np.uint32), x.view(np.uint32))
    assert np.array_equal(hi.view(np.uint32), x.view(np.uint32) & np.uint32(0xffff0000))
    assert (np.abs(mid) <= np.abs(hi) * 2.0 ** -7).all() and (np.abs(lo) <= np.abs(hi) * 2.0 ** -15).all()
    t = torch.from_numpy(x)
    assert np.array_equal(G.round_bf16(x), t.bfloat16().view(torch.int16).numpy())
    assert np.array_equal(G.bf16_value(G.round_bf16(x)), t.bfloat16().float().numpy())
    # fp16 split: one power of two for the matrix, hi + lo within 2^-22 of the scaled value (2^-40 of the maximum below
    # the range of the split)
    for w in (x[:4000].reshape(40, 100) * np.float32(2.0 ** -20), np.zeros((3, 5), np.float32),
              np.array([[1.0, 2.0 ** -20, 3 * 2.0 ** -35, -2.0 ** -39]], np.float32), np.array([[3.0e38, 1.0, -2.0]], np.float32)):
        planes, sc = G.split_f16x2(w)
        assert planes.shape == (2,) + w.shape and planes.dtype == np.int16
        mx = np.abs(w).max()
        assert sc[0] * sc[1] == 1 and np.frexp(sc[0])[0] == 0.5 and (2.0 ** 14 <= mx * sc[0] < 2.0 ** 15 or mx == 0 and sc[0] == 1)
        v = w.astype(np.float64) * float(sc[0])
        hi, lo = (p.astype(np.float64) for p in planes.view(np.float16))
        assert (np.abs(hi + lo - v) <= np.maximum(np.abs(v) * 2.0 ** -22, 2.0 ** -25)).all()
    assert np.array_equal(G.pow2_scale(np.array([0, 1, 1.5, 2, 2.0 ** 14, 2.0 ** 15 - 1, 1e-45, 3e38], np.float32)),
                          np.array([1, 2.0 ** 14, 2.0 ** 14, 2.0 ** 13, 1, 1, 2.0 ** 126, 2.0 ** -113], np.float32))
    a1, a2 = x[:64].reshape(4, 16), -np.abs(x[64:96].reshape(4, 8))
    assert np.array_equal(G.row_absmax(a1, a2), np.abs(np.concatenate([a1, a2], 1)).max(1))


@pytest.mark.parametrize("name", list(G.CASES))
def test_the_documented_arithmetic_meets_the_gate(name):
    case = G.make(name)
    rows = slice(0, case["m"])
    ref, m = G.evaluate(case), G.mag(case)
    ef = G.scaled_error(G.evaluate(case, torch.float32), ref, m)[0]
    assert torch.isfinite(m).all() and ef < 1e-5 and (ef > 0 or not m.any())
    emu, rev = G.emulate(case), G.evaluate(case, torch.float32, order="blocks_reversed")
    for what, got in ((f"{case['mode']} emulation", emu), ("K blocks last to first", rev)):
        e = G.scaled_error(got[rows], ref[rows], m[rows])[0]
        print(f"[parity] gemm_split reference {name}, {what}: E {e:.2e}, E_f32 {ef:.2e}, ratio {e / ef if ef else 0:.2f} (gate 4)")
        assert e <= 4 * ef and e <= CEILING, what
    dead = m == 0
    assert not ref[dead].any() and not emu[dead].any() and not rev[dead].any()
    if case["regime"] == "zero":                                         # a zero row is act(bias), bit for bit
        z = ~case["a1"].any(1) if case["a2"] is None else ~(case["a1"].any(1) | case["a2"].any(1))
        assert 0.2 < float(z.float().mean()) < 0.4
        want = torch.zeros(case["n"]) if case["bias"] is None else case["bias"]
        assert torch.equal(emu[z], want.expand(int(z.sum()), -1)) and torch.equal(ref[z], want.double().expand(int(z.sum()), -1))


def test_the_cases_hold_what_they_promise():
    C = G.CASES
    assert {n.split()[0] for n in C} == {"instantiation", "rows", "seam", "regime", "store", "epilogue", "linear64"}
    assert {G.family(n) for n in C} == {"bf16x6", "bf16", "f16x3", "desc epilogue", "linear64"}
    for mode in G.MODES:
        mine = {n: c for n, c in C.items() if c["mode"] == mode and c.get("entry", "gemm") == "gemm"}
        fam = lambda w: [c for n, c in mine.items() if n.split()[0] == w]                    # noqa: E731
        assert {c["n"] for c in fam("instantiation")} == {64, 128, 192, 256, 320, 384}
        assert all((c["m"], c["k1"] + c.get("k2", 0)) == (129, 96) for c in fam("instantiation"))
        assert {c["m"] for c in fam("rows")} == set(G.ROW_EDGES) | {1025, 1153}
        assert {(c["k1"], c.get("k2", 0)) for c in fam("seam")} == set(G.SEAMS) | {(576, 0)}
        assert any((c["m"], c["n"], c["k1"]) == (300, 576, 576) for c in fam("seam"))
        assert sum(bool(c.get("a1_contig")) for c in fam("seam")) == 1
        assert {(c["regime"], c["m"], c["n"], c["k1"] + c.get("k2", 0)) for c in fam("regime")} == \
            {(r, *s) for r in G.REGIMES for s in ((129, 64, 128), (257, 192, 192))}
        assert {(c["store"], c["n"]) for c in fam("store")} == {(s, n) for s in G.STORES for n in (64, 192)}
        assert {c["store"] for c in mine.values()} == set(G.STORES)
    desc = {n: c for n, c in C.items() if c.get("entry") == "desc"}
    for n_ in G.EPILOGUE_N:
        d = [c for c in desc.values() if c["n"] == n_]
        assert all(c["m"] == 333 and c["mode"] == "bf16x6" for c in d)
        assert {c.get("bias_rows", 1) for c in d} >= {1, 29}
        assert {(c["ns"], c["ws_rows"]) for c in d if c.get("ns")} >= {(a, b) for a in (1, 3, 4) for b in (1, 29, 37)}
        assert {c.get("act", "none") for c in d} == set(G.ACTS)
        assert {(c.get("gate"), c.get("drop_p"), bool(c.get("ns"))) for c in d} >= {
            ("relu", None, False), ("leaky", None, False), (None, 0.3, False), (None, 1.0, False), ("leaky", 0.3, True)}
        for mode in ("f16x3", "bf16"):
            e = [c for n, c in C.items() if n.startswith(f"epilogue {mode} n {n_} ")]
            assert {c.get("bias_rows", 1) for c in e} >= {1, 29} and {c.get("ns", 0) for c in e} >= {1, 3, 4}
    lin = [c for c in C.values() if c.get("entry") == "linear64"]
    assert {(c["m"], c["n"]) for c in lin} == {(a, b) for a in G.LINEAR64_M for b in G.LINEAR64_N}
    assert {c["act"] for c in lin} == set(G.ACTS) and {c["bias_rows"] for c in lin} == {0, 1}
    gate = G.make("epilogue desc n 64 gate leaky")["gate"][:333]
    zero = gate == 0
    assert bool((zero & ~torch.signbit(gate)).any()) and bool((zero & torch.signbit(gate)).any()) and bool((gate < 0).any())
    a = G.make("regime bf16x6 range (129, 64, 128)")["a1"].abs().amax(1)[:129]
    assert a.max() / a.min() > 2.0 ** 24
    a = G.make("regime f16x3 inrow (129, 64, 128)")["a1"].abs()
    assert a[:, 0::2].max() < a[:, 1::2].max() * 2.0 ** -18


def test_the_routing_probe_is_exact_in_every_mode():
    """the probe's expected values are what the restated arithmetic of every mode gives, bit for bit"""
    for mode in G.MODES:
        for n in (64, 192):
            for K in (32, 96):
                A, W, want = G.routing_case(mode, n, K)
                assert sorted(set(((5 * np.arange(129) + 3) % K).tolist())) == list(range(K))
                assert np.array_equal(G.ACCUMULATE[mode](A.numpy(), W.numpy()), want.numpy()), (mode, n, K)
                assert torch.equal(A.double() @ W.double().t(), want.double())
                if mode != "bf16":
                    assert W.unique().numel() == n * K
