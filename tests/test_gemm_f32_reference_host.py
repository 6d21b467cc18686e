"""tests/gemm_f32_reference.py held to what it claims, on the CPU: ``fma32`` is libm's fmaf (and the naive float64 form is
not); the restated split formulas are the library's workspace functions (host calls, nothing is launched); the gate of
tests/test_gemm_f32_kernels_gpu.py is reachable on every named case by the ordered float32 evaluation alone; and known
wrong evaluators break bit-equality -- and, unless they merely reorder a sum, the gate -- on a named case.

A mutation that only reorders (a slab boundary moved by 32 rows, the 16 bias groups folded in reverse) computes the same
sum in another order: it is EXPECTED to stay inside any honest tolerance.  That is the reason the GPU test asserts
bit-equality and not the gate alone; for those two only the broken bits are asserted here."""
import ctypes
import ctypes.util

import numpy as np
import pytest

import gemm_f32_reference as G
from desco_amd import _lib

F32 = np.float32


# ---- fma32 is fmaf ------------------------------------------------------------------------------------------------------------
def _fmaf():
    m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    m.fmaf.restype = ctypes.c_float
    m.fmaf.argtypes = [ctypes.c_float] * 3
    return m.fmaf


def test_fma32_is_libm_fmaf():
    """120 000 triples whose three exponents are drawn independently over +-30, 40 000 more with c within a few ulps of
    -a b (cancellation: the rounding error of the float64 sum decides), and the constructed double-rounding triple"""
    rng = np.random.default_rng(1)

    def draw(count):
        return (rng.uniform(1, 2, count) * rng.choice([-1.0, 1.0], count) * 2.0 ** rng.integers(-30, 31, count)).astype(F32)
    a, b, c = draw(120000), draw(120000), draw(120000)
    a2, b2 = draw(40000), draw(40000)
    c2 = -(a2 * b2)
    c2 = (c2.view(np.int32) + rng.integers(-3, 4, 40000).astype(np.int32)).view(F32)
    a, b, c = np.concatenate([a, a2]), np.concatenate([b, b2]), np.concatenate([c, c2])
    fmaf = _fmaf()
    want = np.array([fmaf(x, y, z) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())], F32)
    got = G.fma32(a, b, c)
    bad = np.flatnonzero(got.view(np.int32) != want.view(np.int32))
    assert bad.size == 0, f"{bad.size} mismatches, first: {a[bad[0]]!r} {b[bad[0]]!r} {c[bad[0]]!r}"


def test_the_naive_float64_form_rounds_twice():
    a, b, c = (F32(v) for v in G.DOUBLE_ROUNDING_TRIPLE)
    assert float(a) == G.DOUBLE_ROUNDING_TRIPLE[0] and float(c) == G.DOUBLE_ROUNDING_TRIPLE[2]     # representable
    want = _fmaf()(float(a), float(b), float(c))
    assert want == float(c)
    assert float(G.fma32(a, b, c)) == want
    assert float(G.fma32_naive(a, b, c)) == float(c) + 2.0 ** 7      # the emulation is needed


def test_fma32_broadcasts_like_a_chain_step():
    a, b, c = np.ones((3, 1), F32), np.full((1, 4), 2, F32), np.zeros((3, 4), F32)
    out = G.fma32(a, b, c)
    assert out.shape == (3, 4) and out.dtype == F32 and (out == 2).all()


# ---- the restated split formulas ------------------------------------------------------------------------------------------------
KN = ((64, 64), (128, 64), (64, 128))


def _case_ms():
    ms = set()
    for name in G.family("tn") + G.family("bwdw"):
        ms.add(G.make(name)["m"])
    return sorted(ms | {140001, 262145, 131073})


def test_split_formulas_are_the_library_workspace_functions():
    L = _lib.lib()
    splits = ctypes.c_int(0)
    for k, n in KN + ((192, 128), (192, 64)):
        for m in list(range(0, 3001)) + _case_ms():
            nb = L.desco_gemm_tn_workspace(m, k, n, ctypes.byref(splits))
            assert (splits.value, nb) == (G.tn_splits(m, k, n)[0], G.tn_workspace_bytes(m, k, n)), (m, k, n)
            assert L.desco_linear_bwd_w_workspace(m, k, n) == G.bwdw_workspace_bytes(m, k, n), (m, k, n)
    for m, k, n in ((513, 64, 64), (1025, 128, 64), (257, 64, 64), (1000, 192, 128)):
        for s, slab in (G.tn_splits(m, k, n), G.bwdw_splits(m, k, n)):
            assert slab % 32 == 0 and slab >= 32 and s * slab >= m


def test_multi_workspace_is_the_sum_of_the_problems():
    L = _lib.lib()
    names = [G.family("bwdw")[i] for i in G.BWDW_MULTI]
    descs = (_lib.BwdWDesc * len(names))()
    total = 0
    for d, name in zip(descs, names):
        c = G.make(name)
        d.k1, d.k2 = c["a1"].shape[1], 0 if c["a2"] is None else c["a2"].shape[1]
        d.m, d.n = c["m"], c["dz"].shape[1]
        total += G.bwdw_workspace_bytes(d.m, d.k1 + d.k2, d.n)
    assert len(names) == 16 and sum(G.make(n)["m"] == 0 for n in names) == 2
    assert L.desco_linear_bwd_w_multi_workspace(len(names), descs) == total


def test_row_slabs_cover_every_row():
    for cap in (512, 1024):
        for m in list(range(0, 1500)) + [140001, 131073, 262145]:
            s, slab = G.rows_splits(m, cap)
            assert 1 <= s <= cap and slab >= 1 and s * slab >= m          # (the last slabs may be empty: 511 * 274 > 140 001)
    assert G.rows_splits(140001, 512) == (512, 274) and G.rows_splits(262145, 1024) == (1024, 257)


# ---- the gate is reachable ------------------------------------------------------------------------------------------------------
ALL = list(G.CASES)


@pytest.mark.parametrize("name", ALL)
def test_the_ordered_float32_evaluation_is_inside_the_gate(name):
    """E_f32 <= 1e-4 (a kernel that IS the ordered evaluation passes E_kernel <= 4 E_f32 and the ceiling), zero where mag
    is zero, the float64 evaluation finite, every non-zero result inside the float32 normal range by a wide margin, and
    for the contractible terms the unfused and the fma32 evaluation within the gate of each other's figure"""
    case, ref, mg, f32, ef = G.host(name)
    for k in ref:
        assert np.isfinite(ref[k]).all() and f32[k].dtype == F32 and f32[k].shape == ref[k].shape
        assert ef[k] <= G.CEILING / 4, (k, ef[k])
        assert (f32[k][mg[k] == 0] == 0).all()
        nz = np.abs(f32[k][f32[k] != 0])
        assert nz.size == 0 or (nz.min() >= 2.0 ** -100 and nz.max() <= 2.0 ** 60)
        if not G.is_pinned(case, k):
            for fused in (False, True):
                e = G.scaled_error(G.evaluate(case, F32, fused=fused)[k], ref[k], mg[k])[0]
                assert e <= 4 * ef[k]


def test_every_named_edge_is_a_case():
    names = " | ".join(ALL)
    for edge in ("bwdw m = 257,", "tn m = 513,", "colsum m = 257, n = 29", "misaligned parent[:, 1:65]", "ldc = n + 3",
                 "gemm m = 33, k = (32, 32), n = 64, bias_rows = 7", "drop m = 5,", "colsum m = 140001, n = 29",
                 "rowdot R = 262145, n = 16", "smallk m = 131073", "gemm m = 32, k = (32, 0), n = 64, bias_rows = none"):
        assert edge in names, edge
    assert any(None in launch[1:-1] for launch in G.MULTI_LAUNCHES)              # an m = 0 product in the middle
    kinds = {G.colsum_kernel(G.make(n)) for n in G.family("colsum")}
    assert kinds == {"scalar", "partial4"}
    assert G.colsum_kernel(G.make("colsum m = 17, n = 64, misaligned parent[:, 1:65]")) == "scalar"
    assert G.colsum_kernel(G.make("colsum m = 17, n = 64, ldx = 65")) == "scalar"
    assert G.colsum_kernel(G.make("colsum m = 17, n = 64")) == "partial4"


# ---- mutations must fail --------------------------------------------------------------------------------------------------------
def _names(word, pred):
    return [n for n in G.family(word) if pred(G.make(n))]


def _mutation_cases():
    big = lambda c: c["kind"] == "gemm" and c["s"] is None
    return {
        # mutation: (cases, output, only a reordering)
        "drop_last_row": (["tn m = 513, k = 64, n = 64, out rowblock", "bwdw m = 257, k = (64, 0), n = 64",
                           "colsum m = 257, n = 29", "colsum m = 257, n = 64", "bwdw m = 33, k = (128, 64), n = 64, a1 column block"],
                          None, False),
        "slab_shift": (["tn m = 513, k = 64, n = 64, out rowblock", "tn m = 1025, k = 128, n = 64, out rowblock",
                        "bwdw m = 257, k = (64, 0), n = 64", "bwdw m = 1000, k = (128, 64), n = 128"], None, True),
        "skip_chunk": (_names("gemm", lambda c: big(c) and c["m"] in (32, 33, 129)), "c", False),
        "swap_segments": (_names("gemm", lambda c: big(c) and c["a2"] is not None and c["m"] in (1, 33, 128)), "c", False),
        "bias_row_off": (_names("gemm", lambda c: big(c) and c["bias"] is not None and c["bias"].shape[0] > 1
                                and c["m"] in (31, 33, 257)), "c", False),
        "transpose_block": (_names("gemm", lambda c: big(c) and c["m"] in (32, 33, 129)), "c", False),
        "row_block_shift": (_names("gemm", lambda c: big(c) and c["m"] in (33, 127, 257)), "c", False),
        "bias_groups_reversed": (["bwdw m = 33, k = (128, 64), n = 64, a1 column block", "bwdw m = 257, k = (64, 0), n = 64",
                                  "bwdw m = 300, k = (64, 64), n = 64"], "dbias", True),
        "gate_ge": (_names("mprod", lambda c: c["gate"] is not None), "c", False),
        "remainder_skip": (["colsum m = 17, n = 64", "colsum m = 65, n = 256", "colsum m = 1000, n = 100",
                            "colsum m = 140001, n = 64"], "out", False),
    }


@pytest.mark.parametrize("mutation", list(_mutation_cases()))
def test_a_wrong_evaluator_breaks_the_bits_and_the_gate(mutation):
    """the last row of a slab dropped, a slab boundary moved by 32, one K chunk of 32 skipped, the a1 / a2 segments
    swapped, the bias row index off by one, the output transposed within a 32 x 32 block, a row block of the A tile read
    one row up (r1 = r0 + 31), the 16 bias groups folded in reverse, the gate read with >= (+-0.0 pass), the remainder
    loop of colsum_partial4_kernel started 16 rows late: bits differ on every listed case; outside the gate on at least
    one, unless the mutation only reorders"""
    names, key, reorder_only = _mutation_cases()[mutation]
    assert names
    outside = 0
    for name in names:
        case, ref, mg, f32, ef = G.host(name)
        mut = G.evaluate(case, F32, mutate=mutation)
        keys = [key] if key else list(ref)
        assert any(not G.same_bits(mut[k], f32[k]) for k in keys), f"{mutation} leaves the bits of {name}"
        for k in keys:
            e = G.scaled_error(mut[k], ref[k], mg[k])[0]
            exact = bool((mut[k][mg[k] == 0] == 0).all())
            outside += (e > 4 * ef[k]) or (e > G.CEILING) or not exact
            print(f"[mutation] {mutation}, {name}, {k}: E {e:.3e} against E_f32 {ef[k]:.3e}")
    assert reorder_only or outside, f"{mutation} stays inside the gate on all of {names}"


def test_a_dropout_quad_from_the_tile_relative_row_is_caught():
    """the quad index from the row within its 128-row tile: the same factors up to row 127, others from row 128 on --
    m = 130 is the case that sees it, m = 1, 3, 5 cannot"""
    seen = {}
    for name in G.family("drop"):
        case, ref, mg, f32, ef = G.host(name)
        wrong = G.quad_factor(case["m"], case["n"], case["drop"], F32(1.0 / (1.0 - case["drop"])), tile_relative=True)
        mut = G.evaluate(case, F32, fac=wrong)["c"]
        seen[name] = not G.same_bits(mut, f32["c"])
        if case["m"] == 130:
            assert (wrong[:128] == case["fac"][:128]).all() and (wrong[128:] != case["fac"][128:]).any()
            assert G.scaled_error(mut, ref["c"], mg["c"])[0] > 4 * ef["c"]
    assert all(seen[n] == (G.make(n)["m"] == 130) for n in seen), seen
