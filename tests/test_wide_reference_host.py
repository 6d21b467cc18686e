"""tests/wide_reference.py on the host, before any GPU is involved, on every case tests/test_wide_kernels_gpu.py runs:
  * the fp64 reference against a dense evaluation of the same contract (the [N vslots, N] incidence matrix of the CSR,
    then matmuls; no ``index_add_``), so that it is not its own only witness; the dense form with two slots exchanged,
    and with the self block left out, must differ;
  * the gate of the GPU test (E_kernel <= 4 E_f32 and <= 1e-4 on the scale ``mag``, over the rows a launch computes) is
    reachable by the documented arithmetic: the kernel's restated f16x3 form (``emulate_f16x3``) and a second fp32
    summation order (one matmul per block, accumulated from the last block to the first) both stay within it;
  * where ``mag`` is 0 the reference and the emulation are exactly 0; a row with x == 0 and no source is relu(bias);
  * the cases hold what they promise: every degree 0..9, hubs, empty virtual rows, edges in the slots a launch must not
    read, sources on both sides of the range."""
import numpy as np
import pytest
import torch

import wide_reference as W

CEILING = 1e-4


def _rows(case):
    return slice(case["row0"], case["row0"] + case["num_rows"])


def _incidence(case):
    """[N vslots, N] float64: entry (v, j) = how often virtual row v reads row j"""
    vrowptr, vcol = case["vrowptr"].numpy(), case["vcol"].numpy()
    N = case["x"].shape[0]
    inc = np.zeros((len(vrowptr) - 1, N))
    for v in range(len(vrowptr) - 1):
        for e in range(vrowptr[v], vrowptr[v + 1]):
            inc[v, vcol[e]] += 1
    return torch.from_numpy(inc)


def _dense(case, inc, swap=False, self_block=True):
    x, Wt, bias = case["x"].double(), case["Wt"].double(), case["bias"].double()
    N, wp = x.shape
    S, vs = case["slots"], case["vslots"]
    order = [1, 0] + list(range(2, S)) if swap else list(range(S))
    A = torch.cat([inc[s::vs] @ x for s in order] + [x if self_block else torch.zeros_like(x)], 1)
    return torch.relu(A @ Wt + bias)


@pytest.mark.parametrize("name", list(W.CASES))
def test_reference_equals_the_dense_incidence_matrix_formula(name):
    case = W.make(name)
    inc, ref, m = _incidence(case), W.evaluate(case), W.mag(case)
    e, _ = W.scaled_error(ref, _dense(case, inc), m)
    print(f"[parity] wide reference vs dense incidence formula, {name}: max |d| / mag = {e:.2e}")
    assert ref.shape == case["x"].shape and e <= 1e-12
    e, _ = W.scaled_error(W.gather(case), inc @ case["x"].double(), W.gather(case, absolute=True))
    assert e <= 1e-12
    # known wrong forms must show
    r = _rows(case)
    assert W.scaled_error(_dense(case, inc, self_block=False)[r], ref[r], m[r])[0] > CEILING
    if case["vcol"].numel():
        assert W.scaled_error(_dense(case, inc, swap=True)[r], ref[r], m[r])[0] > CEILING


@pytest.mark.parametrize("name", list(W.CASES))
def test_the_documented_arithmetic_meets_the_gate(name):
    case = W.make(name)
    r = _rows(case)
    ref, m = W.evaluate(case)[r], W.mag(case)[r]
    f32 = W.evaluate(case, torch.float32)[r]
    emu, rev = W.emulate_f16x3(case)[r], W.evaluate(case, torch.float32, order="blocks_reversed")[r]
    ef = W.scaled_error(f32, ref, m)[0]
    assert torch.isfinite(m).all() and torch.isfinite(f32).all() and 0 < ef < 1e-5
    for what, got in (("f16x3 emulation", emu), ("blocks last to first", rev)):
        e = W.scaled_error(got, ref, m)[0]
        print(f"[parity] wide reference {name}, {what}: E {e:.2e}, E_f32 {ef:.2e}, ratio {e / ef:.2f} (gate 4)")
        assert e <= 4 * ef and e <= CEILING, what
    # exactly 0 where no term exists; the bound is not trivially true elsewhere
    dead = m == 0
    assert not ref[dead].any() and not emu[dead].any() and not f32[dead].any()
    H = case["H"]
    if H is not None:
        assert dead[:, H:].all() and not dead[:, :H].any() and (ref[:, :H] > 0).any()
    else:
        assert not dead.any()
    for i in case["bare"]:
        want = torch.relu(case["bias"])
        assert torch.equal(W.evaluate(case)[i], want.double()) and torch.equal(W.emulate_f16x3(case)[i], want)


def test_the_cases_hold_what_they_promise():
    fam = {n.split()[0] for n in W.CASES}
    assert fam == {"instantiation", "range", "arguments", "outputs", "degrees", "regime", "padding"}
    assert {(c["wp"], c["S"]) for c in W.CASES.values()} >= {(w, s) for w in W.WIDTHS for s in W.SLOTS}
    assert {(c.get("row0", 37), c.get("num_rows", 203)) for n, c in W.CASES.items() if n.startswith("range")} == set(W.RANGES)
    for name in W.CASES:
        case = W.make(name)
        N, vs, S, r0, n = case["x"].shape[0], case["vslots"], case["slots"], case["row0"], case["num_rows"]
        deg = (case["vrowptr"][1:] - case["vrowptr"][:-1]).view(N, vs)
        assert N == r0 + n + W.TAIL
        if not case["vcol"].numel():
            assert name.startswith("degrees empty vcol")
            continue
        used = deg[r0:r0 + n, :S]
        if n >= 63:
            assert set(range(10)) <= set(used.flatten().tolist()), name          # the tail of the four-wide loop
            assert 0.2 < float((used == 0).float().mean()) < 0.45, name
            hubs = sorted(d for d in used.flatten().tolist() if d > 9)
            assert hubs == sorted(W.HUBS) and all(d % 4 for d in hubs), name
        if vs > S:
            assert (deg[:, S:] > 0).any(), name                                  # the slots a launch must not read
        src = case["vcol"]
        assert (src >= r0 + n).any() and (r0 == 0 or (src < r0).any()), name      # sources outside the range
        if case["regime"] == "zero":
            z = ~case["x"].any(1)
            assert 0.2 < float(z.float().mean()) < 0.4 and len(case["bare"]) == 3
            assert all(z[i] and not deg[i].any() for i in case["bare"])
            agg = W.gather(case, absolute=True).view(N, vs, -1)[r0:r0 + n, :S]
            assert ((agg.amax(2) == 0) & (used > 0)).any(), name                  # an all-zero block that has sources
        if case["regime"] == "range":
            a = case["x"].abs().amax(1)[r0:r0 + n]
            assert a.max() / a.min() > 2.0 ** 28
        if case["regime"] == "block":
            b = torch.stack([t[r0:r0 + n].abs().amax(1) for t in W.blocks(case)], 1)          # [n, S + 1]
            live = (b > 0).all(1)
            assert (b[live].amax(1) / b[live].amin(1)).max() > 2.0 ** 18


@pytest.mark.parametrize("width", W.GATHER_WIDTHS)
def test_the_fp32_gather_in_csr_order(width):
    """``gather`` in float32 (the value csr_gather_sum_wide must reproduce bit for bit) against float64 and against a
    plain loop over the edges"""
    for slots in W.GATHER_SLOTS:
        for n in W.GATHER_ROWS:
            x, vrowptr, vcol = W.gather_case(width, slots, n, seed=width + 7 * slots + n)
            g32, g64, m = W.gather((x, vrowptr, vcol), torch.float32), W.gather((x, vrowptr, vcol)), \
                W.gather((x, vrowptr, vcol), absolute=True)
            assert g32.shape == (n * slots, width) and g32.dtype == torch.float32
            e, _ = W.scaled_error(g32, g64, m)
            assert e < 1e-5
            loop = np.zeros((n * slots, width), np.float32)
            xn = x.numpy()
            for v in range(n * slots):
                for e_ in range(int(vrowptr[v]), int(vrowptr[v + 1])):
                    loop[v] = loop[v] + xn[int(vcol[e_])]
            assert np.array_equal(loop, g32.numpy())
    x, vrowptr, vcol = W.gather_case(width, 2, 5, edges=False)
    assert not vcol.numel() and not W.gather((x, vrowptr, vcol), torch.float32).any()
