"""tests/pool_reference.py on the host, before any GPU is involved, on every case tests/test_pool_kernels_gpu.py runs:
  * ``slots_of`` (the slot layout read off the enumeration of the (tile, segment) pairs) gives the pool_bits / pool_slot
    arrays of NeighborhoodBatch.pool_index() (bits and running counts) on every layout;
  * the fp64 reference against a dense evaluation of the same contract (the [B, num_slots] 0/1 incidence matrix times
    the partial arrays, then matmuls), so that it is not its own only witness;
  * known wrong slot decodes and wrong placements of the rows x0 term exceed the ceiling on sweep33;
  * the gate of the GPU test (E_kernel <= 4 E_f32 and <= 1e-4 on the scale ``mag``) is reachable by the documented
    arithmetic: the kernels' restated form (``emulate``) and a second fp32 summation order both stay within it;
  * where ``mag`` is 0 the reference, the fp32 evaluation and the emulation are exactly 0; the fp32 ``reduce`` gives the
    same bits twice;
  * ``tile_partials`` in float32 (what the producers are held to) is the running sum in row order of a plain loop;
  * the cases hold what they promise."""
import functools

import numpy as np
import pytest
import torch

import pool_reference as P

CEILING = 1e-4


@functools.lru_cache(maxsize=None)
def _host(name):
    """(case, fp64 reference, mag, fp32 evaluation), computed once per case"""
    case = P.make(name)
    return case, P.evaluate(case), P.mag(case), P.evaluate(case, torch.float32)


def _incidence(case):
    inc = torch.zeros(len(case["seg_slots"]), case["num_slots"], dtype=torch.float64)
    for b, s in enumerate(case["seg_slots"]):
        inc[b, s] = 1
    return inc


def _lk(z, case):
    return P._act(z, case["act"], case["slope"])


def _dense(case, layer=0):
    if "draws" in case:
        return torch.cat([_dense(d, layer) for d in case["draws"]])
    inc = _incidence(case)
    if case["kind"] == "reduce":
        out = inc @ case["parts"][layer].double()
        return out if case["extra"] is None else out + case["extra"].double()
    rows = (case["seg_ptr"][1:] - case["seg_ptr"][:-1]).double()
    add = torch.cat([rows[:, None] * case["x0"].double()[None, :]] + [inc @ p.double() for p in case["parts"]], 1)
    if case["kind"] == "post":
        anch = case["anch"].double()
    else:
        anch = _lk(case["a"].double() @ case["Wa"].double().t() + case["ba"].double(), case)
    z = (anch + add) @ case["W0"].double().t()
    return _lk(z if case["b0"] is None else z + case["b0"].double(), case)


# ---- the slot layout ------------------------------------------------------------------------------------------------
def _pool_index(seg_ptr):
    from desco_amd.batch import NeighborhoodBatch

    class _P:           # the slice of NeighborhoodPartition that NeighborhoodBatch.pool_index reads
        count_ptr = np.asarray(seg_ptr, np.int32)
    nb = NeighborhoodBatch.__new__(NeighborhoodBatch)
    nb.part, nb.device = _P, torch.device("cpu")
    bits, slot, ns = nb.pool_index()
    return bits.numpy().view(np.uint32), slot.numpy(), ns


@pytest.mark.parametrize("name", P.LAYOUTS)
def test_slot_layout_equals_pool_index(name):
    sp = P.seg_ptr_of(P.layout(name))
    seg_slots, ns, (bits, slot) = P.slots_of(sp, int(sp[-1]))
    pb, ps, pn = _pool_index(sp)
    assert ns == pn and np.array_equal(bits, pb) and np.array_equal(slot, ps)
    assert sorted(s for l in seg_slots for s in l) == list(range(ns))           # every slot belongs to one segment
    # a trailing empty segment (the post kernels' cases; pool_index itself refuses it) changes nothing
    spe = P.seg_ptr_of(P.layout(name), trailing_empty=True)
    se, nse, (be, sle) = P.slots_of(spe, int(spe[-1]))
    assert se == seg_slots + [[]] and nse == ns and np.array_equal(be, bits) and np.array_equal(sle, slot)


def test_the_layouts_hold_what_they_promise():
    T = P.TILE
    lens = P.layout("sweep33")
    sp = P.seg_ptr_of(lens)
    seen = {(int(n), int(s) % T) for n, s in zip(lens[1::2], sp[1:-1:2])}
    assert seen == {(n, f) for n in range(1, 34) for f in range(T)} and len(seen) == 528
    assert lens.max() == 33 and 1 <= lens[0::2].min() and lens[0::2].max() <= T
    assert 1000 <= len(lens) <= 1100 and 13000 <= int(sp[-1]) <= 15000
    seg_slots = P.slots_of(sp, int(sp[-1]))[0]
    assert {len(s) for s in seg_slots} == {1, 2, 3}
    lens = P.layout("ones")
    sp = P.seg_ptr_of(lens)
    _, ns, (bits, slot) = P.slots_of(sp, 300)
    assert len(lens) == 300 and ns == 300 and (bits[:-1] == 0xFFFF).all() and bits[-1] == (1 << 300 % T) - 1
    assert max(bin(int(b) & ((1 << f) - 1)).count("1") for b in bits[:-1] for f in range(T)) == 15
    lens = P.layout("ragged")
    sp = P.seg_ptr_of(lens)
    n = int(sp[-1])
    assert n % T and sp[-2] < (n // T) * T and 1 <= lens.min() and lens.max() <= 33        # last tile: one carried-in segment
    assert P.layout("single33").tolist() == [33] and P.layout("single1").tolist() == [1]
    lens = P.layout("long")
    sp = P.seg_ptr_of(lens)
    assert lens.tolist() == [1, 1000, 16, 17, 3000, 5, 48]
    assert max(len(s) for s in P.slots_of(sp, int(sp[-1]))[0]) >= 188
    for name in P.POST_LAYOUTS:
        sp = P.seg_ptr_of(P.layout(name))
        assert max(len(s) for s in P.slots_of(sp, int(sp[-1]))[0]) <= 3, name


def _check_draw(name, kw, case, m, seen):
    B, L = len(case["seg_slots"]), len(case["parts"])
    a = case["anch" if kw["kind"] == "post" else "a"]
    seen.add((kw["kind"], L, a.shape[1] // 64 - L, kw["layout_name"], kw["regime"]))
    seen.add((kw["kind"], L, a.shape[1] // 64 - L, kw["act"], kw["bias"]))
    assert not case["seg_slots"][-1] and all(case["seg_slots"][:-1]), name     # one trailing empty segment
    if kw["kind"] == "anchor":
        assert torch.equal(case["row_scale"], a.abs().amax(1)), name
    if kw["regime"] == "rows_pm16" and B > 100:
        assert a.abs().amax(1).max() / a.abs().amax(1).min() > 2.0 ** 28, name
    if kw["regime"] == "zeros":
        z = case["zero_rows"]
        assert z and z[0] == 0 and not a[z].any() and (B < 100 or 0.2 < len(z) / B < 0.4), name
        assert case["b0"] is None and not case["x0"].any() and (kw["kind"] == "post" or not case["ba"].any())
        assert not m[z].any() and m[[b for b in range(B) if b not in z]].all(), name
    else:
        assert m.all(), name
    if kw["regime"] == "cancel":
        multi = [s for s in case["seg_slots"] if len(s) > 1]
        assert multi or case["layout"] in ("ones", "single1"), name
        for s in multi:
            for p in case["parts"]:
                ratio = p[s].double().sum(0).abs() / p[s].double().abs().sum(0)
                assert 2.0 ** -14 < ratio.min() and ratio.max() < 2.0 ** -12, name
    return B


def test_the_cases_hold_what_they_promise():
    assert {n.split()[0] for n in P.CASES} == {"reduce", "multi", "post", "anchor"}
    seen = set()
    for name, (fn, kw) in P.CASES.items():
        if fn is P.reduce_case:
            continue
        whole = _host(name)[0]
        assert len(P.draws_of(whole)) == (P.SINGLE_DRAWS if kw["layout_name"].startswith("single") else 1), name
        row0 = 0
        for case in P.draws_of(whole):
            row0 = _check_draw(name, kw, case, _host(name)[2][row0:row0 + len(case["seg_slots"])], seen) + row0
    for kind, Ls, kbs in (("post", P.POST_L, (1,)), ("anchor", P.ANCHOR_L, (0, 1))):
        for L in Ls:
            for kb in kbs:
                for lay in P.POST_LAYOUTS:
                    for reg in P.REGIMES:
                        assert (kind, L, kb, lay, reg) in seen, (kind, L, kb, lay, reg)
                for act in (P.ACT_NONE, P.ACT_RELU, P.ACT_LEAKY):
                    for bias in (False, True):
                        assert (kind, L, kb, act, bias) in seen, (kind, L, kb, act, bias)


# ---- the reference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(P.CASES))
def test_reference_equals_the_dense_incidence_matrix_formula(name):
    case, ref, m, _ = _host(name)
    e, _ = P.scaled_error(ref, _dense(case), m)
    print(f"[parity] pool reference vs dense incidence formula, {name}: max |d| / mag = {e:.2e}")
    assert ref.shape == (sum(len(d["seg_slots"]) for d in P.draws_of(case)), 64) and e <= 1e-12
    for layer in range(1, len(case["parts"]) if case["kind"] == "reduce" else 0):
        assert P.scaled_error(P.evaluate(case, layer=layer), _dense(case, layer), P.mag(case, layer))[0] <= 1e-12
    if case["kind"] == "reduce" or case["layout"] != "sweep33":
        return
    # the producers' partial rows: the slot of a (tile, segment) pair holds the sum of its rows
    rows = torch.randn(int(case["seg_ptr"][-1]), 8, generator=torch.Generator().manual_seed(1))
    part = P.tile_partials(rows, case["seg_ptr"])
    seg = torch.repeat_interleave(torch.arange(len(case["seg_slots"])), case["seg_ptr"][1:] - case["seg_ptr"][:-1])
    tot = torch.zeros(len(case["seg_slots"]), 8, dtype=torch.float64).index_add_(0, seg, rows.double())
    assert P.scaled_error(_incidence(case) @ part, tot, P.reduce(P.tile_partials(rows, case["seg_ptr"], absolute=True),
                                                                  case["seg_slots"]))[0] <= 1e-12


def _wrong_slot_lists(case):
    """the slot lists of three wrong decodes of pool_bits / pool_slot"""
    ns, tile_slot, sp = case["num_slots"], case["slot"], case["seg_ptr"]
    good = case["seg_slots"]
    return {
        "a carried-in segment reads slot + 1": [s[:1] + [min(v + 1, ns - 1) for v in s[1:]] for s in good],
        "the third tile's slot is ignored": [s[:2] for s in good],
        "the first slot without the popcount offset": [([int(tile_slot[int(sp[b]) // P.TILE])] + s[1:]) if s else s
                                                       for b, s in enumerate(good)],
    }


@pytest.mark.parametrize("name", ["reduce sweep33", "multi 8 layers sweep33", "post L 3 sweep33 o1 leaky bias",
                                  "anchor L 5 k 320 sweep33 o1 leaky bias", "anchor L 8 k 576 sweep33 o1 relu bias"])
def test_wrong_forms_exceed_the_ceiling(name):
    case, ref, m, _ = _host(name)
    forms = {k: dict(seg_slots=v) for k, v in _wrong_slot_lists(case).items()}
    if case["kind"] != "reduce":
        forms["the rows x0 term is dropped"] = dict(x0_term="none")
        forms["the rows x0 term is added to block 1"] = dict(x0_term="block 1")
    for what, kw in forms.items():
        e = P.scaled_error(P.evaluate(case, **kw), ref, m)[0]
        print(f"[parity] pool reference {name}, wrong form ({what}): E {e:.2e} (ceiling {CEILING:.0e})")
        assert e > CEILING, what


@pytest.mark.parametrize("name", list(P.CASES))
def test_the_documented_arithmetic_meets_the_gate(name):
    case, ref, m, f32 = _host(name)
    ef = P.scaled_error(f32, ref, m)[0]
    assert torch.isfinite(m).all() and torch.isfinite(f32).all() and ef < 1e-5
    if case["kind"] == "reduce" and case["extra"] is None and max(len(s) for s in case["seg_slots"]) == 1:
        assert ef == 0                       # one partial row per segment and nothing added: exact
    else:
        assert ef > 0
    if case["kind"] == "reduce":
        second = P.evaluate(case, torch.float32, seg_slots=[s[::-1] for s in case["seg_slots"]])      # last tile first
    else:
        second = P.evaluate(case, torch.float32, order="blocks_reversed")
    emu = P.emulate(case)
    for what, got in (("emulation", emu), ("second fp32 order", second)):
        e = P.scaled_error(got, ref, m)[0]
        print(f"[parity] pool reference {name}, {what}: E {e:.2e}, E_f32 {ef:.2e}, ratio {e / ef if ef else 0:.2f} (gate 4)")
        assert e <= 4 * ef and e <= CEILING, what
    dead = m == 0
    assert not ref[dead].any() and not emu[dead].any() and not f32[dead].any()
    if case["kind"] == "reduce":
        again = P.evaluate(case, torch.float32)
        assert torch.equal(f32.view(torch.int32), again.view(torch.int32))


@pytest.mark.parametrize("name", ["sweep33", "ones", "ragged"])
def test_the_fp32_tile_sums_in_row_order(name):
    """``tile_partials`` in float32 (the running sum the producers document) against float64 and against a plain loop
    over the rows that starts a new sum behind every segment end and every tile end"""
    sp = P.seg_ptr_of(P.layout(name))
    n = int(sp[-1])
    rows = torch.relu(torch.randn(n, 8, generator=torch.Generator().manual_seed(n)))
    p32, p64, m = (P.tile_partials(rows, sp, torch.float32), P.tile_partials(rows, sp),
                   P.tile_partials(rows, sp, absolute=True))
    e = P.scaled_error(p32, p64, m)[0]
    assert p32.dtype == torch.float32 and e < 1e-5 and (e > 0 or name == "ones")
    ends, loop, run = set((sp[1:] - 1).tolist()), [], np.zeros(8, np.float32)
    for r in range(n):
        run = run + rows[r].numpy()
        if r in ends or r % P.TILE == P.TILE - 1 or r == n - 1:
            loop.append(run)
            run = np.zeros(8, np.float32)
    assert np.array_equal(np.stack(loop), p32.numpy())
