"""The kernels of the neighborhood models of other widths than 64 (csrc/shmp_wide.hip) -- the fused layer through
ops.shmp_layer_wide, the gather through ops.csr_gather_sum_wide, the un-fused pair csr_gather_sum_wide + gemm_f16x3, and
the autograd nodes GatherSumWide / SegmentSumWide -- per element against the fp64 host reference tests/wide_reference.py.

Gate (that of tests/test_shmp_trunk_kernels_gpu.py; no number of its own): per tensor E_kernel = max |got - ref| / mag
over ALL elements a launch computes, mag = the reference evaluated on absolute values (the sum of |terms| of the element).
E_kernel <= 4 E_f32, where E_f32 is the same figure of the reference evaluated in float32 on the host on the same case,
and E_kernel <= 1e-4 (the ceiling of tests/test_train_kernels_gpu.py).  An element with mag == 0 must be exactly 0.
tests/test_wide_reference_host.py proves the gate reachable on every case below: the kernel's arithmetic restated on the
host and a second fp32 summation order both stay within it.  Every test prints E_kernel, E_f32 and their ratio as
``[parity]`` lines; the worst ratio per family is printed once more when the module ends.

Every layer case runs the fused kernel twice (bit-identical), checks that nothing outside the rows and columns it owns
was written (NaN-filled parents of out, out2 and x), and runs the un-fused pair on the same inputs against the same
reference.  The gather must moreover reproduce the float32 sum in CSR order bit for bit, which is what it documents."""
import collections
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import shmp_reference as R  # noqa: E402
import wide_reference as W  # noqa: E402
from desco_amd import autograd as AG  # noqa: E402
from desco_amd import ops  # noqa: E402

DEV = "cuda"
CEILING = 1e-4
NAN = float("nan")
WORST = collections.defaultdict(float)          # family -> worst E_kernel / E_f32 seen


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    for k in sorted(WORST):
        print(f"[parity] wide worst E_kernel / E_f32 over the module, {k}: {WORST[k]:.2f} (gate 4)")


def _gate(name, family, got, ref, mag, f32):
    """E_kernel <= 4 E_f32 and <= CEILING; zero where mag is zero"""
    g = got.detach().cpu().double().reshape(ref.shape)
    ek, i = W.scaled_error(g, ref, mag)
    ef, _ = W.scaled_error(f32, ref, mag)
    ratio = ek / ef if ef > 0 else (0.0 if ek == 0 else float("inf"))
    WORST[family] = max(WORST[family], ratio)
    print(f"[parity] {family}, {name}: E_kernel {ek:.3e}, E_f32 {ef:.3e}, ratio {ratio:.2f} (gate 4, ceiling {CEILING:.0e})")
    exact = bool((g[mag == 0] == 0).all())
    assert ek <= 4 * ef and ek <= CEILING and exact, (
        f"{family}, {name}: E_kernel {ek:.3e} E_f32 {ef:.3e} ratio {ratio:.2f}; element {i} (row {i // max(ref.shape[-1], 1)}, "
        f"column {i % max(ref.shape[-1], 1)}): got {float(g.flatten()[i])!r}, ref {float(ref.flatten()[i])!r}, "
        f"mag {float(mag.flatten()[i])!r}{'' if exact else '; nonzero where mag == 0'}")


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _all_nan(t):
    return bool(torch.isnan(t).all())


def _i32(t):
    return t.to(torch.int32).to(DEV)


@functools.lru_cache(maxsize=None)
def _host(name):
    """(case, fp64 reference, mag, fp32 evaluation) of a named case, computed once for the module"""
    case = W.make(name)
    return case, W.evaluate(case), W.mag(case), W.evaluate(case, torch.float32)


@functools.lru_cache(maxsize=None)
def _device(name):
    """the case's operands on the device: x (a 16-byte-aligned column view of a NaN-filled parent with ldx = Wp + 12, or
    contiguous), its parent, the index, the weight planes of Wt.T, the bias"""
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
    w = ops.split_f16_planes(case["Wt"].t().contiguous().to(DEV))
    return xd, parent, _i32(case["vrowptr"]), _i32(case["vcol"]), w, case["bias"].to(DEV)


def _fused(name, row0, num_rows, mode, out=None):
    """one launch of the layer kernel on rows [row0, row0 + num_rows) -> the rows it produced [num_rows, Wp]; everything
    else of the NaN-filled out [N, Wp] and of out2's NaN-filled parent [num_rows, 3 Wp + 7] must still be NaN"""
    case = _host(name)[0]
    xd, parent, vrowptr, vcol, w, bias = _device(name)
    N, wp = xd.shape
    fresh = out is None
    if fresh:
        out = torch.full((N, wp), NAN, device=DEV)
    buf2 = torch.full((num_rows, 3 * wp + 7), NAN, device=DEV)
    out2 = buf2[:, wp + 5:2 * wp + 5]                            # a column block that starts at no multiple of 4
    ops.shmp_layer_wide(xd, vrowptr, vcol, case["vslots"], row0, num_rows, case["slots"], w, bias,
                        out=out if mode in ("out", "both") else None, out2=out2 if mode in ("out2", "both") else None)
    rows = out[row0:row0 + num_rows]
    if mode == "out2":
        assert _all_nan(out), f"{name}: out was not given and was written"
    elif fresh:
        assert _all_nan(out[:row0]) and _all_nan(out[row0 + num_rows:]), f"{name}: rows outside the range were written"
    if mode == "out":
        assert _all_nan(buf2), f"{name}: out2 was not given and was written"
    else:
        assert _all_nan(buf2[:, :wp + 5]) and _all_nan(buf2[:, 2 * wp + 5:]), f"{name}: out2 written outside its block"
        if mode == "both":
            assert _same_bits(rows, out2), f"{name}: out and out2 differ"
        rows = out2
    assert not torch.isnan(rows).any(), f"{name}: an element of the range was not written (or is NaN)"
    if case["x_strided"]:
        assert _all_nan(parent[:, :8]) and _all_nan(parent[:, 8 + wp:]) and _same_bits(xd, case["x"].to(DEV))
    return rows.clone()


def _unfused(name, row0, num_rows):
    """the SHMP_WIDE_FUSED = False form of the same launch: csr_gather_sum_wide over all rows, gemm_f16x3 on the range"""
    case = _host(name)[0]
    xd, _, vrowptr, vcol, w, bias = _device(name)
    N, wp = xd.shape
    agg = ops.csr_gather_sum_wide(xd, vrowptr, vcol, N, case["vslots"])
    return ops.gemm_f16x3(agg[row0:row0 + num_rows, :case["slots"] * wp], w, bias, a2=xd[row0:row0 + num_rows],
                          act=ops.ACT_RELU)


def _run_layer(name):
    case, ref, m, f32 = _host(name)
    r0, n = case["row0"], case["num_rows"]
    r = slice(r0, r0 + n)
    got = _fused(name, r0, n, case["out_mode"])
    assert _same_bits(got, _fused(name, r0, n, case["out_mode"])), f"{name}: two launches on the same inputs differ"
    _gate(name, "layer fused", got, ref[r], m[r], f32[r])
    un = _unfused(name, r0, n)
    _gate(name, "layer un-fused", un, ref[r], m[r], f32[r])
    relu_bias = torch.relu(case["bias"]).to(DEV)
    for i in case["bare"]:                                       # x == 0, no source: the scale of every block must be 1
        assert _same_bits(got[i - r0], relu_bias) and _same_bits(un[i - r0], relu_bias), f"{name}: bare row {i}"
    if case["H"] is not None:                                    # the padded channels stay exactly 0
        assert not got[:, case["H"]:].any() and not un[:, case["H"]:].any() and got[:, :case["H"]].any()
    return got


def _family(word):
    return [n for n in W.CASES if n.split()[0] == word]


@pytest.mark.parametrize("name", _family("instantiation"))
def test_every_instantiation_matches_the_reference(name):
    """Wp in {64, 128, 192, 256} x S in {2, 4} (256: the LDS image beyond 64 KiB; 192: three column tiles per wave) on
    O(1) inputs of both signs, launched as the canonical rows are (slots <= vslots = 4, row0 = 37), 203 rows: every degree
    0..9, a third of the virtual rows empty, hubs of 301, 203 and 77 sources."""
    assert {(W.CASES[n]["wp"], W.CASES[n]["S"]) for n in _family("instantiation")} == {(w, s) for w in W.WIDTHS
                                                                                        for s in W.SLOTS}
    _run_layer(name)


@pytest.mark.parametrize("name", _family("range"))
def test_row_ranges_match_the_reference(name):
    """(row0, num_rows) in {(0, 1), (0, 63), (0, 64), (5, 65), (37, 203)}: one row, a tile short of one row, one full
    tile, a second tile of one row, four tiles with a clamped last one; sources on both sides of the range; the rows of
    the NaN-filled ``out`` outside the range stay NaN."""
    _run_layer(name)


@pytest.mark.parametrize("name", _family("arguments") + _family("outputs") + _family("degrees"))
def test_argument_shapes_outputs_and_strides_match_the_reference(name):
    """vslots 4 / slots 2 / row0 > 0 (virtual rows 2 and 3 hold edges that must not be read), vslots 2 / slots 2, vslots 4
    / slots 4; ``out`` only, ``out2`` only (a column block of a [num_rows, 3 Wp + 7] buffer starting at column Wp + 5) and
    both; x a column view with ldx = Wp + 12 and contiguous; an empty ``vcol``."""
    _run_layer(name)


@pytest.mark.parametrize("name", _family("regime") + _family("padding"))
def test_value_ranges_and_padding_match_the_reference(name):
    """Rows at 2^-16 .. 2^16 mixed inside the 64-row tiles, everything x 1e5 and x 1e-4, 30 % all-zero rows (a zero row
    without sources gives relu(bias) bit for bit; an all-zero block next to live ones), one block of a row at 2^-20 of
    the others; H = 100 in Wp = 128 and H = 32 in Wp = 64 with zero padding: the columns >= H are exactly 0."""
    _run_layer(name)


@pytest.mark.parametrize("name", _family("instantiation"))
def test_a_result_does_not_depend_on_the_tiling(name):
    """rows (37, 203) launched once, and as (37, 50) + (87, 153) -- other rows share a 64-row tile, the scales of a row
    are its own -- give the same bits"""
    case = _host(name)[0]
    assert (case["row0"], case["num_rows"]) == (37, 203)
    once = _fused(name, 37, 203, "out")
    out = torch.full(tuple(case["x"].shape), NAN, device=DEV)
    _fused(name, 37, 50, "out", out=out)
    assert _all_nan(out[:37]) and _all_nan(out[87:])
    _fused(name, 87, 153, "out", out=out)
    assert _all_nan(out[:37]) and _all_nan(out[240:])
    assert _same_bits(once, out[37:240]), f"{name}: the rows depend on the launch's tiling"


# ---- csr_gather_sum_wide ----------------------------------------------------------------------------------------------
def _gather_dev(x, vrowptr, vcol, num_rows, slots, strided=True):
    """the kernel on a column view of x (ldx = width + 8, 16 bytes in) into rows 1 .. num_rows of a NaN-filled buffer"""
    n_src, width = x.shape
    if strided:
        parent = torch.full((n_src, width + 8), NAN)
        parent[:, 4:4 + width] = x
        xd = parent.to(DEV)[:, 4:4 + width]
        assert xd.stride(0) > width and xd.data_ptr() % 16 == 0
    else:
        xd = x.to(DEV)
    buf = torch.full((num_rows + 2, slots * width), NAN, device=DEV)
    out = ops.csr_gather_sum_wide(xd, _i32(vrowptr), _i32(vcol), num_rows, slots, out=buf[1:num_rows + 1])
    assert _all_nan(buf[0]) and _all_nan(buf[-1]), "rows outside out were written"
    assert out.data_ptr() == buf[1:].data_ptr()
    return out.clone()


@pytest.mark.parametrize("width", W.GATHER_WIDTHS)
def test_gather_is_the_fp32_sum_in_csr_order(width):
    """widths {4, 32, 100, 128, 252, 256} (100 and 252: lanes beyond the width leave early) x slots {1, 2, 4} x num_rows
    {1, 3, 4, 5, 203} (four virtual rows per workgroup and its tail): bit-identical to the float32 sum in CSR order, and
    within the gate of the fp64 sum; ldx > width; every degree 0..9 and hubs at 203 rows; an empty vcol.  (``out`` must
    be contiguous, so there are no columns beyond the width to guard: the rows around it are.)"""
    for slots in W.GATHER_SLOTS:
        for n in W.GATHER_ROWS:
            args = W.gather_case(width, slots, n, seed=width + 7 * slots + n)
            got = _gather_dev(*args, n, slots).view(n * slots, width)
            f32 = W.gather(args, torch.float32)
            _gate(f"width {width}, slots {slots}, {n} rows", "gather", got, W.gather(args), W.gather(args, absolute=True), f32)
            assert _same_bits(got.cpu(), f32), f"width {width}, slots {slots}, {n} rows: not the fp32 sum in CSR order"
    args = W.gather_case(width, 2, 203, seed=width)
    deg = (args[1][1:] - args[1][:-1]).tolist()
    assert set(range(10)) <= set(deg) and set(W.HUBS) <= set(deg)
    assert _same_bits(_gather_dev(*args, 203, 2, strided=False).view(406, width).cpu(), W.gather(args, torch.float32))
    args = W.gather_case(width, 4, 5, edges=False)
    assert not args[2].numel() and not _gather_dev(*args, 5, 4).any()


# ---- the autograd nodes -------------------------------------------------------------------------------------------------
def _query_batch():
    from desco_amd.batch import QueryBatch
    graphs = list(R.SHAPES) + [R.wheel(20), R.star(9), R.random_graph(30, 1)]
    return "query batch", QueryBatch(graphs, DEV)


def _neighborhood_batch():
    from helpers import golden_graphs
    from desco_amd.batch import NeighborhoodBatch
    from desco_amd.graphs import GraphSet
    from desco_amd.partition import build_partition
    return "neighborhood batch", NeighborhoodBatch(build_partition(GraphSet.from_edge_lists(golden_graphs(max_n=41)[:10]), 4), DEV)


@pytest.mark.parametrize("width", [4, 100, 256])
@pytest.mark.parametrize("make", [_query_batch, _neighborhood_batch])
def test_gather_node_matches_torch_autograd_in_fp64(make, width):
    """autograd.GatherSumWide, forward and backward, against torch autograd in float64 over the explicit index lists
    (``index_add`` of x[vcol] at the edges' virtual rows), with the transposed index of the product's own train_index()
    (ops.vcsr_transpose_sym), as shmp_forward_train_wide runs it -- after that index has been shown to be the transpose
    of the forward one.  Two slots (query graphs) and four (count and canonical rows)."""
    tag, batch = make()
    N, S = batch.num_rows, batch.slots
    vrowptr, vcol = batch.vrowptr.cpu().long(), batch.vcol.cpu().long()
    assert vrowptr.numel() == N * S + 1
    deg = vrowptr[1:] - vrowptr[:-1]
    vrow = torch.repeat_interleave(torch.arange(N * S), deg)
    assert int(deg.min()) == 0 and int(deg.max()) >= 8
    ti = batch.train_index()
    order = torch.from_numpy(np.argsort(vcol.numpy(), kind="stable"))          # edges by source, then by virtual row
    t_rowptr = torch.cat([torch.zeros(1, dtype=torch.long), torch.bincount(vcol, minlength=N).cumsum(0)])
    assert torch.equal(ti["t_rowptr"].cpu().long(), t_rowptr), f"{tag}: t_rowptr is not the transpose's"
    assert torch.equal(ti["t_col"].cpu().long(), vrow[order]), f"{tag}: t_col is not the transpose's"
    g = torch.Generator().manual_seed(width + S)
    x, dagg = torch.randn(N, width, generator=g), torch.randn(N, S * width, generator=g)
    xd = x.to(DEV).requires_grad_()
    agg = AG.GatherSumWide.apply(xd, batch.vrowptr, batch.vcol, ti["t_rowptr"], ti["t_col"], N, S)
    (agg * dagg.to(DEV)).sum().backward()
    xr = x.double().requires_grad_()
    ref = torch.zeros(N * S, width, dtype=torch.float64).index_add(0, vrow, xr[vcol]).view(N, S * width)
    (ref * dagg.double()).sum().backward()
    fwd = (x, vrowptr, vcol)
    shape = (N, S * width)
    _gate(f"{tag}, width {width}, forward", "GatherSumWide", agg, ref.detach(), W.gather(fwd, absolute=True).view(shape),
          W.gather(fwd, torch.float32).view(shape))
    bwd = (dagg.view(N * S, width), t_rowptr, vrow[order])
    _gate(f"{tag}, width {width}, backward", "GatherSumWide", xd.grad, xr.grad, W.gather(bwd, absolute=True),
          W.gather(bwd, torch.float32))


@pytest.mark.parametrize("width", [4, 100, 256])
@pytest.mark.parametrize("extra", [False, True])
def test_segment_sum_node_matches_torch_autograd_in_fp64(extra, width):
    """autograd.SegmentSumWide with and without ``extra``, forward and backward (a broadcast by csr_gather_sum_wide over
    the segment ids: exact), 60 segments of 0, 1 and up to 70 rows, against torch autograd in float64"""
    sizes = [0, 1, 5, 0, 0, 1, 70, 3, 64, 0] + np.random.default_rng(5).integers(0, 40, 50).tolist()
    seg_ptr = torch.tensor([0] + list(np.cumsum(sizes)), dtype=torch.int64)
    n, B = int(seg_ptr[-1]), len(sizes)
    seg = torch.repeat_interleave(torch.arange(B), seg_ptr[1:] - seg_ptr[:-1])
    seg_ptr_d = _i32(seg_ptr)
    seg_id = ops.segment_ids(seg_ptr_d, n)
    assert torch.equal(seg_id.cpu().long(), seg)
    ident_ptr = torch.arange(n + 1, device=DEV, dtype=torch.int32)
    g = torch.Generator().manual_seed(width + extra)
    x, ex, dout = torch.randn(n, width, generator=g), torch.randn(B, width, generator=g), torch.randn(B, width, generator=g)
    xd = x.to(DEV).requires_grad_()
    exd = ex.to(DEV).requires_grad_() if extra else None
    out = AG.SegmentSumWide.apply(xd, seg_ptr_d, seg_id, ident_ptr, exd)
    (out * dout.to(DEV)).sum().backward()

    def host(dtype, absolute=False):
        conv = (lambda t: t.to(dtype).abs()) if absolute else (lambda t: t.to(dtype))    # noqa: E731
        xr, er = conv(x).requires_grad_(), conv(ex).requires_grad_()
        o = torch.zeros(B, width, dtype=dtype).index_add(0, seg, xr)
        if extra:
            o = o + er
        (o * conv(dout)).sum().backward()
        return o.detach(), xr.grad, er.grad
    ref, m, f32 = host(torch.float64), host(torch.float64, True), host(torch.float32)
    tag = f"width {width}, extra {extra}"
    _gate(f"{tag}, forward", "SegmentSumWide", out, ref[0], m[0], f32[0])
    _gate(f"{tag}, dx", "SegmentSumWide", xd.grad, ref[1], m[1], f32[1])
    assert _same_bits(xd.grad.cpu(), dout[seg]), f"{tag}: dx is not the broadcast of dout"
    if extra:
        assert _same_bits(exd.grad.cpu(), dout), f"{tag}: dextra is not dout"
        assert not out.detach()[0].cpu().sub(ex[0]).any(), f"{tag}: an empty segment is not its extra row"
    else:
        assert not out.detach()[0].any() and not out.detach()[3].any(), f"{tag}: an empty segment is not zero"
