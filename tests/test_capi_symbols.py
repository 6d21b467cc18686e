"""The C-ABI library loads on a CPU-only host and exports every symbol include/desco_hip.h declares.
No compute entry point is called (there is no GPU here)."""
import ctypes
import os
import re

import numpy as np
import pytest

from desco_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "desco_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(desco_[a-z0-9_]+)\s*\(", src)))


def test_library_loads_and_exports_header_symbols():
    L = _lib.lib()
    names = declared_symbols()
    assert len(names) >= 15
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/desco_hip.h but not exported"
    assert set(names) == set(_lib.SIGNATURES), "ctypes SIGNATURES out of sync with the header"
    assert L.desco_abi_version() == _lib.ABI_VERSION == 6
    assert L.desco_count_head_bwd_workspace(512, 29, 256) == 32 * 30 * 256 * 4
    assert L.desco_count_head_bwd_workspace(10 ** 6, 29, 256) == 1024 * 30 * 256 * 4


def test_argument_errors_are_reported_not_crashed():
    L = _lib.lib()
    rc = L.desco_gemm_f32(None, 0, 48, None, 0, 0, None, 64, None, 1, None, 0, None, 0, 0.0, None,
                          64, 5, None)
    assert rc == -1
    assert b"desco_gemm_f32" in L.desco_last_error()
    with pytest.raises(RuntimeError):
        _lib.check(rc, "gemm")


def test_new_entry_points_validate_their_arguments():
    """Round-3 entry points: bad arguments come back as DESCO_EINVAL with a message (no launch, no crash)."""
    L = _lib.lib()
    cp = np.zeros(1, np.int32)
    vr = np.zeros(1, np.int32)
    assert L.desco_partition_degree_sort(None, 0, vr.ctypes.data, None, None, None, vr.ctypes.data, None, None, 0) == -1
    assert b"desco_partition_degree_sort" in L.desco_last_error()
    assert L.desco_partition_degree_sort(cp.ctypes.data, -1, vr.ctypes.data, None, None, cp.ctypes.data,
                                         vr.ctypes.data, None, None, 0) == -1
    # an empty block is fine (no rows, no edges)
    out = np.zeros(1, np.int32)
    assert L.desco_partition_degree_sort(cp.ctypes.data, 0, vr.ctypes.data, None, None, cp.ctypes.data,
                                         out.ctypes.data, None, None, 1) == 0 and out[0] == 0
    assert L.desco_gossip_tile_order(None, 5, None, None) == -1
    assert b"desco_gossip_tile_order" in L.desco_last_error()
    assert L.desco_gossip_tile_order(None, 0, None, None) == 0          # nothing to do
    assert L.desco_gossip_fused_f32(*([None] * 3), 7, 29, *([None] * 16), 0.0, None, None, None) == -1
    assert b"desco_gossip_fused_f32" in L.desco_last_error()


def test_round4_entry_points_validate_their_arguments():
    """Round-4 entry points: bad arguments come back as DESCO_EINVAL with a message naming the entry point."""
    L = _lib.lib()
    one = np.zeros(4, np.float32)
    assert L.desco_adam_step_f32(1, None, None, None, None, None, None, None, None, 0.9, 0.999, 1e-8, 0.0, None) == -1
    assert b"desco_adam_step_f32" in L.desco_last_error()
    assert L.desco_adam_step_f32(0, None, None, None, None, None, None, None, None, 0.9, 0.999, 1e-8, 0.0, None) == 0
    assert L.desco_gemm_f32_multi(5, None, None) == -1 and b"desco_gemm_f32_multi" in L.desco_last_error()
    assert L.desco_gemm_f32_multi(0, None, None) == 0
    d = (_lib.GemmDesc * 1)()
    d[0].m, d[0].k1, d[0].n = 8, 48, 64                    # k % 32 != 0, null operands
    assert L.desco_gemm_f32_multi(1, d, None) == -1
    assert L.desco_linear_bwd_w_multi_f32(17, None, None, None) == -1
    assert b"desco_linear_bwd_w_multi_f32" in L.desco_last_error()
    b = (_lib.BwdWDesc * 2)()
    b[0].m, b[0].k1, b[0].n = 1000, 64, 64
    b[1].m, b[1].k1, b[1].k2, b[1].n = 10, 128, 64, 64
    assert L.desco_linear_bwd_w_multi_workspace(2, b) == (L.desco_linear_bwd_w_workspace(1000, 64, 64) +
                                                          L.desco_linear_bwd_w_workspace(10, 192, 64))
    assert L.desco_rowdot_bwd_f32(None, 256, 256, None, None, 4, None, 256, None, None, None) == -1
    assert b"desco_rowdot_bwd_f32" in L.desco_last_error()
    assert L.desco_linear_smallk_bwd_f32(None, 1, 1, None, 64, 4, None, None, None) == -1
    assert b"desco_linear_smallk_bwd_f32" in L.desco_last_error()
    assert L.desco_shmp_trunk_small_max_rows() == 144
    assert L.desco_shmp_trunk_small_fwd_f32(None, None, None, 200, 8, None, None, None, 29, None, None, 576, None) == -1
    assert b"desco_shmp_trunk_small_fwd_f32" in L.desco_last_error()
    assert L.desco_shmp_trunk_small_bwd_f32(*([None] * 7), 10, 8, None, None, 576, None, None, None, None) == -1
    assert L.desco_gossip_fused_f16x3_f32(*([None] * 3), 7, 29, *([None] * 14), 0.0, None, None, None, None) == -1
    assert b"desco_gossip_fused_f16x3_f32" in L.desco_last_error()
    assert L.desco_gemm_f16x3_f32 is not None and L.desco_row_absmax_f32 is not None


def test_gossip_scalars_refuses_query_counts_outside_1_to_64():
    """desco_gossip_scalars_f32 maps one lane to one query: num_q = 0 and 65 are refused on the host, before any launch,
    with every pointer valid and aligned (so that the query count is the only thing wrong), naming the entry point."""
    L = _lib.lib()
    buf = np.zeros(64, np.float32)
    idx = np.zeros(4, np.int32)
    aligned = buf.ctypes.data + (-buf.ctypes.data % 16)          # scal4 has to be 16-byte aligned
    for num_q in (0, 65, -1):
        L.desco_gemm_f32_multi(5, None, None)                   # (another entry point's message in between)
        assert L.desco_gossip_scalars_f32(buf.ctypes.data, num_q, idx.ctypes.data, idx.ctypes.data, 1, num_q,
                                          buf.ctypes.data, buf.ctypes.data, aligned, None) == -1
        assert b"desco_gossip_scalars_f32" in L.desco_last_error()


def test_ops_refuse_cpu_tensors():
    import torch
    from desco_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.csr_gather_sum(torch.zeros(4, 64), torch.zeros(5, dtype=torch.int32),
                           torch.zeros(0, dtype=torch.int32), 1, 4)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.DescoLibraryError, match="no CPU or PyTorch fallback"):
        _lib.lib()


def test_adam_refuses_cpu_parameters():
    from desco_amd.optim import Adam
    import torch
    p = torch.zeros(4, requires_grad=True)
    p.grad = torch.ones(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Adam([p]).step()


def test_shipped_isa_passes_the_operand_selection_rule():
    """tools/check_isa.py on the library these tests load: no packed fp32 instruction takes its low lane from the high
    dword of src1/src2 (wrong values in lanes 48-63 beside MFMAs on MI355X, profiles/r5_a_gossip_f16_hazard.md).  The
    Makefile runs the same check at link time; this covers a library that was built some other way."""
    import subprocess
    import sys
    from desco_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tool = os.path.join(root, "tools", "check_isa.py")
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("llvm-objdump not installed")
    r = subprocess.run([sys.executable, tool, _lib.LIB_PATH], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "packed-fp32 instructions scanned, 0 with OP_SEL" in r.stdout
    # and the checker itself catches the form
    import tempfile
    with tempfile.NamedTemporaryFile("w", suffix=".s", delete=False) as f:
        f.write("k:\n\tv_pk_mul_f32 v[2:3], v[4:5], v[6:7] op_sel:[0,1]\n\tv_pk_fma_f32 v[2:3], v[4:5], v[6:7], v[8:9] op_sel_hi:[1,0,1]\n"
                "\tv_pk_fma_f32 v[2:3], v[4:5], v[6:7], v[8:9] op_sel:[1,0,0]\n\tv_pk_add_f32 v[2:3], v[4:5], v[6:7] op_sel:[0,0,1]\n")
        name = f.name
    r = subprocess.run([sys.executable, tool, name], capture_output=True, text=True)
    os.unlink(name)
    assert r.returncode == 1 and "4 packed-fp32 instructions scanned, 2 with OP_SEL" in r.stdout, r.stdout


def test_round6_entry_points_validate_their_arguments():
    """Dropout entry points: bad arguments come back as DESCO_EINVAL with a message (no launch, no crash)."""
    L = _lib.lib()
    assert L.desco_rng_next(None, None, None) == -1 and b"desco_rng_next" in L.desco_last_error()
    d = _lib.Dropout()
    one = np.zeros(4, np.float32)
    assert L.desco_dropout_mask_f32(ctypes.byref(d), 4, 1, one.ctypes.data, 1, None) == -1      # no key
    assert b"dropout" in L.desco_last_error()
    assert L.desco_dropout_mask_f32(ctypes.byref(d), 0, 64, None, 64, None) == 0                # nothing to do
    key = np.zeros(2, np.uint64)
    d.key, d.site = key.ctypes.data, 256
    assert L.desco_dropout_mask_f32(ctypes.byref(d), 4, 1, one.ctypes.data, 1, None) == -1      # site out of range
    assert b"site" in L.desco_last_error()
    assert L.desco_affine_rows_dropout_f32(None, one.ctypes.data, 1, one.ctypes.data, 1, 0, 0.0, None,
                                           one.ctypes.data, 1, None) == -1
    assert b"desco_affine_rows_dropout_f32" in L.desco_last_error()
    assert L.desco_act_grad_dropout_f32(None, None, 1, 0.0, ctypes.byref(d), None, 4, 64, None) == -1
    assert b"desco_act_grad_dropout_f32" in L.desco_last_error()
    g = (_lib.GemmDesc * 1)()
    assert ctypes.sizeof(_lib.GemmDesc) % 8 == 0 and _lib.GemmDesc.drop.offset % 8 == 0


def test_training_entry_points_validate_their_arguments():
    """Training-step entry points: each limit below comes back as DESCO_EINVAL naming the entry point, before any HIP call.
    Every other argument is valid, so the one limit named is what each call trips on."""
    L = _lib.lib()
    buf = np.zeros(64 * 1024, np.float32)
    p = buf.ctypes.data
    assert p % 16 == 0

    def rejects(name, rc):
        assert rc == -1, name
        assert name.encode() in L.desco_last_error(), (name, L.desco_last_error())
        assert L.desco_rng_next(None, None, None) == -1          # (resets the message for the next case)

    rejects("desco_affine_rows_bwd_f32", L.desco_affine_rows_bwd_f32(p, 3, p, 29, 29 * 5 + 1, p, p, None))  # rows % qv
    rejects("desco_affine_rows_bwd_f32", L.desco_affine_rows_bwd_f32(p, 9, p, 29, 29 * 5, p, p, None))      # ks = 9
    rejects("desco_count_head_wide_f32", L.desco_count_head_wide_f32(p, 96, p, 96, 96, p, 0.0, None, 0.01, 0, p, 4, 10, 4,
                                                                     None))                              # hid = 96
    rejects("desco_count_head_wide_f32", L.desco_count_head_wide_f32(p, 64, p, 64, 64, p, 0.0, None, 0.01, 0, p, 33, 10, 33,
                                                                     None))                              # num_q = 33
    rejects("desco_loss_f32", L.desco_loss_f32(p, p, 0, 0, p, p, p, None))                                # count 0
    rejects("desco_loss_f32", L.desco_loss_f32(p, p, 0, 1, p, p, p, None))
    table = np.zeros(64, np.int64)
    rejects("desco_fold_shmp_fwd_f32", L.desco_fold_shmp_fwd_f32(table.ctypes.data, 1, 5, 1, p, p, None))  # slots = 5
    prm, out = _lib.GossipFoldParams(), _lib.GossipFoldOut()
    for n, _ in _lib.GossipFoldParams._fields_:
        if n == "num_q":
            continue
        v = getattr(prm, n)
        if isinstance(v, ctypes.Array):
            for i in range(len(v)):
                v[i] = p
        else:
            setattr(prm, n, p)
    for n, _ in _lib.GossipFoldOut._fields_:
        setattr(out, n, p)
    prm.num_q = 65
    rejects("desco_gossip_fold_fwd_f32", L.desco_gossip_fold_fwd_f32(ctypes.byref(prm), ctypes.byref(out), None))


def test_per_graph_trunk_entry_points_validate_their_arguments():
    """desco_shmp_trunk_graphs_fwd_f32 / _bwd_f32: each call below is wrong in ONE way (every other argument valid and
    16-byte aligned) and comes back as DESCO_EINVAL naming the entry point, before any HIP call."""
    L = _lib.lib()
    buf = np.zeros(64 * 1024, np.float32)
    idx = np.zeros(64, np.int32)
    p, q = buf.ctypes.data, idx.ctypes.data
    assert p % 16 == 0
    key = np.zeros(2, np.uint64)
    layers, ldp = 3, 64 * 4

    def drop(site, k=key.ctypes.data):
        d = _lib.Dropout()
        d.key, d.site, d.threshold, d.scale = k, site, 1 << 30, 4.0 / 3.0
        return ctypes.byref(d)

    def rejects(name, rc):
        assert rc == -1, name
        assert name.encode() in L.desco_last_error(), (name, L.desco_last_error())
        assert L.desco_rng_next(None, None, None) == -1          # (resets the message for the next case)

    def fwd(x0=p, rows=8, nl=layers, wt=p, bias=p, d=None, xall=p, pooled=p, ld=ldp):
        return L.desco_shmp_trunk_graphs_fwd_f32(x0, q, q, rows, nl, wt, bias, q, 2, d, xall, pooled, ld, None)

    def bwd(x0=p, xall=p, nl=layers, wt=p, dp=p, ld=ldp, dwt=p, ws=p):
        return L.desco_shmp_trunk_graphs_bwd_f32(x0, xall, q, q, q, q, q, 2, 8, nl, wt, dp, ld, 1.0, dwt, p, p, ws, None)

    name = "desco_shmp_trunk_graphs_fwd_f32"
    rejects(name, fwd(x0=None))                                  # a null pointer
    rejects(name, fwd(pooled=None))
    rejects(name, fwd(ld=ldp - 4))                               # ldp < 64 (L + 1)
    rejects(name, fwd(ld=ldp + 2))                               # ldp % 4
    rejects(name, fwd(xall=p + 4))                               # a misaligned pointer
    rejects(name, fwd(nl=0))
    rejects(name, fwd(d=drop(256 - 2 * layers)))                 # site + 2 L >= 256
    rejects(name, fwd(d=drop(5, None)))                          # a descriptor without a key
    assert fwd(rows=0) == 0                                      # nothing to do
    name = "desco_shmp_trunk_graphs_bwd_f32"
    rejects(name, bwd(x0=None))
    rejects(name, bwd(ws=None))
    rejects(name, bwd(ld=ldp - 4))
    rejects(name, bwd(ld=ldp + 2))
    rejects(name, bwd(dp=p + 4))
    rejects(name, bwd(nl=0))
    assert L.desco_shmp_trunk_graphs_max_rows() == 8


def test_entry_points_refuse_misaligned_pointers():
    """A float4-accessed operand that is 4 bytes off a 16-byte boundary comes back as DESCO_EINVAL naming the entry point,
    before any HIP call.  Every other argument of each call is valid (fake aligned host pointers, never dereferenced),
    so the misaligned pointer is what the call trips on."""
    L = _lib.lib()
    buf = np.zeros(64 * 1024, np.float32)
    idx = np.zeros(64, np.int32)
    p, q = buf.ctypes.data, idx.ctypes.data
    assert p % 16 == 0
    o, t, w = p + 65536, p + 131072, p + 196608            # distinct aligned operands: out, table / second input, weights

    def rejects(name, rc):
        assert rc == -1, name
        assert name.encode() in L.desco_last_error(), (name, L.desco_last_error())
        assert L.desco_rng_next(None, None, None) == -1          # (resets the message for the next case)

    def layer_f32(x=p, ytab=t, out=o):
        return L.desco_shmp_layer_f32(x, 64, q, q, 0, 8, 4, 2, 2, w, w, ytab, 128, 0, out, 64, None, 0, None)

    def layer_f16(x=p, ytab=t, out=o, planes=w):
        return L.desco_shmp_layer_f16x3_f32(x, 64, q, q, 0, 8, 4, 2, 2, planes, w, w, ytab, 128, 0, out, 64, None, 0,
                                            None, None, 0, None)

    def linear64(x=p, planes=w, out=o):
        return L.desco_linear64_bf16x6_f32(x, 64, planes, 1, w, 0, 0.0, out, 64, 8, None)

    def gemm_x6(a1=p, planes=w):
        return L.desco_gemm_bf16x6_f32(a1, 64, 64, None, 0, 0, planes, 64, None, 1, None, 0, None, 0, 0.0, o, 64, 8, None)

    def gemm_f16(a1=p, planes=w):
        return L.desco_gemm_f16x3_f32(a1, 64, 64, None, 0, 0, planes, t, 64, None, 1, None, 0, None, 0, 0.0, o, 64, 8, t,
                                      None)

    def gemm_tn(a=p, b=t):
        return L.desco_gemm_tn_f32(a, 64, b, 64, 8, 64, 64, o, 64, 0, w, None)

    def gossip_layer(h=p, acc=t, out=o):
        return L.desco_gossip_layer_f16x3_f32(h, q, q, 8, 2, w, w, w, w, w, w, w, None, None, acc, out, None)

    parts = (ctypes.c_void_p * 2)(t, t + 4096)

    def anchor_post(a=p, x0=w, pp=parts):
        return L.desco_anchor_pool_post_f16x3_f32(a, 192, 192, w, w, w, 0, 0.0, w, 2, w, w, 0, 0.0, o, 64, 8, q, q, q, pp,
                                                  x0, 16, None)

    def gather_wide(x=p, out=o):
        return L.desco_csr_gather_sum_wide_f32(x, 64, q, q, 8, 4, 64, out, 64, None)

    def layer_wide(x=p, planes=w):
        return L.desco_shmp_layer_wide_f16x3_f32(x, 64, q, q, 4, 0, 8, 4, 64, planes, w, w, o, 64, None, 0, None)

    rejects("desco_shmp_layer_f32", layer_f32(x=p + 4))
    rejects("desco_shmp_layer_f32", layer_f32(ytab=t + 4))
    rejects("desco_shmp_layer_f32", layer_f32(out=o + 4))
    rejects("desco_shmp_layer_f16x3_f32", layer_f16(x=p + 4))
    rejects("desco_shmp_layer_f16x3_f32", layer_f16(planes=w + 4))
    rejects("desco_shmp_layer_f16x3_f32", layer_f16(out=o + 4))
    rejects("desco_linear64_bf16x6_f32", linear64(x=p + 4))
    rejects("desco_linear64_bf16x6_f32", linear64(planes=w + 4))
    rejects("desco_linear64_bf16x6_f32", linear64(out=o + 4))
    rejects("desco_gemm_bf16x6_f32", gemm_x6(a1=p + 4))
    rejects("desco_gemm_bf16x6_f32", gemm_x6(planes=w + 4))
    rejects("desco_gemm_f16x3_f32", gemm_f16(a1=p + 4))
    rejects("desco_gemm_f16x3_f32", gemm_f16(planes=w + 4))
    rejects("desco_gemm_tn_f32", gemm_tn(a=p + 4))
    rejects("desco_gemm_tn_f32", gemm_tn(b=t + 4))
    rejects("desco_gossip_layer_f16x3_f32", gossip_layer(h=p + 4))
    rejects("desco_gossip_layer_f16x3_f32", gossip_layer(acc=t + 4))
    rejects("desco_anchor_pool_post_f16x3_f32", anchor_post(a=p + 4))
    rejects("desco_anchor_pool_post_f16x3_f32", anchor_post(x0=w + 4))
    rejects("desco_anchor_pool_post_f16x3_f32", anchor_post(pp=(ctypes.c_void_p * 2)(t, t + 4100)))
    rejects("desco_csr_gather_sum_wide_f32", gather_wide(x=p + 4))
    rejects("desco_csr_gather_sum_wide_f32", gather_wide(out=o + 4))
    rejects("desco_shmp_layer_wide_f16x3_f32", layer_wide(x=p + 4))
    rejects("desco_shmp_layer_wide_f16x3_f32", layer_wide(planes=w + 4))
