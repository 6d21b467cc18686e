"""The wait structure of gossip_fused_f16_kernel's query chain, read off the compiler's assembly by tools/isa_waits.py
(cross-compiles, needs hipcc but no GPU; skipped where hipcc is absent).

Between the first and the last MFMA of a query the kernel's LDS traffic is its own ordered inline-asm stream -- the weight
ring and the epilogue constants requested ahead -- and every wait is a counted one.  What the counted waits rest on is
asserted here on the ISA: no compiler-issued LDS read, no `lgkmcnt(0)`, no scalar memory load (those return out of order
and share the counter), every constant read at least one pair step (six MFMAs) in front of the wait that covers it, and
the register budget of two waves per SIMD without spilling (VGPR spills and scratch; the SGPRs the compiler parks in
VGPR lanes do not touch memory and are not counted)."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("isa_waits", os.path.join(ROOT, "tools", "isa_waits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_gossip_f16_query_chain_waits():
    tool = _tool()
    if not (shutil.which(tool.hipcc()) or os.path.exists(tool.hipcc())):
        pytest.skip("hipcc not found")
    r = tool.report("gossip_f16.hip", "gossip_fused_f16_kernel")
    print(f"[isa] gossip_fused_f16_kernel query chain: {r}")
    assert r["branches"] == 0, "the query chain is expected to be straight-line code"
    assert r["mfma"] == 216
    assert r["lgkmcnt0_waits"] == 0, r["waits"]
    assert r["lds_reads_compiler"] == 0 and r["lds_writes_compiler"] == 0
    assert r["scalar_loads"] == 0
    assert r["constant_reads"] == 52                     # u, d1, tp, zp_q (4 quads each), b3 (4), 4 x (b5, w7) (8)
    assert r["min_mfma_constant_read_to_wait"] >= 6
    assert r["vgprs"] <= 256 and r["vgpr_spills"] == 0 and r["scratch_bytes"] == 0
