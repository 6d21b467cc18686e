"""The wait structure of gossip_planned_f16_kernel's query chain, read off the compiler's assembly by tools/isa_waits.py
(cross-compiles, needs hipcc but no GPU; skipped where hipcc is absent): the planned kernel shares the query chain of
gossip_fused_f16_kernel (one body in gossip_f16.hip), so it is held to the assertions of tests/test_gossip_isa_waits.py --
and to what it was written for: no SGPR parked in a VGPR lane."""
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


def test_gossip_planned_query_chain_waits():
    tool = _tool()
    if not (shutil.which(tool.hipcc()) or os.path.exists(tool.hipcc())):
        pytest.skip("hipcc not found")
    r = tool.report("gossip_f16.hip", "gossip_planned_f16_kernel")
    print(f"[isa] gossip_planned_f16_kernel query chain: {r}")
    assert "gossip_fused_f16_kernel" not in r["kernel"]
    assert r["branches"] == 0, "the query chain is expected to be straight-line code"
    assert r["mfma"] == 216
    assert r["lgkmcnt0_waits"] == 0, r["waits"]
    assert r["lds_reads_compiler"] == 0 and r["lds_writes_compiler"] == 0
    assert r["scalar_loads"] == 0
    assert r["constant_reads"] == 52                     # u, d1, tp, zp_q (4 quads each), b3 (4), 4 x (b5, w7) (8)
    assert r["min_mfma_constant_read_to_wait"] >= 6
    assert r["vgprs"] <= 256 and r["vgpr_spills"] == 0 and r["scratch_bytes"] == 0
    assert r["sgpr_spills"] == 0
