"""desco_gossip_layer_f16x3_f32 (one gossip layer of a depth-L model, --gossip_layer_num != 2) on a CPU-only host:
declared in the header, exported by the library, bound in SIGNATURES, and bad arguments come back as DESCO_EINVAL
with a message (nothing is launched: no GPU here)."""
import os
import re

import numpy as np

from desco_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "desco_gossip_layer_f16x3_f32"


def test_gossip_layer_entry_point_is_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "desco_hip.h")).read()
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", src)
    assert hasattr(_lib.lib(), NAME)
    assert NAME in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[NAME][1]) == 17
    assert _lib.lib().desco_abi_version() == 6


BUF = np.zeros(8192, np.float32)          # host memory: every call below must fail its argument check (no launch)
BASE = BUF.ctypes.data + (-BUF.ctypes.data) % 16


def _call(**over):
    args = dict(h=BASE, rowptr=BASE + 1024, col=BASE + 2048, num_nodes=3, num_q=2, g=BASE, c3=BASE, v=BASE, w=BASE,
                ws=BASE, p=BASE, ps=BASE, pn=None, pns=None, acc=BASE + 4096, out=BASE + 8192)
    args.update(over)
    # every case differs from a valid call in exactly one way, so none of them may get as far as a launch
    assert any(args[k] is None for k in ("h", "rowptr", "col", "g", "c3", "v", "w", "ws", "p", "ps", "acc", "out")) \
        or args["num_q"] < 1 or args["num_nodes"] < 0 or (args["pn"] is None) != (args["pns"] is None) \
        or any(args[k] % 16 for k in ("h", "acc", "out")) or len({args["h"], args["acc"], args["out"]}) < 3
    return _lib.lib().desco_gossip_layer_f16x3_f32(*args.values(), None)


def test_gossip_layer_rejects_bad_arguments():
    L = _lib.lib()
    for over in (dict(h=None), dict(rowptr=None), dict(col=None), dict(g=None), dict(c3=None), dict(v=None),
                 dict(w=None), dict(ws=None), dict(p=None), dict(ps=None), dict(acc=None), dict(out=None),
                 dict(num_q=0), dict(num_nodes=-1)):
        assert _call(**over) == -1, over
        assert NAME.encode() in L.desco_last_error(), over
    assert _call(pn=BASE) == -1 and b"pn_planes" in L.desco_last_error()          # only one of pn_planes / pn_scale
    assert _call(h=BASE + 4) == -1 and b"16-byte" in L.desco_last_error()         # misaligned operands
    assert _call(out=BASE + 8196) == -1 and b"16-byte" in L.desco_last_error()
    assert _call(out=BASE) == -1 and b"distinct" in L.desco_last_error()          # out / acc aliasing h
    assert _call(acc=BASE) == -1 and b"distinct" in L.desco_last_error()


def test_gossip_layer_empty_batch_is_a_no_op():
    assert _lib.lib().desco_gossip_layer_f16x3_f32(None, None, None, 0, 1, *([None] * 11), None) == 0
