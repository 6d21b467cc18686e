"""desco_anchor_pool_post_f16x3_f32 (anchor MLP + pooled sums + post_mp.0 in one launch) on a CPU-only host: declared in
the header, exported by the library, bound in SIGNATURES, and bad arguments come back as DESCO_EINVAL with a message
(nothing is launched: no GPU here)."""
import ctypes
import os
import re

import numpy as np

from desco_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "desco_anchor_pool_post_f16x3_f32"


def test_anchor_post_entry_point_is_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "desco_hip.h")).read()
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", src)
    assert hasattr(_lib.lib(), NAME)
    assert len(_lib.SIGNATURES[NAME][1]) == 24
    assert _lib.lib().desco_abi_version() == 6


BUF = np.zeros(8192, np.float32)          # host memory: every call below must fail its argument check (no launch)
BASE = BUF.ctypes.data + (-BUF.ctypes.data) % 16
PARTS = (ctypes.c_void_p * 8)(*([BASE] * 8))


def _call(**over):
    args = dict(a=BASE, lda=512, k=512, aw=BASE, ascale=BASE, abias=BASE, act=2, slope=0.1, row_scale=BASE, L=8,
                w0=BASE, b0=BASE, act0=2, slope0=0.1, out=BASE, ldo=64, m=1000, seg_ptr=BASE, bits=BASE, slot=BASE,
                parts=PARTS, x0=BASE, tile_rows=16)
    args.update(over)
    return _lib.lib().desco_anchor_pool_post_f16x3_f32(*args.values(), None)


def test_anchor_post_rejects_bad_arguments():
    L = _lib.lib()
    for over in (dict(a=None), dict(aw=None), dict(ascale=None), dict(row_scale=None), dict(w0=None), dict(out=None),
                 dict(seg_ptr=None), dict(bits=None), dict(slot=None), dict(parts=None), dict(x0=None),
                 dict(L=0), dict(L=9), dict(L=7, k=448), dict(L=3, k=192), dict(k=480), dict(k=544),
                 dict(tile_rows=32), dict(lda=510), dict(lda=256), dict(ldo=32), dict(m=-1), dict(m=(1 << 24) + 1),
                 dict(a=BASE + 4), dict(aw=BASE + 4), dict(w0=BASE + 8), dict(x0=BASE + 4),
                 dict(parts=(ctypes.c_void_p * 8)(*([BASE] * 7 + [None]))),
                 dict(parts=(ctypes.c_void_p * 8)(*([BASE] * 7 + [BASE + 4])))):
        assert _call(**over) == -1, over
        assert NAME.encode() in L.desco_last_error(), over


def test_anchor_post_empty_batch_is_a_no_op():
    assert _call(m=0, a=None) == 0
