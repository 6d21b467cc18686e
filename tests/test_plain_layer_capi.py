"""The entry point of the fused plain-layer kernel (csrc/plain_layer.hip): declared, exported, in SIGNATURES, and its
argument errors come back as DESCO_EINVAL naming it, before any HIP call (so this runs on a host without a GPU)."""
import numpy as np

from desco_amd import _lib
from test_capi_symbols import declared_symbols

NAME = "desco_plain_layer_f16x3_f32"


def test_declared_exported_and_in_signatures():
    assert NAME in declared_symbols() and NAME in _lib.SIGNATURES and hasattr(_lib.lib(), NAME)
    assert len(_lib.SIGNATURES[NAME][1]) == 21
    assert _lib.lib().desco_abi_version() == 6                    # an addition: the ABI version stays


def test_bad_arguments_are_refused_by_name_before_any_launch():
    L = _lib.lib()
    buf = np.zeros(4 * 64 * 64 + 64, np.float32)
    p = buf.ctypes.data + (-buf.ctypes.data % 16)                 # 16-byte aligned host memory: never dereferenced
    idx = np.zeros(16, np.int32).ctypes.data
    out = np.zeros(64 * 8 + 8, np.float32)
    o = out.ctypes.data + (-out.ctypes.data % 16)
    good = dict(x=p, ldx=64, rowptr=idx, col=idx, s=None, row0=0, num_rows=8, width=64, mats=2, w1=p, s1=p, b1=p, w2=p, s2=p,
                b2=p, out=o, ldo=64, out2=None, ld2=0, out2_row0=0)

    def call(**over):
        a = dict(good, **over)
        return L.desco_plain_layer_f16x3_f32(a["x"], a["ldx"], a["rowptr"], a["col"], a["s"], a["row0"], a["num_rows"],
                                             a["width"], a["mats"], a["w1"], a["s1"], a["b1"], a["w2"], a["s2"], a["b2"],
                                             a["out"], a["ldo"], a["out2"], a["ld2"], a["out2_row0"], None)
    bad = [dict(x=None), dict(rowptr=None), dict(col=None), dict(w1=None), dict(s1=None), dict(b1=None), dict(w2=None),
           dict(s2=None), dict(b2=None), dict(out=None), dict(x=p + 4), dict(w1=p + 2), dict(w2=p + 8), dict(ldx=66),
           dict(ldx=60), dict(ldo=63), dict(out2=o, ld2=32), dict(width=96), dict(width=320), dict(mats=0), dict(mats=3),
           dict(out=p), dict(out2=p, ld2=64), dict(row0=-1), dict(num_rows=-1), dict(out2_row0=-1),
           dict(num_rows=64 * 2 ** 31 + 1)]
    for over in bad:
        L.desco_gemm_f32_multi(5, None, None)                     # (another entry point's message in between)
        assert call(**over) == -1, over
        assert NAME.encode() in L.desco_last_error(), over
    assert call(num_rows=0) == 0                                  # nothing to do: no launch
    assert call(num_rows=0, mats=1, w2=None, s2=None, b2=None) == 0
