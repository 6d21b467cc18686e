"""The three entry points of the wide neighborhood path (csrc/shmp_wide.hip): declared, exported, in SIGNATURES, and
argument errors reported without a launch (no GPU needed)."""
from desco_amd import _lib

NEW = ("desco_shmp_layer_wide_f16x3_f32", "desco_csr_gather_sum_wide_f32", "desco_count_head_wide_f32")


def test_wide_symbols_are_declared_exported_and_bound():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "desco_hip.h")).read()
    L = _lib.lib()
    for n in NEW:
        assert n + "(" in hdr and n in _lib.SIGNATURES and hasattr(L, n), n
    assert L.desco_abi_version() == 6


def test_wide_entry_points_validate_their_arguments():
    L = _lib.lib()
    # width 96 is no padded width; slots 3 is no slot count; vslots below slots
    assert L.desco_shmp_layer_wide_f16x3_f32(None, 96, None, None, 4, 0, 10, 4, 96, None, None, None, None, 0, None, 0,
                                             None) == -1
    assert b"desco_shmp_layer_wide_f16x3_f32" in L.desco_last_error()
    assert L.desco_shmp_layer_wide_f16x3_f32(None, 128, None, None, 2, 0, 10, 4, 128, None, None, None, None, 0, None,
                                             0, None) == -1
    assert L.desco_shmp_layer_wide_f16x3_f32(None, 128, None, None, 4, 0, 10, 4, 128, None, None, None, None, 0, None,
                                             0, None) == -1        # NULL pointers
    assert L.desco_csr_gather_sum_wide_f32(None, 260, None, None, 10, 1, 260, None, 260, None) == -1
    assert b"desco_csr_gather_sum_wide_f32" in L.desco_last_error()
    assert L.desco_csr_gather_sum_wide_f32(None, 128, None, None, 10, 3, 128, None, 128, None) == -1
    assert L.desco_count_head_wide_f32(None, 1088, None, 1088, 1088, None, 0.0, None, 0.01, 0, None, 29, 10, 29,
                                       None) == -1
    assert b"up to 1024" in L.desco_last_error()
    assert L.desco_count_head_wide_f32(None, 512, None, 512, 512, None, 0.0, None, 0.01, 0, None, 33, 10, 33,
                                       None) == -1
    # nothing to do is no error
    assert L.desco_count_head_wide_f32(None, 512, None, 512, 512, None, 0.0, None, 0.01, 0, None, 29, 0, 29, None) == 0
