"""The device batch set-up entry points (csrc/batch_dev.hip) at the C ABI, on a CPU-only host: declared, exported, bound,
and every bad argument comes back as DESCO_EINVAL naming the entry point before any HIP call; empty blocks return 0
without a launch.  (What they compute is checked on the GPU: tests/test_batch_dev_gpu.py.)"""
import os
import re

import numpy as np

from desco_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("desco_partition_dev_slice", "desco_partition_dev_degree_sort",
                "desco_partition_dev_degree_sort_workspace", "desco_pool_index_dev", "desco_neigh_rows_dev")


def test_entry_points_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "desco_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = _lib.lib()
    for n in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % n, src), f"{n} not declared in include/desco_hip.h"
        assert hasattr(L, n), f"{n} not exported"
        assert n in _lib.SIGNATURES, f"{n} not bound in _lib.SIGNATURES"
    assert L.desco_abi_version() == _lib.ABI_VERSION == 6
    assert int(re.search(r"#define DESCO_ABI_VERSION (\d+)", src).group(1)) == 6


def _rejects(L, name, rc):
    assert rc == -1, name
    assert name.encode() in L.desco_last_error(), (name, L.desco_last_error())
    assert L.desco_rng_next(None, None, None) == -1          # (another message, so the next case cannot pass on this one)


def test_bad_arguments_are_refused_by_name():
    L = _lib.lib()
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data          # a valid (host) address: no call below may reach a launch
    # slice(count_ptr, vrowptr, vcol, count_orig, B, Nc, b0, b1, block_count, block_edges, outs x4, stream)
    _rejects(L, "desco_partition_dev_slice", L.desco_partition_dev_slice(None, p, p, p, 4, 8, 0, 2, 3, 5, p, p, p, p, None))
    _rejects(L, "desco_partition_dev_slice", L.desco_partition_dev_slice(p, None, p, p, 4, 8, 0, 2, 3, 5, p, p, p, p, None))
    _rejects(L, "desco_partition_dev_slice", L.desco_partition_dev_slice(p, p, p, p, 4, 8, 0, 2, 3, 5, None, p, p, p, None))
    _rejects(L, "desco_partition_dev_slice", L.desco_partition_dev_slice(p, p, p, p, 4, 8, 0, 2, 3, 5, p, p, None, p, None))
    _rejects(L, "desco_partition_dev_slice", L.desco_partition_dev_slice(p, p, None, p, 4, 8, 0, 2, 3, 5, p, p, p, p, None))
    _rejects(L, "desco_partition_dev_slice", L.desco_partition_dev_slice(p, p, p, None, 4, 8, 0, 2, 3, 5, p, p, p, p, None))
    _rejects(L, "desco_partition_dev_slice", L.desco_partition_dev_slice(p, p, p, p, 4, 8, 3, 2, 3, 5, p, p, p, p, None))   # b0 > b1
    _rejects(L, "desco_partition_dev_slice", L.desco_partition_dev_slice(p, p, p, p, 4, 8, -1, 2, 3, 5, p, p, p, p, None))
    _rejects(L, "desco_partition_dev_slice", L.desco_partition_dev_slice(p, p, p, p, 4, 8, 0, 5, 3, 5, p, p, p, p, None))   # b1 > B
    _rejects(L, "desco_partition_dev_slice", L.desco_partition_dev_slice(p, p, p, p, -4, 8, 0, 0, 0, 0, p, p, p, p, None))
    _rejects(L, "desco_partition_dev_slice", L.desco_partition_dev_slice(p, p, p, p, 4, -8, 0, 2, 3, 5, p, p, p, p, None))
    _rejects(L, "desco_partition_dev_slice", L.desco_partition_dev_slice(p, p, p, p, 4, 8, 0, 2, -3, 5, p, p, p, p, None))
    _rejects(L, "desco_partition_dev_slice", L.desco_partition_dev_slice(p, p, p, p, 4, 8, 0, 2, 3, -5, p, p, p, p, None))
    # degree_sort(count_ptr, B, Nc, E, vrowptr, vcol, count_orig, key, key_stride, outs x3, workspace, blocks, stream)
    name = "desco_partition_dev_degree_sort"
    f = L.desco_partition_dev_degree_sort
    _rejects(L, name, f(None, 2, 6, 9, p, p, p, p, 2, p, p, p, p, 0, None))
    _rejects(L, name, f(p, 2, 6, 9, None, p, p, p, 2, p, p, p, p, 0, None))
    _rejects(L, name, f(p, 2, 6, 9, p, None, p, p, 2, p, p, p, p, 0, None))
    _rejects(L, name, f(p, 2, 6, 9, p, p, None, p, 2, p, p, p, p, 0, None))
    _rejects(L, name, f(p, 2, 6, 9, p, p, p, p, 2, None, p, p, p, 0, None))
    _rejects(L, name, f(p, 2, 6, 9, p, p, p, p, 2, p, None, p, p, 0, None))
    _rejects(L, name, f(p, 2, 6, 9, p, p, p, p, 2, p, p, None, p, 0, None))
    _rejects(L, name, f(p, 2, 6, 9, p, p, p, p, 2, p, p, p, None, 0, None))      # no workspace
    _rejects(L, name, f(p, -2, 6, 9, p, p, p, p, 2, p, p, p, p, 0, None))
    _rejects(L, name, f(p, 2, -6, 9, p, p, p, p, 2, p, p, p, p, 0, None))
    _rejects(L, name, f(p, 2, 6, -9, p, p, p, p, 2, p, p, p, p, 0, None))
    _rejects(L, name, f(p, 2, 6, 9, p, p, p, p, 0, p, p, p, p, 0, None))         # key stride 0
    _rejects(L, name, f(p, 2, 6, 9, p, p, p, p, 2, p, p, p, p, -1, None))        # negative geometry
    _rejects(L, name, f(p, 2, 2 ** 30, 9, p, p, p, p, 2, p, p, p, p, 0, None))   # 4 rows + 1 beyond int32
    # pool_index(count_ptr, B, Nc, bits, slot, totals, stream)
    name = "desco_pool_index_dev"
    _rejects(L, name, L.desco_pool_index_dev(None, 3, 40, p, p, p, None))
    _rejects(L, name, L.desco_pool_index_dev(p, 3, 40, None, p, p, None))
    _rejects(L, name, L.desco_pool_index_dev(p, 3, 40, p, None, p, None))
    _rejects(L, name, L.desco_pool_index_dev(p, 3, 40, p, p, None, None))
    _rejects(L, name, L.desco_pool_index_dev(p, -3, 40, p, p, p, None))
    _rejects(L, name, L.desco_pool_index_dev(p, 3, -40, p, p, p, None))
    # neigh_rows(neigh_index, B, graph_ptr, G, scatter, ngp, stream)
    name = "desco_neigh_rows_dev"
    _rejects(L, name, L.desco_neigh_rows_dev(None, 3, p, 2, p, p, None))
    _rejects(L, name, L.desco_neigh_rows_dev(p, 3, None, 2, p, p, None))
    _rejects(L, name, L.desco_neigh_rows_dev(p, 3, p, 2, None, p, None))
    _rejects(L, name, L.desco_neigh_rows_dev(p, 3, p, 2, p, None, None))
    _rejects(L, name, L.desco_neigh_rows_dev(p, -3, p, 2, p, p, None))
    _rejects(L, name, L.desco_neigh_rows_dev(p, 3, p, -2, p, p, None))


def test_empty_blocks_return_zero_without_a_launch():
    L = _lib.lib()
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data
    assert L.desco_partition_dev_slice(p, p, None, None, 4, 8, 2, 2, 0, 0, p, None, p, None, None) == 0      # b0 == b1
    assert L.desco_partition_dev_slice(p, p, None, None, 0, 0, 0, 0, 0, 0, p, None, p, None, None) == 0
    assert L.desco_partition_dev_degree_sort(p, 0, 0, 0, p, None, None, None, 0, None, p, None, None, 0, None) == 0
    assert L.desco_pool_index_dev(p, 0, 0, None, None, p, None) == 0
    assert L.desco_neigh_rows_dev(None, 0, p, 5, None, p, None) == 0
    assert not buf.any()                                        # and nothing was written


def test_workspace_query():
    L = _lib.lib()
    q = L.desco_partition_dev_degree_sort_workspace
    assert q(0, 0) == 0 and q(-1, 5) == 0
    # keys of neighborhoods above the LDS limit (int64) + order + new_of_old + renamed sources (int32 each)
    assert q(1000, 5000) == 16 * 1000 + 4 * 5000
    assert q(3, 0) >= 16 * 3
