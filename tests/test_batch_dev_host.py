"""Lazy host views of a device-resident NeighborhoodPartition, on a CPU-only host: CPU tensors stand in for the device
arrays.  A field is downloaded the first time it is read and only then; the sizes never download anything; a partition
built from numpy arrays behaves as it always did."""
import numpy as np
import pytest
import torch

from helpers import golden_graphs

from desco_amd.batch import NeighborhoodBatch
from desco_amd.graphs import GraphSet
from desco_amd.partition import NeighborhoodPartition, build_partition

FIELDS = ("neigh_index", "indicator", "count_ptr", "count_orig", "vrowptr", "vcol")


def _host_part():
    return build_partition(GraphSet.from_edge_lists(golden_graphs(max_n=30)[:12]), 4)


def _stand_in(host):
    da = {"device": torch.device("cpu")}
    for f in FIELDS:
        a = getattr(host, f)
        da[f] = torch.from_numpy(np.ascontiguousarray(a.astype(np.uint8) if f == "indicator" else a).copy())
    return NeighborhoodPartition.from_device_arrays(da, host.num_neigh, host.num_count, host.num_edges, host.depth)


def test_sizes_never_download():
    host = _host_part()
    dev = _stand_in(host)
    assert (dev.num_neigh, dev.num_count, dev.num_rows, dev.num_edges, len(dev)) == \
        (host.num_neigh, host.num_count, host.num_rows, host.num_edges, len(host))
    assert host.num_neigh > 0 and host.num_edges > 0
    assert dev.downloads == {f: 0 for f in FIELDS}


def test_a_field_is_downloaded_on_first_access_only():
    host = _host_part()
    dev = _stand_in(host)
    for k, f in enumerate(FIELDS):
        a = getattr(dev, f)
        assert isinstance(a, np.ndarray) and a.dtype == getattr(host, f).dtype, f
        assert np.array_equal(a, getattr(host, f)), f
        assert getattr(dev, f) is a, f                              # kept: the second read is the same array
        assert dev.downloads == {g: int(j <= k) for j, g in enumerate(FIELDS)}, f
    assert dev.indicator.dtype == np.bool_


def test_device_arrays_keeps_its_keys_and_feeds_the_batch_without_upload():
    host = _host_part()
    dev = _stand_in(host)
    assert isinstance(dev.device_arrays, dict)
    assert {"device", "count_ptr", "vrowptr", "vcol", "neigh_index", "indicator", "count_orig"} <= set(dev.device_arrays)
    b = NeighborhoodBatch(dev, "cpu")
    for f in ("count_ptr", "vrowptr", "vcol"):
        assert getattr(b, f).data_ptr() == dev.device_arrays[f].data_ptr(), f
    assert (b.num_graphs, b.num_count, b.num_rows) == (host.num_neigh, host.num_count, host.num_rows)
    assert dev.downloads == {f: 0 for f in FIELDS}


def test_host_methods_work_on_a_device_resident_partition():
    host = _host_part()
    dev = _stand_in(host)
    B = host.num_neigh
    for a, b in ((dev.slice(1, B - 1), host.slice(1, B - 1)), (dev.degree_sorted(1), host.degree_sorted(1)),
                 (dev.select([0, 2, B - 1]), host.select([0, 2, B - 1]))):
        for f in FIELDS:
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
    da, hb = dev.edge_index_dict(), host.edge_index_dict()
    assert da.keys() == hb.keys() and all(np.array_equal(da[k], hb[k]) for k in hb)
    assert all(n == 1 for n in dev.downloads.values())


def test_numpy_built_partition_is_unchanged():
    host = _host_part()
    p = NeighborhoodPartition(host.neigh_index, host.indicator, host.count_ptr, host.count_orig, host.vrowptr,
                              host.vcol, 3, 2)                                    # positional, as the tests build it
    assert p.depth == 3 and p.quirk_batch == 2 and p.device_arrays is None
    for f in FIELDS:
        assert getattr(p, f) is getattr(host, f), f
    assert p.num_neigh == len(host.count_ptr) - 1 and p.num_count == int(host.count_ptr[-1])
    assert p.num_edges == int(host.vrowptr[-1]) and p.num_rows == p.num_count + p.num_neigh
    q = NeighborhoodPartition(neigh_index=host.neigh_index, indicator=host.indicator, count_ptr=host.count_ptr,
                              count_orig=host.count_orig, vrowptr=host.vrowptr, vcol=host.vcol)
    assert q.depth == 4 and q.quirk_batch == 0 and q.vcol is host.vcol
    q.vcol = host.vcol[:3]                                           # fields stay assignable
    assert len(q.vcol) == 3
    assert p.downloads == {f: 0 for f in FIELDS}
    with pytest.raises(RuntimeError, match="built on the device"):
        p.slice_device(0, 1)
    with pytest.raises(RuntimeError, match="built on the device"):
        p.degree_sorted_device()
    # the batch of a host partition on the CPU keeps the numpy pooling index
    b = NeighborhoodBatch(host.degree_sorted(1), "cpu")
    bits, slot, n = b.pool_index()
    assert bits.dtype == torch.int32 and slot.numel() == (host.num_count + 15) // 16 and n >= host.num_neigh
    assert b.max_count_rows() == int(np.diff(host.count_ptr).max())
