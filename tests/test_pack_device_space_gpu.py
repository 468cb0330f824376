"""tsfa_pack_device with space=TSFA_DEVICE: columns that already lie in HBM are packed in place, nothing is staged.  Only the
C-ABI reaches that branch (`_native.DevicePack` always passes TSFA_HOST), so the test calls the bound library itself and
compares the pack bit for bit with a `DevicePack` of the same host columns."""
import ctypes

import numpy as np
import pytest

import pack_cases
from tsfresh_amd import _native

pytestmark = pytest.mark.gpu


def _shuffled(n):
    """Crosses a tile boundary and is out of order: the sort runs passes between both buffer sets."""
    rng = np.random.default_rng(3)
    return rng.integers(-20, 30, n).astype(np.int64), rng.permutation(n).astype(np.int64), rng.standard_normal(n).astype(np.float32)


def _in_order(n):
    """Already grouped and sorted: one buffer set, no pass."""
    rng = np.random.default_rng(4)
    return (np.repeat(np.arange(10, dtype=np.int64), n // 10), np.tile(np.arange(n // 10, dtype=np.int64), 10),
            rng.standard_normal(n).astype(np.float32))


@pytest.mark.parametrize("frame, n, in_order", [(_shuffled, pack_cases.TILE + 1, False), (_in_order, 1000, True)])
def test_device_columns_pack_like_host_columns(gpu, frame, n, in_order):
    import torch

    ids, sort, values = frame(n)
    want = _native.DevicePack((ids, _native.TSFA_I64), (sort, _native.TSFA_I64), (values, _native.TSFA_F32), keep_sort=True)
    assert want.was_in_order == in_order and (want.n_passes == 0) == in_order and want.n_rows == n

    d_ids, d_sort, d_values = (torch.from_numpy(a).to("cuda:0") for a in (ids, sort, values))
    torch.cuda.synchronize(0)
    lib = _native.load()
    handle = ctypes.c_void_p()
    _native._check(lib, lib.tsfa_pack_device(d_ids.data_ptr(), _native.TSFA_I64, d_sort.data_ptr(), _native.TSFA_I64,
                                             d_values.data_ptr(), _native.TSFA_F32, n, _native.TSFA_DEVICE,
                                             _native.TSFA_PACK_KEEP_SORT, 0, ctypes.byref(handle)))
    got = _native.DevicePack.__new__(_native.DevicePack)   # as DevicePackSet.values wraps its handles
    got._adopt(lib, handle, 0, ids.dtype, sort.dtype)
    try:
        assert (got.n_rows, got.n_series, got.flags, got.n_passes) == (want.n_rows, want.n_series, want.flags, want.n_passes)
        assert got.values_type == want.values_type
        assert np.array_equal(got.values_host().view(np.uint32), want.values_host().view(np.uint32))
        assert np.array_equal(got.offsets, want.offsets)
        assert got.ids.dtype == want.ids.dtype and np.array_equal(got.ids, want.ids)
        assert got.sort.dtype == want.sort.dtype and np.array_equal(got.sort, want.sort)
    finally:
        got.close()
        want.close()
