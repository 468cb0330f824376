"""The device packer's kernel bodies (csrc/pack_device.h), emulated with one thread per workgroup (tests/emul/emul_pack.cpp),
against data._pack's host route with `_pack_presorted` disabled.  Equality is exact: a packer moves and converts."""
import numpy as np
import pytest

import emul_pack_lib
import pack_cases
from tsfresh_amd import _native
from tsfresh_amd.feature_extraction import data


def test_tile_size_matches_the_cases():
    assert emul_pack_lib.tile() == pack_cases.TILE


@pytest.mark.parametrize("n", pack_cases.SIZES)
@pytest.mark.parametrize("name", sorted(pack_cases.CASES))
def test_emulated_pack_equals_host_route(name, n, monkeypatch):
    ids, sort, values = pack_cases.make_case(name, n)
    pack = pack_cases.assert_equals_host(emul_pack_lib.EmulPack, ids, sort, values, monkeypatch)
    assert not pack.value_nan
    if name == "in_order":
        assert pack.was_in_order and pack.n_passes == 0     # the early exit: nothing is sorted
    elif name in ("random", "reverse", "time_major"):
        assert not pack.was_in_order and pack.n_passes > 0


@pytest.mark.parametrize("n", (1, 2, 3))
def test_tiny_frames(n, monkeypatch):
    ids = np.array([5, 3, 5][:n], dtype=np.int64)
    sort = np.array([1, 0, 0][:n], dtype=np.int64)
    pack_cases.assert_equals_host(emul_pack_lib.EmulPack, ids, sort, np.arange(n, dtype=np.float32), monkeypatch)


def test_nan_value_sets_the_flag(monkeypatch):
    for dtype in (np.float32, np.float64):
        ids, sort, _ = pack_cases.make_case("random", 5000)
        values = np.arange(5000, dtype=dtype)
        id_col, _, sort_col, val_col = data._device_pack_columns(ids, values, sort)[1]
        assert not emul_pack_lib.EmulPack(id_col, sort_col, val_col).value_nan
        values[4321] = np.nan
        id_col, _, sort_col, val_col = data._device_pack_columns(ids, values, sort)[1]
        assert emul_pack_lib.EmulPack(id_col, sort_col, val_col).value_nan


@pytest.mark.parametrize("n", (3000, pack_cases.TILE * 3 + 5))
def test_constant_digits_are_skipped(n, monkeypatch):
    rng = np.random.default_rng(n)
    k = rng.integers(0, 1000, n)
    frames = {
        # ids 0 .. 199 and stamps 0 .. 99: one significant byte each
        "small": (rng.integers(0, 200, n), rng.integers(0, 100, n)),
        # high bytes constant: the minimum is subtracted, one byte remains of the id; the stamps span three bytes
        "high_bytes_constant": (np.int64(2 ** 40) + rng.integers(0, 200, n), np.int64(-2 ** 50) + rng.integers(0, 2 ** 20, n)),
        # a constant byte BETWEEN two that vary: bytes 0 and 2 of the id are passes, byte 1 is not
        "middle_byte_constant": ((k & 0xff) | ((k >> 8) << 16), rng.integers(0, 100, n)),
        # int32 ids below zero, no sort column
        "no_sort": ((rng.integers(-300, 300, n)).astype(np.int32), None),
    }
    for name, (ids, sort) in frames.items():
        ids = np.asarray(ids)
        values = rng.standard_normal(n).astype(np.float32)
        pack = pack_cases.assert_equals_host(emul_pack_lib.EmulPack, ids, sort, values, monkeypatch)
        assert pack.n_passes == pack_cases.expected_passes(ids, sort), name
    assert pack_cases.expected_passes(*frames["middle_byte_constant"]) == 3
    assert pack_cases.expected_passes(*frames["small"]) == 2


def test_pack_routes_through_the_device_pack(monkeypatch):
    """data._pack(pack="device") hands the prepared columns to _native.DevicePack and wraps the result: ids, lazy offsets and
    values equal the host route's; a NaN raises the reference's message; nothing else of the package is involved."""
    ids, sort, values = pack_cases.make_case("time_major", 5000)
    want = data._pack("v", ids, values, sort, pack="host")
    monkeypatch.setattr(_native, "DevicePack", emul_pack_lib.EmulPack)
    got = data._pack("v", ids, values, sort, pack="device")
    assert got.device_pack is not None and want.device_pack is None
    assert got.n_series == want.n_series and np.array_equal(got.ids, want.ids)
    assert np.array_equal(got.offsets, want.offsets)
    assert got.values.dtype == want.values.dtype and np.array_equal(np.asarray(got.values), want.values)
    assert np.array_equal(got.values[got.offsets[3]:got.offsets[4]], want.values[want.offsets[3]:want.offsets[4]])
    bad = values.copy()
    bad[17] = np.nan
    with pytest.raises(ValueError, match="Column must not contain NaN values: v"):
        data._pack("v", ids, bad, sort, nan_name="v", pack="device")
    with pytest.raises(ValueError, match="Column must not contain NaN values: v"):
        data._pack("v", ids, bad, sort, nan_name="v", pack="host")
    # a frame in packed order never reaches the device packer
    order = np.lexsort((sort, ids))
    monkeypatch.setattr(_native, "DevicePack", None)
    assert data._pack("v", ids[order], values[order], sort[order], pack="device").device_pack is None
