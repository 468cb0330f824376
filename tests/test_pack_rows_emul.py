"""The row packer's kernel bodies (tsfresh_amd/csrc/pack_rows.h: tsfa_pack_set_rows, tsfa_pack_set_hours) on the CPU: the g++
-DTSFA_EMUL build, one thread per workgroup, against numpy (`values[perm]`, `astype(float64)`) and against
`data._hours_since_first` on the DatetimeIndex of the same stamps -- exactly.  No GPU needed; tests/test_pack_rows_gpu.py
compares the GPU with this emulation."""
import os
import subprocess

import numpy as np
import pandas as pd
import pytest

import emul_pack_rows_lib as epr
from tsfresh_amd import _native
from tsfresh_amd.feature_extraction import data

ALL_TYPES = (np.float32, np.float64, np.int64, np.uint64, np.int32, np.uint32, np.int16, np.uint16, np.int8, np.uint8, np.bool_)
MAX_TILE_C = 32
COLS = (1, 2, 3, MAX_TILE_C - 1, MAX_TILE_C, MAX_TILE_C + 1, 2 * MAX_TILE_C + 1)


def row_counts(n_cols):
    tile = epr.geometry(n_cols)["tile_t"]
    return (1, tile - 1, tile, tile + 1, 3 * tile + 5)


def make_values(rng, shape, dtype):
    if dtype == np.bool_:
        return rng.integers(0, 2, size=shape).astype(np.bool_)
    if np.dtype(dtype).kind == "f":
        return rng.standard_normal(shape).astype(dtype)
    info = np.iinfo(dtype)
    v = rng.integers(info.min, info.max, size=shape, dtype=dtype, endpoint=True)
    v.reshape(-1)[:2] = (info.min, info.max)[:v.size]   # the extremes: 64-bit integers beyond 2^53 round to nearest even
    return v


def layouts(rng, n, c, dtype):
    """(name, [n, c] view) for a row-major matrix, a column-major one, and two sliced views whose gaps hold NaN (floats; a
    load outside the view would raise a column's flag) or other numbers."""
    base = make_values(rng, (n, c), dtype)
    yield "row-major", np.ascontiguousarray(base)
    yield "column-major", np.asfortranarray(base)
    for name, sl in (("sliced rows, unit columns", (slice(1, None, 2), slice(1, 1 + c))),
                     ("sliced rows and columns", (slice(0, None, 3), slice(1, 1 + 2 * c, 2)))):
        big = make_values(rng, (3 * n + 2, 2 * c + 3), dtype)
        if np.dtype(dtype).kind == "f":
            big[...] = np.nan
        view = big[sl][:n]
        assert view.shape == (n, c)
        view[...] = base
        yield name, view


def check_rows(view, perm, **kw):
    res = epr.EmulRows(view, perm, **kw)
    odt = np.float32 if view.dtype == np.float32 else np.float64
    want = view[perm].astype(odt).T
    assert res.status >= 0 and res.guards_intact
    assert res.columns.dtype == odt and np.array_equal(res.columns.view(np.uint32 if odt == np.float32 else np.uint64),
                                                       np.ascontiguousarray(want).view(np.uint32 if odt == np.float32 else np.uint64))
    assert not res.nan.any()
    return res


@pytest.mark.parametrize("dtype", ALL_TYPES, ids=lambda d: np.dtype(d).name)
def test_rows_every_type_shape_and_layout(dtype):
    rng = np.random.default_rng(11)
    routes = set()
    for c in COLS:
        for n in row_counts(c):
            perm = rng.permutation(n).astype(np.uint32)
            for name, view in layouts(rng, n, c, dtype):
                res = check_rows(view, perm)
                routes.add((res.status, name))
    # the tiles route takes what has unit column stride and several columns, the gather everything else
    assert (0, "row-major") in routes and (0, "sliced rows, unit columns") in routes
    assert (1, "column-major") in routes and (1, "sliced rows and columns") in routes and (1, "row-major") in routes   # (C = 1)


@pytest.mark.parametrize("c", (1, 3, MAX_TILE_C + 1))
def test_rows_fewer_workgroups_than_tiles_and_identity(c):
    rng = np.random.default_rng(5)
    n = row_counts(c)[-1]
    x = make_values(rng, (n, c), np.float64)
    perm = rng.permutation(n).astype(np.uint32)
    full = check_rows(x, perm)
    for wgs in (1, 2, 3):
        assert np.array_equal(check_rows(x, perm, n_workgroups=wgs).columns, full.columns)
        assert np.array_equal(check_rows(np.asfortranarray(x), perm, n_workgroups=wgs).columns, full.columns)
    # an in-order set keeps the identity
    ident = check_rows(x, np.arange(n, dtype=np.uint32))
    assert np.array_equal(ident.columns, x.T)


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_rows_nan_flag_per_column(dtype):
    rng = np.random.default_rng(3)
    for c, bad_cols in ((1, (0,)), (3, (1,)), (MAX_TILE_C + 1, (0, MAX_TILE_C)), (2 * MAX_TILE_C + 1, (MAX_TILE_C - 1, 2 * MAX_TILE_C))):
        n = row_counts(c)[-1]
        x = make_values(rng, (n, c), dtype)
        perm = rng.permutation(n).astype(np.uint32)
        for col in bad_cols:
            x[rng.integers(0, n), col] = np.nan
        for view in (x, np.asfortranarray(x)):
            res = epr.EmulRows(view, perm)
            assert res.status >= 0 and res.guards_intact
            assert sorted(np.nonzero(res.nan)[0]) == sorted(bad_cols)
            got, want = res.columns, x[perm].T
            assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])


def test_rows_refusals():
    x = np.zeros((4, 3))
    perm = np.arange(4, dtype=np.uint32)
    lib = epr.load()
    out, flags = np.zeros(12), np.zeros(3, dtype=np.uint32)
    for args in ((0, 1, 3, 1), (4, 0, 3, 1), (4, 3, -3, 1), (4, 3, 3, -1)):
        n, c, sr, sc = args
        assert lib.tsfa_emul_pack_rows(x.ctypes.data, _native.TSFA_F64, perm.ctypes.data, n, c, sr, sc, out.ctypes.data, flags.ctypes.data, 0) < 0
    assert lib.tsfa_emul_pack_rows(x.ctypes.data, 99, perm.ctypes.data, 4, 3, 3, 1, out.ctypes.data, flags.ctypes.data, 0) < 0
    assert lib.tsfa_emul_pack_rows(None, _native.TSFA_F64, perm.ctypes.data, 4, 3, 3, 1, out.ctypes.data, flags.ctypes.data, 0) < 0


# ---------------------------------------------------------------------------------------------
# hours
# ---------------------------------------------------------------------------------------------
TILE = 4096
UNITS = {"s": 1, "ms": 10 ** 3, "us": 10 ** 6, "ns": 10 ** 9}


def frame_keys(rng):
    """ids, kinds and sort keys of a frame of two kinds, rows shuffled: groups of 1 and 2 rows, a group that ends on a tile
    edge, a tile made only of one-row groups, a group spanning three tiles, and the same id on either side of the kinds'
    boundary."""
    lengths0 = [1, 2, 5, TILE - 8] + [1] * TILE + [2 * TILE + 10, 1, 2]
    lengths1 = [2, 1, 700, 1]
    assert sum(lengths0[:4]) == TILE and sum(lengths0[:4 + TILE]) == 2 * TILE
    ids, kinds, sort = [], [], []
    for kind, lengths in enumerate((lengths0, lengths1)):
        # kind 1 starts with the id kind 0 ends with
        first_id = 100 if kind == 0 else 100 + len(lengths0) - 1
        for g, length in enumerate(lengths):
            ids.append(np.full(length, first_id + g))
            kinds.append(np.full(length, kind))
            sort.append(rng.permutation(length))
    ids, kinds, sort = (np.concatenate(a).astype(np.int64) for a in (ids, kinds, sort))
    shuffle = rng.permutation(len(ids))
    return ids[shuffle], kinds[shuffle], sort[shuffle]


def reference_hours(ticks, unit, perm, offsets):
    index = pd.DatetimeIndex(ticks.view("M8[%s]" % unit))
    assert str(index.dtype) == "datetime64[%s]" % unit
    return data._hours_since_first(index, perm.astype(np.int64), offsets)


def assert_same_bits(got, want):
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok].view(np.uint64), want[ok].view(np.uint64))


@pytest.fixture(scope="module")
def keys():
    rng = np.random.default_rng(23)
    ids, kinds, sort = frame_keys(rng)
    perm, offsets = epr.sort_order(ids, sort, kinds)
    return ids, kinds, sort, perm, offsets


@pytest.mark.parametrize("unit", sorted(UNITS))
def test_hours_units_against_the_datetime_index(keys, unit):
    ids, kinds, sort, perm, offsets = keys
    rng = np.random.default_rng(31)
    # stamps that do not ascend, two centuries wide in the unit's ticks
    ticks = rng.integers(-3 * 10 ** 9, 3 * 10 ** 9, size=len(ids)) * UNITS[unit] + rng.integers(0, UNITS[unit], size=len(ids))
    want = reference_hours(ticks, unit, perm, offsets)
    for wgs in (0, 2):
        res = epr.EmulHours(ticks, UNITS[unit], perm, offsets, n_workgroups=wgs)
        assert res.status == 0 and res.guards_intact and res.flags == 0
        assert_same_bits(res.hours, want)
    # a stepped view of the stamps is read through its stride
    wide = np.zeros(2 * len(ticks), dtype=np.int64)
    wide[::2] = ticks
    res = epr.EmulHours(wide[::2], UNITS[unit], perm, offsets)
    assert res.status == 0 and res.flags == 0
    assert_same_bits(res.hours, want)


def test_hours_float_seconds(keys):
    ids, kinds, sort, perm, offsets = keys
    rng = np.random.default_rng(37)
    whole = rng.integers(-3 * 10 ** 9, 3 * 10 ** 9, size=len(ids))
    res = epr.EmulHours(whole.astype(np.float64), 1, perm, offsets)
    assert res.status == 0 and res.guards_intact and res.flags == 0
    assert_same_bits(res.hours, reference_hours(whole, "s", perm, offsets))   # whole seconds: the frame with a [s] index
    frac = rng.standard_normal(len(ids)) * 1e6
    first = frac[perm][np.repeat(offsets[:-1], np.diff(offsets))]
    res = epr.EmulHours(frac, 1, perm, offsets)
    assert_same_bits(res.hours, (frac[perm] - first) / 3600.0)   # the documented arithmetic


def test_hours_missing_stamps(keys):
    ids, kinds, sort, perm, offsets = keys
    rng = np.random.default_rng(41)
    ticks = rng.integers(0, 10 ** 15, size=len(ids))
    nat = np.iinfo(np.int64).min
    big = int(np.argmax(np.diff(offsets)))            # the group spanning three tiles
    first_of = lambda g: perm[offsets[g]]             # noqa: E731
    inside_of = lambda g: perm[offsets[g] + 3]        # noqa: E731
    for rows in ([first_of(big)], [inside_of(big)], [first_of(0)], [inside_of(2), first_of(len(offsets) - 2)]):
        t = ticks.copy()
        t[rows] = nat
        want = reference_hours(t, "ns", perm, offsets)
        assert np.isnan(want).any()
        res = epr.EmulHours(t, 10 ** 9, perm, offsets)
        assert res.status == 0 and res.guards_intact and res.flags == 16   # TSFA_DENSE_BAD_TIME
        assert_same_bits(res.hours, want)
        sec = t.astype(np.float64)
        sec[rows] = np.nan
        res = epr.EmulHours(sec, 1, perm, offsets)
        assert res.flags == 16 and np.array_equal(np.isnan(res.hours), np.isnan(want))


def test_hours_small_frames_and_one_kind():
    rng = np.random.default_rng(43)
    for lengths in ([1], [2], [1, 1, 2], [TILE], [TILE, 1], [TILE - 1, 2, TILE - 1], [3] * 1500):
        ids = np.repeat(np.arange(len(lengths)), lengths)
        shuffle = rng.permutation(len(ids))
        ids = ids[shuffle]
        sort = rng.permutation(len(ids))
        perm, offsets = epr.sort_order(ids, sort)
        assert list(np.diff(offsets)) == lengths
        ticks = rng.integers(0, 10 ** 18, size=len(ids))
        res = epr.EmulHours(ticks, 10 ** 9, perm, offsets)
        assert res.status == 0 and res.guards_intact and res.flags == 0
        assert_same_bits(res.hours, reference_hours(ticks, "ns", perm, offsets))


def test_hours_refusals():
    lib = epr.load()
    t, perm, offsets, out, flag = np.zeros(4, dtype=np.int64), np.arange(4, dtype=np.uint32), np.array([0, 4]), np.zeros(4), np.zeros(1, dtype=np.uint32)
    call = lambda ttype, tps, stride, tptr=t.ctypes.data: lib.tsfa_emul_pack_hours(   # noqa: E731
        tptr, ttype, tps, stride, perm.ctypes.data, offsets.ctypes.data, 4, 1, out.ctypes.data, flag.ctypes.data, 0)
    i64 = _native.TSFA_I64
    assert call(i64, 10 ** 9, 1) == 0 and call(_native.TSFA_F64, 0, 1) == 0
    assert call(i64, 7, 1) < 0 and call(i64, 10 ** 9, -1) < 0 and call(_native.TSFA_F32, 1, 1) < 0 and call(i64, 1, 1, None) < 0


def test_the_drivers_build_as_a_program_of_their_own(tmp_path):
    """The same file with its own main (no Python around it): the build a sanitizer run uses."""
    exe = str(tmp_path / "emul_pack_rows")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-DTSFA_EMUL", "-DTSFA_EMUL_MAIN", epr.SRC, "-o", exe])
    out = subprocess.check_output([exe]).decode()
    assert "0 failures" in out and os.path.exists(exe)
