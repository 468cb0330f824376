"""The row packer's two kernels on the device (`tsfa_pack_set_rows`, `tsfa_pack_set_hours`, through
`_native.DevicePackSet(space=TSFA_DEVICE)`) against their g++ emulation (tests/test_pack_rows_emul.py pins that to numpy and
pandas), exactly: every value type, column count, row count and layout of the emulation's grid, the NaN flag per column, the
hours in every unit through the device's own conversion and divisions, missing stamps -- and one case per kernel with more
work items than its launch covers without striding (the counts come from the launch geometry)."""
import numpy as np
import pytest
import torch

import emul_pack_rows_lib as epr
from test_pack_rows_emul import ALL_TYPES, COLS, MAX_TILE_C, UNITS, frame_keys, layouts, make_values, row_counts
from tsfresh_amd import _native

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_SIGNED = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}


def _to_gpu(a):
    """A numpy view's twin on the device, with the same strides: the stretch of memory the view spans (gaps included) goes
    over as it lies and the view is taken there.  Unsigned types travel as their bit patterns."""
    strides = [s // a.itemsize for s in a.strides]
    span = sum((n - 1) * s for n, s in zip(a.shape, strides)) + 1
    flat = np.lib.stride_tricks.as_strided(a, (span,), (a.itemsize,)).copy()
    if flat.dtype.kind == "u":
        flat = flat.view(_SIGNED[flat.itemsize])
    return torch.as_strided(torch.from_numpy(flat).to(DEV), a.shape, strides)


def _key(t, dtype=np.int64):
    return t.data_ptr(), _native._DEVICE_PACK_TYPES[np.dtype(dtype)], dtype


def _set(ids, sort=None, kinds=None):
    cols = [None if c is None else torch.from_numpy(np.ascontiguousarray(c, dtype=np.int64)).to(DEV) for c in (ids, sort, kinds)]
    torch.cuda.synchronize()
    pack_set = _native.DevicePackSet(_key(cols[0]), None if sort is None else _key(cols[1]), None if kinds is None else _key(cols[2]),
                                     device=0, space=_native.TSFA_DEVICE, n_rows=len(ids))
    pack_set._columns = cols   # (the set read them in place while it was made)
    return pack_set


def _device_rows(pack_set, view):
    """-> ([C, N] gathered columns, [C] NaN flags) of tsfa_pack_set_rows for the numpy view's twin on the device."""
    v = view if view.ndim == 2 else view[:, None]
    t = _to_gpu(v)
    assert list(t.stride()) == [s // v.itemsize for s in v.strides]
    torch.cuda.synchronize()
    packs = pack_set.rows(t.data_ptr(), _native._DEVICE_PACK_TYPES[v.dtype], v.shape[1], t.stride(0), t.stride(1))
    try:
        assert all(p.ids is None and p.n_rows == v.shape[0] for p in packs)
        return np.stack([p.values_host() for p in packs]), np.array([p.value_nan for p in packs])
    finally:
        for p in packs:
            p.close()


def _same_bits(a, b):
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(u), np.ascontiguousarray(b).view(u))


@pytest.mark.parametrize("dtype", ALL_TYPES, ids=lambda d: np.dtype(d).name)
def test_rows_equal_the_emulation_on_its_grid(gpu, dtype):
    rng = np.random.default_rng(11)
    for c in COLS:
        for n in row_counts(c):
            ids = rng.integers(0, max(2, n // 3), size=n)
            perm, _ = epr.sort_order(ids)
            with _set(ids) as pack_set:
                for name, view in layouts(rng, n, c, dtype):
                    want = epr.EmulRows(view, perm)
                    got, nan = _device_rows(pack_set, view)
                    assert _same_bits(got, want.columns), (name, n, c)
                    assert not nan.any() and not want.nan.any()


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_rows_nan_flag_per_column_and_identity(gpu, dtype):
    rng = np.random.default_rng(3)
    for c, bad_cols in ((1, (0,)), (3, (1,)), (MAX_TILE_C + 1, (0, MAX_TILE_C)), (2 * MAX_TILE_C + 1, (MAX_TILE_C - 1, 2 * MAX_TILE_C))):
        n = row_counts(c)[-1]
        x = make_values(rng, (n, c), dtype)
        for col in bad_cols:
            x[rng.integers(0, n), col] = np.nan
        ids = np.sort(rng.integers(0, 50, size=n))   # in order: the set keeps the identity
        with _set(ids) as pack_set:
            assert pack_set.was_in_order and pack_set.n_passes == 0
            for view in (x, np.asfortranarray(x)):
                got, nan = _device_rows(pack_set, view)
                assert sorted(np.nonzero(nan)[0]) == sorted(bad_cols)
                assert np.array_equal(np.isnan(got), np.isnan(x.T)) and np.array_equal(got[~np.isnan(got)], x.T[~np.isnan(x.T)])


def test_rows_more_work_items_than_one_launch_covers(gpu):
    """Both routes stride: the tiles route over position tiles, the gather over cells."""
    rng = np.random.default_rng(7)
    c = MAX_TILE_C
    geo = epr.geometry(c)
    n = (geo["rows_max_grid"] + 3) * geo["tile_t"] + 5
    assert n * c > geo["rows_max_grid"] * 256   # the gather's launch: rows_max_grid workgroups of 256 lanes, one cell each
    x = rng.standard_normal((n, c)).astype(np.float32)
    ids = rng.integers(0, 1000, size=n)
    perm, _ = epr.sort_order(ids)
    want = np.ascontiguousarray(x[perm].T)
    assert _same_bits(epr.EmulRows(x, perm).columns, want)
    with _set(ids) as pack_set:
        for view in (x, np.asfortranarray(x)):
            got, nan = _device_rows(pack_set, view)
            assert _same_bits(got, want) and not nan.any()


def _device_hours(pack_set, t, tps):
    n = pack_set.n_rows
    tt = _to_gpu(t)
    hours = torch.full((n + 16,), -7.25, dtype=torch.float64, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    pack_set.hours(tt.data_ptr(), _native.TSFA_I64 if t.dtype == np.int64 else _native.TSFA_F64, tps, tt.stride(0), hours.data_ptr(),
                   flag.data_ptr())
    out = hours.cpu().numpy()
    assert np.all(out[n:] == -7.25)
    return out[:n], int(flag.item())


def _assert_hours(got, want):
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok].view(np.uint64), want[ok].view(np.uint64))


def test_hours_equal_the_emulation_in_every_unit(gpu):
    rng = np.random.default_rng(23)
    ids, kinds, sort = frame_keys(rng)
    perm, offsets = epr.sort_order(ids, sort, kinds)
    n = len(ids)
    nat = np.iinfo(np.int64).min
    with _set(ids, sort, kinds) as pack_set:
        assert pack_set.n_kinds == 2 and not pack_set.was_in_order
        for unit, tps in sorted(UNITS.items()):
            ticks = rng.integers(-3 * 10 ** 9, 3 * 10 ** 9, size=n) * tps + rng.integers(0, tps, size=n)
            want = epr.EmulHours(ticks, tps, perm, offsets)
            got, flag = _device_hours(pack_set, ticks, tps)
            _assert_hours(got, want.hours)
            assert flag == 0 == want.flags
            wide = np.zeros(2 * n, dtype=np.int64)
            wide[::2] = ticks
            got, flag = _device_hours(pack_set, wide[::2], tps)
            _assert_hours(got, want.hours)
        seconds = rng.standard_normal(n) * 1e6
        got, flag = _device_hours(pack_set, seconds, 1)
        _assert_hours(got, epr.EmulHours(seconds, 1, perm, offsets).hours)
        # NaT as the first stamp of the group that spans three tiles, and inside another group
        big = int(np.argmax(np.diff(offsets)))
        ticks = rng.integers(0, 10 ** 15, size=n)
        ticks[[perm[offsets[big]], perm[offsets[2] + 3]]] = nat
        want = epr.EmulHours(ticks, 10 ** 9, perm, offsets)
        got, flag = _device_hours(pack_set, ticks, 10 ** 9)
        _assert_hours(got, want.hours)
        assert flag == want.flags == _native.TSFA_DENSE_BAD_TIME and np.isnan(got).sum() == offsets[big + 1] - offsets[big] + 1
        seconds = ticks.astype(np.float64)
        seconds[ticks == nat] = np.nan
        got, flag = _device_hours(pack_set, seconds, 1)
        assert flag == _native.TSFA_DENSE_BAD_TIME and np.array_equal(np.isnan(got), np.isnan(want.hours))


def test_hours_more_tiles_than_one_launch_covers(gpu):
    rng = np.random.default_rng(29)
    geo = epr.geometry()
    n = (geo["hours_max_grid"] + 2) * geo["hours_tile"] + 5
    lengths = rng.integers(1, 3000, size=n // 1000)
    ids = np.repeat(np.arange(len(lengths)), lengths)[:n]
    ids = np.concatenate([ids, np.full(n - len(ids), len(lengths))])   # in order: the identity permutation
    perm, offsets = epr.sort_order(ids)
    ticks = rng.integers(0, 10 ** 18, size=n)
    want = epr.EmulHours(ticks, 10 ** 9, perm, offsets)
    with _set(ids) as pack_set:
        assert pack_set.was_in_order
        got, flag = _device_hours(pack_set, ticks, 10 ** 9)
    _assert_hours(got, want.hours)
    assert flag == 0
