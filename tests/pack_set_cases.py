"""Test helper: the frames the pack set (tsfa_pack_set_*, `_native.DevicePackSet`) is checked on, and the exact comparison with
data._pack's host route, kind by kind.

Shared by tests/test_pack_set_emul.py (the g++ emulation of the kernel bodies, no GPU) and tests/test_pack_set_gpu.py (the
kernels on the GPU): same cases, same reference, same equality.  The yardstick is what `pack_timeseries` did before the set
existed: select the rows of one kind on the host, `data._pack(..., pack="host")` them.  A packer moves and converts, so
equality is exact: np.array_equal on ids, offsets, values and the packed sort column, dtypes included.
"""
import numpy as np

import pack_cases
from tsfresh_amd import _native
from tsfresh_amd.feature_extraction import data

TILE = pack_cases.TILE
SIZES = (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)


def _in_id_sort_order(n, rng):
    ids, pos = pack_cases._ragged(n, rng)
    return ids * 3 - 50, pos


def _c_edge_ids(n, rng):
    # kind 0 ends with id 9 and kind 1 starts with it, kind 1 ends with id 12 and kind 2 starts with it: those rows must
    # head new series.  Id 3 is in kind 0 only.  Kind 2 is ONE row (when there are at least 3 rows).  Many rows share their
    # (kind, id, sort): the values (0, 1, 2, ...) must keep their input order.
    kinds = rng.integers(0, 2, n).astype(np.int32)
    ids = np.where(kinds == 0, rng.choice([3, 5, 9], n), rng.choice([9, 12], n)).astype(np.int64)
    if n >= 3:
        kinds[n // 2], ids[n // 2] = 2, 12
    return ids, rng.integers(0, 4, n), kinds, np.arange(n, dtype=np.float64)


def _c_interleaved(n, rng):
    # the usual long frame: rows in (id, time) order, the kinds interleave
    ids, pos = _in_id_sort_order(n, rng)
    return ids, pos, rng.integers(0, 3, n).astype(np.int16), rng.standard_normal(n).astype(np.float32)


def _c_kind_major(n, rng):
    ids, pos, kinds, values = _c_interleaved(n, rng)
    order = np.lexsort((pos, ids, kinds))
    return ids[order], pos[order], kinds[order], values


def _c_random(n, rng):
    ids, pos, _, values = _c_interleaved(n, rng)
    order = rng.permutation(n)
    return ids[order], pos[order], rng.integers(0, 5, n).astype(np.uint8), values


def _c_no_sort(n, rng):
    ids, _, kinds, _ = _c_random(n, rng)
    return ids, None, kinds, np.arange(n, dtype=np.float64)


def _c_kinds_int8_negative(n, rng):
    ids, pos, _, values = _c_random(n, rng)
    return ids, pos, np.array([-100, -3, 0, 7, 100], dtype=np.int8)[rng.integers(0, 5, n)], values


def _c_kinds_int64(n, rng):
    ids, pos, _, values = _c_random(n, rng)
    return ids, pos, np.array([-2 ** 40, 5, 2 ** 50], dtype=np.int64)[rng.integers(0, 3, n)], values


CASES = {
    "edge_ids": _c_edge_ids,
    "interleaved": _c_interleaved,
    "kind_major": _c_kind_major,
    "random": _c_random,
    "no_sort": _c_no_sort,
    "kinds_int8_negative": _c_kinds_int8_negative,
    "kinds_int64": _c_kinds_int64,
}


def make_case(name, n, seed=0):
    rng = np.random.default_rng([seed, n, sorted(CASES).index(name)])
    ids, sort, kinds, values = CASES[name](n, rng)
    return np.asarray(ids), None if sort is None else np.asarray(sort), np.asarray(kinds), np.asarray(values)


# where kind 1 starts along the sorted order of a frame of 2 * TILE + 1 rows: inside a tile, on the last row of a tile
# (kind 0 ends one row before the tile's edge), on the first row of a tile (kind 0 ends exactly on the edge)
BOUNDARIES = {"inside_a_tile": 1000, "last_row_of_a_tile": TILE - 1, "first_row_of_a_tile": TILE}


def make_boundary_case(first_kind_rows, seed=0):
    n = 2 * TILE + 1
    rng = np.random.default_rng([seed, first_kind_rows])
    ids, pos = _in_id_sort_order(n, rng)
    kinds = np.ones(n, dtype=np.int32)
    kinds[rng.choice(n, first_kind_rows, replace=False)] = 0
    order = rng.permutation(n)
    return ids[order], pos[order], kinds[order], rng.standard_normal(n).astype(np.float32)


def dense_kinds_in_id_sort_order(n_kinds, n=3 * TILE + 17, seed=0):
    """Rows in (id, sort) order, kinds 0 .. n_kinds - 1 (every one present) interleaved."""
    rng = np.random.default_rng([seed, n_kinds])
    ids, pos = _in_id_sort_order(n, rng)
    kinds = rng.integers(0, n_kinds, n)
    kinds[rng.choice(n, n_kinds, replace=False)] = np.arange(n_kinds)
    return ids, pos, kinds.astype(np.uint8 if n_kinds <= 256 else np.uint16), rng.standard_normal(n).astype(np.float32)


def five_kinds_on_ragged_ids(n=3 * TILE + 17, seed=3):
    """5 kinds interleaved in time order on ragged ids: every 64-row round of the scatter holds several kinds."""
    rng = np.random.default_rng(seed)
    ids, pos = _in_id_sort_order(n, rng)
    kinds = rng.integers(0, 5, n).astype(np.int32)
    order = np.lexsort((kinds, ids, pos))
    return ids[order], pos[order], kinds[order], rng.standard_normal(n)


def wide_columns(n, seed=0):
    """(ids, sort, [value columns]): float32, int64 beyond 2^53 and bool over one shuffled frame."""
    rng = np.random.default_rng([seed, n])
    ids, pos = _in_id_sort_order(n, rng)
    order = rng.permutation(n)
    big = (np.int64(2 ** 53) + rng.integers(1, 2 ** 20, n)) * np.where(rng.random(n) < 0.5, -1, 1)
    return ids[order], pos[order], [rng.standard_normal(n).astype(np.float32), big.astype(np.int64), rng.random(n) < 0.5]


def assert_pack_equals(pack, want_ids, want_offsets, want_values, want_sort):
    """One DevicePack-like object against expected arrays, exactly."""
    got_ids = np.asarray(pack.ids)
    assert got_ids.dtype == want_ids.dtype and np.array_equal(got_ids, want_ids)
    assert pack.n_series == len(want_ids) and pack.n_rows == len(want_values)
    got_offsets = np.asarray(pack.offsets)
    assert got_offsets.dtype == np.int64 and np.array_equal(got_offsets, want_offsets)
    got_values = pack.values_host()
    assert got_values.dtype == want_values.dtype, (got_values.dtype, want_values.dtype)
    assert np.array_equal(pack_cases._bits(got_values), pack_cases._bits(want_values))
    if want_sort is None:
        assert pack.sort is None
    else:
        got_sort = pack_cases._bits(pack.sort)
        assert got_sort.dtype.itemsize == want_sort.dtype.itemsize
        assert np.array_equal(got_sort, pack_cases._bits(want_sort).view(got_sort.dtype))


def assert_set_equals_host(set_class, ids, sort, kinds, values, monkeypatch):
    """Sort the frame once with `set_class` (the DevicePackSet interface), gather `values`, and compare every kind's pack
    with the host route on that kind's rows.  The set is closed BEFORE its packs are read: they must not need it.
    -> (the set, the packs), all closed."""
    reason, columns = data._device_pack_columns(ids, values, sort)
    assert reason is None, reason
    id_col, labels, sort_col, val_col = columns
    assert labels is None
    kind_col = None if kinds is None else _native.pack_column(np.asarray(kinds))
    pack_set = set_class(id_col, sort_col, kind_col, device=0, keep_sort=True)
    try:
        packs = pack_set.values(val_col)
    finally:
        pack_set.close()
    try:
        kind_values = np.unique(kinds) if kinds is not None else [None]
        assert pack_set.n_kinds == len(kind_values) == len(packs)
        if kinds is not None:
            assert pack_set.kinds.dtype == np.asarray(kinds).dtype and np.array_equal(pack_set.kinds, kind_values)
        for kv, pack in zip(kind_values, packs):
            sel = slice(None) if kv is None else np.flatnonzero(kinds == kv)
            want = pack_cases.host_pack(ids[sel], None if sort is None else sort[sel], values[sel], monkeypatch)
            assert_pack_equals(pack, np.asarray(want.ids), want.offsets, want.values, want.sort)
            assert pack.n_passes == pack_set.n_passes and pack.was_in_order == pack_set.was_in_order
    finally:
        for pack in packs:
            pack.close()
    return pack_set, packs


def assert_set_equals_single_packer(set_class, pack_class, ids, sort, kinds, value_columns):
    """Every value column through ONE set (kinds: None or a constant column) against its own `pack_class` (the DevicePack
    interface) result, byte for byte; the set ran the passes the single packer ran."""
    reason, keys = data._device_key_columns(ids, sort)
    assert reason is None, reason
    id_col, _, sort_col = keys
    kind_col = None if kinds is None else _native.pack_column(np.asarray(kinds))
    with set_class(id_col, sort_col, kind_col, device=0, keep_sort=True) as pack_set:
        assert pack_set.n_kinds == 1
        for values in value_columns:
            val_col = _native.pack_column(np.asarray(values))
            single = pack_class(id_col, sort_col, val_col, device=0, keep_sort=True)
            (pack,) = pack_set.values(val_col)
            try:
                assert_pack_equals(pack, single.ids, single.offsets, single.values_host(), single.sort)
                assert pack_set.n_passes == single.n_passes and pack_set.was_in_order == single.was_in_order
            finally:
                pack.close()
                single.close()
