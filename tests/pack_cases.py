"""Test helper: the frames the device packer is checked on, and the exact comparison with data._pack's host route.

Shared by tests/test_pack_device_emul.py (the g++ emulation of the kernel bodies, no GPU) and tests/test_pack_device.py (the
kernels on the GPU): same cases, same reference, same equality.  A packer moves and converts, it does not compute, so
equality is exact: np.array_equal on ids, offsets, values and the packed sort column, dtypes included.
"""
import numpy as np

from tsfresh_amd.feature_extraction import data

TILE = 4096   # rows per tile of the sort kernels (csrc/pack_device.h: PK_TILE); the emulation test asserts it
SIZES = (1000, TILE - 1, TILE, TILE + 1, (1 << 20) + 77)


def _ragged(n, rng, mean_len=37):
    """ids (ascending, int64, ragged groups) and the position of every row inside its group, n rows in all."""
    n_ids = max(1, n // mean_len)
    cuts = np.sort(rng.choice(np.arange(1, n), size=min(n_ids - 1, n - 1), replace=False)) if n > 1 and n_ids > 1 else []
    starts = np.concatenate([[0], cuts]).astype(np.int64)
    lengths = np.diff(np.concatenate([starts, [n]]))
    ids = np.repeat(np.arange(len(starts), dtype=np.int64), lengths)
    pos = np.arange(n, dtype=np.int64) - np.repeat(starts, lengths)
    return ids, pos


def _layout(name, ids, pos, rng):
    n = len(ids)
    if name == "in_order":
        return np.arange(n)
    if name == "reverse":
        return np.arange(n)[::-1].copy()
    if name == "time_major":   # one row per (timestamp, id), ordered by time, ids interleaved: the sensor log
        return np.lexsort((ids, pos))
    return rng.permutation(n)


def _base(n, rng, layout="random"):
    ids, pos = _ragged(n, rng)
    order = _layout(layout, ids, pos, rng)
    return ids[order], pos[order], rng.standard_normal(n).astype(np.float32)


def _c_layout(layout):
    def make(n, rng):
        return _base(n, rng, layout)
    return make


def _c_duplicates(n, rng):
    # many equal (id, sort) pairs: the values must come out in original row order (stability)
    return rng.integers(0, 5, n), rng.integers(0, 3, n), np.arange(n, dtype=np.float64)


def _c_ids(transform):
    def make(n, rng):
        ids, sort, values = _base(n, rng)
        return transform(ids, rng), sort, values
    return make


def _c_sort(transform):
    def make(n, rng):
        ids, sort, values = _base(n, rng)
        return ids, transform(sort, rng), values
    return make


def _c_values(make_values):
    def make(n, rng):
        ids, sort, _ = _base(n, rng)
        return ids, sort, make_values(n, rng)
    return make


def _float_sort_with_zeros(sort, rng):
    s = (sort - 3).astype(np.float64) * 0.5      # negative values
    z = rng.random(len(s)) < 0.3                  # both zeros, many times in every group
    s[z] = np.where(rng.random(int(z.sum())) < 0.5, -0.0, 0.0)
    return s


def _around_2_53(n, rng):
    base = np.array([2 ** 53 + 1, -(2 ** 53 + 1), 2 ** 53 + 2, 2 ** 53 + 3, -(2 ** 53) - 3, 2 ** 53 - 1, 2 ** 62 + 1,
                     -(2 ** 63), 2 ** 63 - 1, 0, -1], dtype=np.int64)
    return base[rng.integers(0, len(base), n)] + rng.integers(-2, 3, n) * (rng.random(n) < 0.5)


def _big_u64(n, rng):
    return (np.uint64(2 ** 63) + rng.integers(0, 2 ** 62, n).astype(np.uint64) * np.uint64(2)
            + rng.integers(0, 2, n).astype(np.uint64))


CASES = {
    "time_major": _c_layout("time_major"),
    "random": _c_layout("random"),
    "in_order": _c_layout("in_order"),
    "reverse": _c_layout("reverse"),
    "duplicates": _c_duplicates,
    "ids_negative_int64": _c_ids(lambda ids, rng: (ids - len(ids) // 80) * np.int64(2 ** 45 + 12345)),
    "ids_int32": _c_ids(lambda ids, rng: (ids * 7 - 1000).astype(np.int32)),
    "ids_uint64_above_2_63": _c_ids(lambda ids, rng: np.uint64(2 ** 63 + 5) + ids.astype(np.uint64) * np.uint64(3)),
    "ids_single": _c_ids(lambda ids, rng: np.full(len(ids), 42, dtype=np.int64)),
    "ids_every_id_once": _c_ids(lambda ids, rng: rng.permutation(len(ids)).astype(np.int64)),
    "ids_strings": _c_ids(lambda ids, rng: np.array(["s%05d" % (v % 997) for v in ids], dtype=object)),
    "sort_int64_wide": _c_sort(lambda s, rng: s * np.int64(2 ** 33 + 1) - np.int64(2 ** 41)),
    "sort_float64_zeros": _c_sort(_float_sort_with_zeros),
    "sort_float32": _c_sort(lambda s, rng: ((s % 50) - 20).astype(np.float32) * np.float32(0.25)),
    "sort_datetime64": _c_sort(lambda s, rng: np.datetime64("2020-01-01", "ns") + s.astype("timedelta64[s]")),
    "sort_none": lambda n, rng: (lambda t: (t[0], None, t[2]))(_base(n, rng)),
    "values_float64": _c_values(lambda n, rng: rng.standard_normal(n)),
    "values_bool": _c_values(lambda n, rng: rng.random(n) < 0.5),
    "values_int8": _c_values(lambda n, rng: rng.integers(-128, 128, n).astype(np.int8)),
    "values_int16": _c_values(lambda n, rng: rng.integers(-32768, 32768, n).astype(np.int16)),
    "values_uint16": _c_values(lambda n, rng: rng.integers(0, 65536, n).astype(np.uint16)),
    "values_int32": _c_values(lambda n, rng: rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32)),
    "values_int64_around_2_53": _c_values(_around_2_53),
    "values_uint64_above_2_63": _c_values(_big_u64),
}


def make_case(name, n, seed=0):
    rng = np.random.default_rng([seed, n, sorted(CASES).index(name)])
    ids, sort, values = CASES[name](n, rng)
    return np.asarray(ids), None if sort is None else np.asarray(sort), np.asarray(values)


def host_pack(ids, sort, values, monkeypatch):
    """data._pack's host route with the presorted shortcut disabled: factorize + lexsort + gather, always."""
    monkeypatch.setattr(data, "_pack_presorted", lambda *a, **k: None)
    return data._pack("v", ids, values, sort, pack="host")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view("u%d" % a.dtype.itemsize) if a.dtype.kind in "fmM" else a


def assert_equals_host(pack_class, ids, sort, values, monkeypatch):
    """Pack the columns with `pack_class` (the DevicePack interface) and compare with the host route, exactly.
    -> the pack object (closed)."""
    want = host_pack(ids, sort, values, monkeypatch)
    reason, columns = data._device_pack_columns(ids, values, sort)
    assert reason is None, reason
    id_col, labels, sort_col, val_col = columns
    pack = pack_class(id_col, sort_col, val_col, device=0, keep_sort=True)
    try:
        got_ids = pack.ids if labels is None else labels[pack.ids]
        want_ids = np.asarray(want.ids)
        assert got_ids.dtype == want_ids.dtype and np.array_equal(got_ids, want_ids)
        assert pack.n_series == want.n_series
        assert pack.offsets.dtype == np.int64 and np.array_equal(pack.offsets, want.offsets)
        got_values = pack.values_host()
        assert got_values.dtype == want.values.dtype, (got_values.dtype, want.values.dtype)
        assert np.array_equal(_bits(got_values), _bits(want.values))
        if sort is None:
            assert pack.sort is None
        else:
            got_sort = pack.sort
            assert got_sort.dtype.itemsize == want.sort.dtype.itemsize
            assert np.array_equal(_bits(got_sort), _bits(want.sort).view(_bits(got_sort).dtype))
    finally:
        pack.close()
    return pack


def expected_passes(ids, sort):
    """Radix passes the skipping rule leaves for integer columns: the bytes of (key - min) that are not constant."""
    n = 0
    for col in (ids, sort):
        if col is None:
            continue
        col = np.asarray(col)
        wide = np.uint64 if col.dtype.kind == "u" else np.int64
        k = (col.astype(wide) - col.astype(wide).min()).astype(np.uint64)
        for b in range(8):
            digit = (k >> np.uint64(8 * b)) & np.uint64(255)
            n += int(digit.min() != digit.max())
    return n
