"""`extract_features_long_tensor` above the kernels: the checks and their exceptions, the native call sequence of the wide, long
and timed forms, names, column order and `ids_out` -- on CPU tensors, with numpy and the g++ build of the row packer's bodies
standing in for the device and a numpy plan standing in for the kernels (the manner of test_tensor_entry_routes.py).
No GPU needed."""
import ctypes
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch

import emul_pack_rows_lib as epr
import tsfresh_amd
from tsfresh_amd import MinimalFCParameters, _native, extract_features, tensor_long
from tsfresh_amd.feature_extraction import extraction
from tsfresh_amd.feature_extraction.registry import UnsupportedFeature

CALLS = []   # the native calls of one entry call, in order

_NP = {code: np.dtype(dt) for dt, code in _native._DEVICE_PACK_TYPES.items()}


def _host(ptr, n, dtype, stride=1):
    """n elements of `dtype` (element stride `stride`) at a HOST pointer: what a CPU tensor's data_ptr() is."""
    dtype = np.dtype(dtype)
    span = (n - 1) * stride + 1
    raw = (ctypes.c_char * (span * dtype.itemsize)).from_address(ptr)
    return np.frombuffer(raw, dtype=dtype)[::stride][:n] if stride else np.repeat(np.frombuffer(raw, dtype=dtype)[:1], n)


class _NumpyPlan:
    """Column j of a series is (j + 1) * its sum + its length (+ the sum of its hours with stamps), however it arrives."""

    def __init__(self, n_cols):
        self.n_cols = n_cols

    def _rows(self, values, offsets, hours=None):
        values = np.asarray(values, dtype=np.float64)
        base = np.array([[values[a:b].sum(), b - a] for a, b in zip(offsets[:-1], offsets[1:])], dtype=np.float64).reshape(-1, 2)
        if hours is not None:
            base[:, 0] += np.array([hours[a:b].sum() for a, b in zip(offsets[:-1], offsets[1:])])
        return np.stack([(j + 1) * base[:, 0] + base[:, 1] for j in range(self.n_cols)], axis=1)

    def extract_host(self, values, offsets, times=None, out=None):
        return self._rows(values, offsets, times)

    def extract_into(self, values, offsets, matrix, col0=0, times=None, pack=None, times_ptr=None):
        assert values is None and offsets is None and isinstance(matrix, _native.BorrowedMatrix)
        assert matrix.ptr == matrix.owner.data_ptr() and matrix.ld == matrix.owner.shape[1] and matrix.shape[0] == pack.n_series
        CALLS.append(("extract_into", pack.name, col0, times_ptr is not None))
        hours = None if times_ptr is None else _host(times_ptr, pack.n_rows, np.float64)
        matrix.owner.numpy()[:, col0:col0 + self.n_cols] = self._rows(pack.values_host(), pack.offsets, hours)


class _EmulPack:
    def __init__(self, name, values, offsets, ids, nan, device):
        self.name, self._values, self.offsets, self.ids_np, self.value_nan, self.device = name, values, offsets, ids, nan, device
        self.n_rows, self.n_series, self.ids_dtype = len(values), len(ids), ids.dtype

    def values_host(self):
        return self._values

    def close(self):
        CALLS.append(("pack.close", self.name))


class _EmulSet:
    """Stands in for `_native.DevicePackSet(space=TSFA_DEVICE)`: the same raw pointers in (host pointers here), numpy's
    stable sorts for the radix sort, the g++ build of pack_rows.h for the two new kernels."""

    def __init__(self, ids, sort, kinds, device=0, keep_sort=False, space=_native.TSFA_HOST, n_rows=None):
        assert space == _native.TSFA_DEVICE and not keep_sort
        CALLS.append(("set.create", sort is not None, kinds is not None, n_rows))
        col = lambda c: None if c is None else _host(c[0], n_rows, c[2])   # noqa: E731
        assert all(c is None or _NP[c[1]] == np.dtype(c[2]) for c in (ids, sort, kinds))
        self._ids, self._kinds = col(ids), col(kinds)
        self.perm, self.offsets = epr.sort_order(self._ids, col(sort), self._kinds)
        self.n_rows, self.device = n_rows, device
        self.kinds = None if kinds is None else np.unique(self._kinds)
        self.n_kinds = 1 if kinds is None else len(self.kinds)
        self.flags = _native.TSFA_PACK_IN_ORDER if np.array_equal(self.perm, np.arange(n_rows)) else 0

    def _kind_ranges(self):
        if self.kinds is None:
            return [(0, self.n_rows)]
        sk = self._kinds[self.perm]
        return [(int(np.searchsorted(sk, k, "left")), int(np.searchsorted(sk, k, "right"))) for k in self.kinds]

    def _pack(self, name, column, r0, r1, nan):
        inside = (self.offsets >= r0) & (self.offsets <= r1)
        offsets = self.offsets[inside] - r0
        ids = self._ids[self.perm][self.offsets[inside][:-1]]
        return _EmulPack(name, column[r0:r1], offsets, ids, nan, self.device)

    def rows(self, values_ptr, value_type, n_cols, stride_row, stride_col):
        CALLS.append(("set.rows", n_cols, stride_row, stride_col))
        dt = _NP[value_type]
        span = (self.n_rows - 1) * stride_row + (n_cols - 1) * stride_col + 1
        flat = _host(values_ptr, span, dt)
        view = np.lib.stride_tricks.as_strided(flat, (self.n_rows, n_cols), (stride_row * dt.itemsize, stride_col * dt.itemsize))
        res = epr.EmulRows(view, self.perm)
        assert res.status >= 0 and res.guards_intact
        return [self._pack(c, res.columns[c], 0, self.n_rows, bool(res.nan[c])) for c in range(n_cols)]

    def values(self, column):
        CALLS.append(("set.values",))
        ptr, vtype = column
        v = _host(ptr, self.n_rows, _NP[vtype])
        res = epr.EmulRows(v, self.perm)
        nan = bool(res.nan[0])
        return [self._pack(int(k), res.columns[0], r0, r1, nan) for k, (r0, r1) in zip(self.kinds, self._kind_ranges())]

    def hours(self, t_ptr, t_type, ticks_per_second, stride, hours_ptr, flags_ptr):
        CALLS.append(("set.hours", ticks_per_second, stride))
        t = _host(t_ptr, self.n_rows, np.int64 if t_type == _native.TSFA_I64 else np.float64, stride)
        res = epr.EmulHours(t, ticks_per_second, self.perm, self.offsets)
        assert res.status == 0 and res.guards_intact
        np.ctypeslib.as_array((ctypes.c_double * self.n_rows).from_address(hours_ptr))[:] = res.hours
        np.ctypeslib.as_array((ctypes.c_int32 * 1).from_address(flags_ptr))[0] |= res.flags

    def close(self):
        CALLS.append(("set.close",))


@pytest.fixture
def emulated(monkeypatch):
    del CALLS[:]
    monkeypatch.setattr(extraction, "_acquire_plan", lambda fplan, device, pins=None: _NumpyPlan(len(fplan.names)))
    monkeypatch.setattr(tensor_long._native, "DevicePackSet", _EmulSet)
    monkeypatch.setattr(tensor_long, "_to_device", lambda t, device: t)
    monkeypatch.setattr(tensor_long, "_synchronize", lambda torch_, device: None)
    monkeypatch.setattr(tensor_long, "_ids_tensor", lambda torch_, pack, dtype, device: torch.from_numpy(pack.ids_np.copy()))


@pytest.fixture
def no_native(monkeypatch):
    """Any native call -- a plan, a pack set -- is a test failure: the refusals come first."""
    def forbidden(*a, **k):
        raise AssertionError("a native call was made before the refusal")
    monkeypatch.setattr(extraction, "_acquire_plan", forbidden)
    monkeypatch.setattr(tensor_long._native, "DevicePackSet", forbidden)
    monkeypatch.setattr(tensor_long, "_to_device", forbidden)
    monkeypatch.setattr(_native, "load", forbidden)


def _frame(seed=0, n_ids=7, C=3, dtype=np.float64):
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 9, size=n_ids)
    ids = np.repeat(np.arange(n_ids) * 3 - 4, lens)
    sort = np.concatenate([np.arange(L) for L in lens])
    x = rng.standard_normal((len(ids), C)).astype(dtype)
    shuffle = rng.permutation(len(ids))
    return ids[shuffle], sort[shuffle], x[shuffle]


def test_reexported_and_torch_stays_out_of_the_package_import():
    assert tsfresh_amd.extract_features_long_tensor is tensor_long.extract_features_long_tensor
    code = "import sys, tsfresh_amd, tsfresh_amd.tensor_long; assert 'torch' not in sys.modules, 'torch was imported'"
    subprocess.check_call([sys.executable, "-c", code])


def test_wide_form_names_order_values_and_calls(emulated):
    ids, sort, x = _frame()
    names = ["b", "a", "c"]
    params = MinimalFCParameters()
    df = pd.DataFrame(dict({"id": ids, "t": sort}, **{k: x[:, c] for c, k in enumerate(names)}))
    want = extract_features(df, column_id="id", column_sort="t", default_fc_parameters=params, pack="host")
    feats, cols, ids_out = tsfresh_amd.extract_features_long_tensor(torch.from_numpy(ids), torch.from_numpy(x), sort=sort,
                                                                   kind_names=names, default_fc_parameters=params)
    assert cols == list(want.columns) and np.array_equal(ids_out.numpy(), want.index.to_numpy()) and ids_out.dtype == torch.int64
    assert feats.dtype == torch.float64 and np.array_equal(feats.numpy(), want.to_numpy())
    w = len(params)
    assert CALLS == [("set.create", True, False, len(ids)), ("set.rows", 3, 3, 1),
                     ("extract_into", 0, 0, False), ("extract_into", 1, w, False), ("extract_into", 2, 2 * w, False),
                     ("pack.close", 0), ("pack.close", 1), ("pack.close", 2), ("set.close",)]
    # one column, a column-major view and no sort column: the strides reach the packer as they are
    del CALLS[:]
    xt = torch.from_numpy(np.asfortranarray(x))
    a, cols1, _ = tsfresh_amd.extract_features_long_tensor(ids, xt[:, 1], default_fc_parameters=params)
    assert cols1 == ["0__" + c.split("__")[1] for c in cols[:w]] and CALLS[0] == ("set.create", False, False, len(ids))
    assert CALLS[1][:3] == ("set.rows", 1, 1)
    del CALLS[:]
    b, _, _ = tsfresh_amd.extract_features_long_tensor(ids, xt, default_fc_parameters=params)
    assert CALLS[1] == ("set.rows", 3, 1, len(ids)) and torch.equal(b[:, w:2 * w], a)


def test_long_form_unequal_id_sets_and_names_out_of_code_order(emulated):
    rng = np.random.default_rng(4)
    names = {5: "zeta", 9: "alpha", 7: "mid"}
    id_sets = {5: [1, 2, 3, 8], 9: [2, 3, 4], 7: [-6, 8]}
    rows = [(i, k, t, rng.standard_normal()) for k, idl in id_sets.items() for i in idl for t in range(rng.integers(1, 6))]
    rows = [rows[j] for j in rng.permutation(len(rows))]
    ids, kinds, sort, vals = (np.array(c) for c in zip(*rows))
    params = MinimalFCParameters()
    df = pd.DataFrame({"id": ids, "kind": [names[k] for k in kinds], "t": sort, "v": vals})
    want = extract_features(df, column_id="id", column_sort="t", column_kind="kind", column_value="v", default_fc_parameters=params,
                            pack="host")
    for kind_names in (names, [None] * 5 + ["zeta", None, "mid", None, "alpha"]):
        del CALLS[:]
        feats, cols, ids_out = tsfresh_amd.extract_features_long_tensor(ids.astype(np.int32), vals, sort=sort, kinds=kinds.astype(np.int16),
                                                                       kind_names=kind_names, default_fc_parameters=params)
        assert cols == list(want.columns) and cols[0].startswith("alpha__") and cols[-1].startswith("zeta__")
        assert ids_out.dtype == torch.int32 and ids_out.tolist() == [-6, 1, 2, 3, 4, 8] == list(want.index)
        got, ref = feats.numpy(), want.to_numpy()
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(ref).any() and np.array_equal(got[~np.isnan(got)], ref[~np.isnan(ref)])
        # packs come in code order (5, 7, 9); the column blocks in name order (alpha = 9, mid = 7, zeta = 5)
        w = len(params)
        assert CALLS[:2] == [("set.create", True, True, len(ids)), ("set.values",)]
        assert CALLS[2:5] == [("extract_into", 9, 0, False), ("extract_into", 7, 0, False), ("extract_into", 5, 0, False)]
    # equal id sets: straight into the column blocks
    del CALLS[:]
    both = np.concatenate([ids, ids])
    k2 = np.concatenate([np.zeros(len(ids), dtype=np.int64), np.ones(len(ids), dtype=np.int64)])
    feats, cols, ids_out = tsfresh_amd.extract_features_long_tensor(both, np.concatenate([vals, -vals]), kinds=k2, default_fc_parameters=params)
    assert cols[0].startswith("0__") and [c[:3] for c in CALLS if c[0] == "extract_into"] == [("extract_into", 0, 0), ("extract_into", 1, w)]
    assert not torch.isnan(feats).any()
    with pytest.raises(ValueError, match="kind code 7 has no name"):
        tsfresh_amd.extract_features_long_tensor(ids, vals, kinds=kinds, kind_names={5: "a", 9: "b"}, default_fc_parameters=params)


@pytest.mark.parametrize("unit", ("ns", "s"))
def test_timed_form_serves_linear_trend_timewise(emulated, unit):
    ids, sort, x = _frame(seed=2, C=2)
    rng = np.random.default_rng(9)
    ticks = rng.integers(0, 10 ** 6, size=len(ids)) * (10 ** 9 if unit == "ns" else 1)
    params = dict(MinimalFCParameters(), linear_trend_timewise=[{"attr": "slope"}])
    want_hours = None
    for arg in (ticks, ticks.view("M8[%s]" % unit), torch.from_numpy(ticks)):
        del CALLS[:]
        feats, cols, _ = tsfresh_amd.extract_features_long_tensor(ids, x, sort=sort, times=arg, time_unit=unit, default_fc_parameters=params)
        assert 'linear_trend_timewise__attr_"slope"' in "".join(cols) and len(cols) == 2 * len(params)
        assert CALLS[:3] == [("set.create", True, False, len(ids)), ("set.rows", 2, 2, 1), ("set.hours", 10 ** 9 if unit == "ns" else 1, 1)]
        assert [c for c in CALLS if c[0] == "extract_into"] == [("extract_into", 0, 0, True), ("extract_into", 1, len(params), True)]
        want_hours = feats if want_hours is None else want_hours
        assert torch.equal(feats, want_hours)
    bad = ticks.copy()
    bad[3] = np.iinfo(np.int64).min
    with pytest.raises(ValueError, match="times must not contain NaT / NaN"):
        tsfresh_amd.extract_features_long_tensor(ids, x, sort=sort, times=bad, time_unit=unit, default_fc_parameters=params)
    feats, _, _ = tsfresh_amd.extract_features_long_tensor(ids, x, sort=sort, times=bad, time_unit=unit, default_fc_parameters=params,
                                                           check_nan=False)
    assert torch.isnan(feats).any()


def test_nan_errors_after_the_pack(emulated):
    ids, sort, x = _frame()
    params = MinimalFCParameters()
    xn = x.copy()
    xn[4, 1] = np.nan
    with pytest.raises(ValueError, match="Column must not contain NaN values: v$"):
        tsfresh_amd.extract_features_long_tensor(ids, xn, sort=sort, kind_names=["u", "v", "w"], default_fc_parameters=params)
    assert ("set.rows", 3, 3, 1) in CALLS and CALLS[-1] == ("set.close",) and not any(c[0] == "extract_into" for c in CALLS)
    feats, _, _ = tsfresh_amd.extract_features_long_tensor(ids, xn, sort=sort, default_fc_parameters=params, check_nan=False)
    assert torch.isnan(feats).any()
    kinds = np.arange(len(ids)) % 2 + 3
    with pytest.raises(ValueError, match="Column must not contain NaN values: odd$"):
        tsfresh_amd.extract_features_long_tensor(ids, xn[:, 1], sort=sort, kinds=kinds, kind_names={3: "odd", 4: "even"},
                                                 default_fc_parameters=params)
    fs = sort.astype(np.float64)
    fs[2] = np.nan
    with pytest.raises(ValueError, match="Column must not contain NaN values: sort$"):
        tsfresh_amd.extract_features_long_tensor(ids, x, sort=fs, default_fc_parameters=params)


@pytest.mark.parametrize("bad_ids", (np.zeros(4), np.zeros(4, dtype=np.float32), np.zeros(4, dtype=bool), torch.zeros(4, dtype=torch.float64),
                                     torch.zeros(4, dtype=torch.bool), np.array(["a", "b", "c", "d"])))
def test_float_bool_and_string_ids_are_refused(no_native, bad_ids):
    name = str(bad_ids.dtype).replace("torch.", "")
    with pytest.raises(TypeError, match="ids must be .*" + name.replace("<", ".")):
        tsfresh_amd.extract_features_long_tensor(bad_ids, np.zeros(4), default_fc_parameters=MinimalFCParameters())


def test_refusals_before_anything_moves(no_native):
    params = MinimalFCParameters()
    ids, x = np.arange(6), np.zeros((6, 2))
    call = tsfresh_amd.extract_features_long_tensor
    for kw, exc, match in (
            (dict(ids=ids[:5], values=x), ValueError, "one entry per row"),
            (dict(ids=ids, values=x, sort=np.arange(5)), ValueError, "sort must have one entry per row"),
            (dict(ids=ids, values=x[:, 0], kinds=np.zeros(7, dtype=np.int64)), ValueError, "kinds must have one entry per row"),
            (dict(ids=ids, values=x, times=np.arange(5)), ValueError, "times must have shape"),
            (dict(ids=ids[:0], values=x[:0]), ValueError, "at least one row"),
            (dict(ids=ids.reshape(2, 3), values=x), ValueError, "one-dimensional"),
            (dict(ids=ids, values=x, kinds=np.zeros(6, dtype=np.int64)), ValueError, "kinds goes with one value column"),
            (dict(ids=ids, values=np.zeros((6, 2, 2))), ValueError, r"shape \(N,\) or \(N, C\)"),
            (dict(ids=ids, values=x.astype(np.float16)), TypeError, "values must be .*float16"),
            (dict(ids=ids, values=x.astype(np.complex64)), TypeError, "values must be .*complex64"),
            (dict(ids=ids, values=torch.zeros((6, 2), dtype=torch.bfloat16)), TypeError, "values must be .*bfloat16"),
            (dict(ids=ids, values=x, sort=np.zeros(6, dtype=bool)), TypeError, "sort must be .*bool"),
            (dict(ids=ids, values=x, sort=np.zeros(6, dtype=np.float16)), TypeError, "sort must be .*float16"),
            (dict(ids=ids, values=x[:, 0], kinds=np.zeros(6)), TypeError, "kinds must be integer codes, not .*float64"),
            (dict(ids=ids, values=x, times=np.zeros(6, dtype=np.float32)), TypeError, "times must be .*float32"),
            (dict(ids=ids, values=x, times=np.zeros(6, dtype=np.int64), time_unit="h"), ValueError, "time_unit"),
            (dict(ids=ids, values=x, kind_names=["a"]), ValueError, "2 value columns"),
            (dict(ids=ids, values=x, kind_names=["a", "a"]), ValueError, "distinct"),
            (dict(ids=ids, values=x, kind_names=["a", "b__c"]), ValueError, "not allowed to contain '__'"),
            (dict(ids=[1, 2, 3], values=x[:3]), TypeError, "ids must be a torch.Tensor or a numpy array, not list")):
        with pytest.raises(exc, match=match):
            call(default_fc_parameters=params, **kw)

    def my_feature(x):
        return 0.0
    for kw in (dict(values=x), dict(values=x[:, 0], kinds=np.zeros(6, dtype=np.int64))):
        with pytest.raises(UnsupportedFeature, match="custom \\(callable\\) calculators are evaluated per series on the host"):
            call(ids, default_fc_parameters={"maximum": None, my_feature: None}, **kw)
        with pytest.raises(UnsupportedFeature, match="callable"):
            call(ids, default_fc_parameters=params, kind_to_fc_parameters={"0": {my_feature: None}}, **kw)


def test_more_rows_than_the_permutation_indexes(no_native, monkeypatch):
    monkeypatch.setattr(tensor_long, "_MAX_ROWS", 5)
    with pytest.raises(ValueError, match="4 294 967 295 rows"):
        tsfresh_amd.extract_features_long_tensor(np.arange(6), np.zeros(6), default_fc_parameters=MinimalFCParameters())


def test_union_of_unsigned_and_wide_ids():
    """The id sets' union sorts like the ids do, whatever torch's sort takes: uint64 beyond 2^63 through an order key."""
    big = 2 ** 63
    sets = [np.array([1, 5, big + 2], dtype=np.uint64), np.array([5, big, big + 2, 2 ** 64 - 1], dtype=np.uint64)]
    ids_out, rows = tensor_long._union_rows(torch, [torch.from_numpy(s) for s in sets], torch.uint64)
    assert ids_out.dtype == torch.uint64 and ids_out.numpy().tolist() == [1, 5, big, big + 2, 2 ** 64 - 1]
    assert [r.tolist() for r in rows] == [[0, 1, 3], [1, 2, 3, 4]]
    same, rows = tensor_long._union_rows(torch, [torch.tensor([-3, 4]), torch.tensor([-3, 4])], torch.int64)
    assert rows is None and same.tolist() == [-3, 4]
    ids_out, rows = tensor_long._union_rows(torch, [torch.tensor([-3, 4], dtype=torch.int8), torch.tensor([-5, 4], dtype=torch.int8)], torch.int8)
    assert ids_out.dtype == torch.int8 and ids_out.tolist() == [-5, -3, 4] and [r.tolist() for r in rows] == [[1, 2], [0, 2]]


def test_the_device_pointer_path_of_the_native_wrappers_needs_a_device_and_n_rows():
    buf = np.zeros(8, dtype=np.int64)
    if _native.device_count() == 0:   # (with a device tests/test_pack_rows_gpu.py runs the path)
        with pytest.raises(_native.NativeError) as ei:
            _native.DevicePackSet((buf.ctypes.data, _native.TSFA_I64, np.int64), None, None, space=_native.TSFA_DEVICE, n_rows=8)
        assert ei.value.code == _native.TSFA_ERR_NO_DEVICE
    with pytest.raises(ValueError, match="n_rows"):
        _native.DevicePackSet((buf.ctypes.data, _native.TSFA_I64, np.int64), None, None, space=_native.TSFA_DEVICE)
