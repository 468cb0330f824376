"""`nan_policy="drop"` on the tensor entries above the kernels: the values are those of the wide frame after `dropna()`, the
rolled entry's positions are original step indices, the default policy makes exactly the calls it made before, a bad policy
name and a series without a kept step are `ValueError`s -- on CPU tensors, with the g++ builds of the valid-step packer's, the
times packer's and the window builder's bodies standing in for the device and the numpy plan of test_tensor_times_routes.py
standing in for the kernels.  No GPU needed."""
import numpy as np
import pandas as pd
import pytest
import torch

import emul_pack_valid_lib as epv
import test_tensor_times_routes as ttr
import tsfresh_amd
from tsfresh_amd import MinimalFCParameters, _native, extract_features, extract_rolled_features, tensor, tensor_selection
from tsfresh_amd.feature_extraction import extraction

TIMEWISE = ttr.TIMEWISE
NAT = np.iinfo(np.int64).min
CALLS = ttr.CALLS
LENGTHS = [9, 5, 2, 6]


def _emul_valid_pack(torch_, x3, lengths, times, device):
    t = unit = None
    if times is not None:
        tt, t_type, tps = times
        t = tt.numpy()
        assert t.strides == tuple(8 * s for s in tt.stride())   # the view's own strides reach the packer
        unit = {v: k for k, v in epv.ept.TICKS_PER_SECOND.items()}[tps]
    CALLS.append(("_valid_pack", tuple(x3.shape), None if lengths is None else lengths.tolist(), times is not None, device))
    res = epv.EmulValid(x3.numpy(), lengths=None if lengths is None else lengths.numpy(), t=t, unit=unit or "ns")
    assert res.status == 0 and res.guards_intact
    packs = [ttr._EmulChannel(res.values[c], res.offsets, device) for c in range(x3.shape[1])]
    hours = None if res.hours is None else torch.from_numpy(res.hours)
    return packs, torch.tensor([res.flags], dtype=torch.int32), hours, torch.from_numpy(res.steps), torch.from_numpy(res.offsets)


def _forbidden(name):
    def fail(*a, **k):
        raise AssertionError(name + " was called")
    return fail


@pytest.fixture
def emulated(monkeypatch):
    monkeypatch.setattr(extraction, "_acquire_plan", lambda fplan, device, pins=None: ttr._NumpyPlan(len(fplan.names)))
    monkeypatch.setattr(tensor, "_valid_pack", _emul_valid_pack)
    monkeypatch.setattr(tensor, "_dense_pack", _forbidden("_dense_pack"))
    monkeypatch.setattr(tensor, "_times_pack", _forbidden("_times_pack"))
    monkeypatch.setattr(tensor, "_roll_windows", ttr._emul_roll_windows)
    monkeypatch.setattr(tensor, "_to_device", lambda t, device: t)
    monkeypatch.setattr(tensor, "_synchronize", lambda torch_, device: None)
    del CALLS[:]


def _batch(B=4, C=2, n=9, seed=0):
    """x (B, C, n) with NaN placed per kind -- one inside every series, in different kinds, and one beyond a length --, the
    (B, n) stamps with a NaT on a step whose values are fine."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, C, n))
    x[0, 0, 3] = x[0, 1, 5] = np.nan
    x[1, 1, 0] = np.nan                      # a series that loses its first step
    x[1, 0, 7] = np.nan                      # beyond lengths[1] = 5: never read
    x[3, 0, 4] = x[3, 1, 4] = np.nan
    x[3, 1, 1] = np.inf                      # a value
    t = ttr._stamps(B, n)
    t[0, 7] = NAT
    t[2, 5] = NAT                            # beyond lengths[2] = 2
    return x, t


def _dropped_frame(x, kinds, lengths=None, stamps=None, unit="ns"):
    """The wide frame of the batch after dropna(): columns id, t (the step index) and the kinds; with stamps they are its
    DatetimeIndex (a NaT stamp is dropped with its row)."""
    B, C, n = x.shape
    lens = np.full(B, n) if lengths is None else np.asarray(lengths)
    cols = {"id": np.repeat(np.arange(B), lens), "t": np.concatenate([np.arange(k) for k in lens])}
    for c, kind in enumerate(kinds):
        cols[kind] = np.concatenate([x[b, c, :lens[b]] for b in range(B)])
    if stamps is not None:
        cols["stamp"] = np.concatenate([stamps[b, :lens[b]] for b in range(B)]).view("datetime64[%s]" % unit)
    frame = pd.DataFrame(cols).dropna()
    if stamps is not None:
        frame = frame.set_index(pd.DatetimeIndex(frame.pop("stamp")))
    return frame


@pytest.mark.parametrize("lengths", (None, LENGTHS), ids=("dense", "ragged"))
@pytest.mark.parametrize("timed", (False, True), ids=("plain", "times"))
def test_values_are_those_of_the_frame_after_dropna(emulated, lengths, timed):
    x, t = _batch()
    kinds = ["b", "a"]
    params = dict(MinimalFCParameters(), **(TIMEWISE if timed else {}))
    frame = _dropped_frame(x, kinds, lengths, t if timed else None)
    assert len(frame) < (sum(lengths) if lengths else 36)
    want = extract_features(frame.drop(columns="t"), column_id="id", default_fc_parameters=params, pack="host")
    for check_nan in (True, False):   # irrelevant under "drop"
        feats, cols = tsfresh_amd.extract_features_tensor(x, lengths=lengths, kinds=kinds, default_fc_parameters=params,
                                                          nan_policy="drop", check_nan=check_nan, times=t if timed else None, device=0)
        assert cols == list(want.columns)
        assert np.array_equal(feats.numpy(), want.to_numpy())
    assert [c[0] for c in CALLS] == ["_valid_pack"] * 2 and CALLS[0][1:] == ((4, 2, 9), lengths, timed, 0)
    # other forms of the same batch
    forms = [dict(x=torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))), channels_last=True),
             dict(x=x.astype(np.float32))]
    for kw in forms:
        feats, _ = tsfresh_amd.extract_features_tensor(lengths=lengths, kinds=kinds, default_fc_parameters=params, nan_policy="drop",
                                                       times=torch.from_numpy(t) if timed else None, **kw)
        if kw["x"].dtype in (np.float32, torch.float32):
            f32 = _dropped_frame(x.astype(np.float32).astype(np.float64), kinds, lengths, t if timed else None)
            want32 = extract_features(f32.drop(columns="t"), column_id="id", default_fc_parameters=params, pack="host")
            assert np.array_equal(feats.numpy(), want32.to_numpy())
        else:
            assert np.array_equal(feats.numpy(), want.to_numpy())


def test_one_clock_for_the_batch_drops_its_nat_steps_everywhere(emulated):
    x, t = _batch()
    clock = t[0]                             # NaT at step 7
    params = dict(MinimalFCParameters(), **TIMEWISE)
    want = extract_features(_dropped_frame(x, ["0", "1"], LENGTHS, np.broadcast_to(clock, t.shape)).drop(columns="t"), column_id="id",
                            default_fc_parameters=params, pack="host")
    feats, cols = tsfresh_amd.extract_features_tensor(x, lengths=LENGTHS, default_fc_parameters=params, nan_policy="drop", times=clock)
    assert cols == list(want.columns) and np.array_equal(feats.numpy(), want.to_numpy())


@pytest.mark.parametrize("roll", (dict(max_timeshift=4), dict(rolling_direction=-1, max_timeshift=4), dict(rolling_direction=2, min_timeshift=1),
                                  dict(rolling_direction=-2, max_timeshift=3)), ids=("dir1", "dir-1", "dir2", "dir-2"))
@pytest.mark.parametrize("lengths", (None, LENGTHS), ids=("dense", "ragged"))
def test_rolled_entry_equals_the_frame_and_positions_are_original_steps(emulated, roll, lengths):
    x, _ = _batch()
    kinds = ["b", "a"]
    frame = _dropped_frame(x, kinds, lengths)
    want = extract_rolled_features(frame, column_id="id", column_sort="t", default_fc_parameters=MinimalFCParameters(), pack="host", **roll)
    feats, cols, series, positions = tsfresh_amd.extract_rolled_features_tensor(
        x, lengths=lengths, kinds=kinds, default_fc_parameters=MinimalFCParameters(), nan_policy="drop", **roll)
    assert cols == list(want.columns)
    assert positions.dtype == torch.int64 and series.dtype == torch.int64
    assert list(zip(series.tolist(), positions.tolist())) == list(want.index)   # the t half is the ORIGINAL step index
    assert np.array_equal(feats.numpy(), want.to_numpy())
    kept = {b: frame.loc[frame["id"] == b, "t"].tolist() for b in range(4)}
    assert any(kept[b] != list(range(len(kept[b]))) for b in kept)               # (steps were dropped before the end)
    assert all(p in kept[s] for s, p in zip(series.tolist(), positions.tolist()))


def test_rolled_entry_with_times(emulated):
    x, t = _batch()
    kinds = ["b", "a"]
    params = dict(MinimalFCParameters(), **TIMEWISE)
    frame = _dropped_frame(x, kinds, LENGTHS, t)
    steps = frame.pop("t")
    want = extract_rolled_features(frame, column_id="id", default_fc_parameters=params, pack="host", max_timeshift=3)
    feats, cols, series, positions = tsfresh_amd.extract_rolled_features_tensor(x, lengths=LENGTHS, kinds=kinds, default_fc_parameters=params,
                                                                                nan_policy="drop", times=t, max_timeshift=3)
    assert cols == list(want.columns) and np.array_equal(feats.numpy(), want.to_numpy())
    assert series.tolist() == [i for i, _ in want.index]
    # the frame's own window names count the kept rows; the tensor entry names the original step of each
    per_series = {b: steps[(frame["id"] == b).to_numpy()].tolist() for b in range(4)}
    assert positions.tolist() == [per_series[i][k] for i, k in want.index]


def test_relevant_entry_passes_the_policy_on(emulated, monkeypatch):
    seen = {}

    def select(features, y, columns=None, **kw):
        seen["columns"], seen["features"] = list(columns), features.clone()
        return features[:, :1], [columns[0]], torch.tensor([0], dtype=torch.int32)

    monkeypatch.setattr(tensor_selection, "impute_tensor", lambda X: X)
    monkeypatch.setattr(tensor_selection, "select_features_tensor", select)
    x, t = _batch()
    got, names = tsfresh_amd.extract_relevant_features_tensor(x, np.array([0, 1, 0, 1]), lengths=LENGTHS, kinds=["b", "a"],
                                                              default_fc_parameters=MinimalFCParameters(), nan_policy="drop")
    want = extract_features(_dropped_frame(x, ["b", "a"], LENGTHS).drop(columns="t"), column_id="id",
                            default_fc_parameters=MinimalFCParameters(), pack="host")
    assert seen["columns"] == list(want.columns) and np.array_equal(seen["features"].numpy(), want.to_numpy())
    assert names == [want.columns[0]]


def test_default_policy_makes_the_calls_made_before(monkeypatch):
    monkeypatch.setattr(extraction, "_acquire_plan", lambda fplan, device, pins=None: ttr._UntimedPlan(len(fplan.names)))
    monkeypatch.setattr(tensor, "_dense_pack", ttr._emul_dense_pack)
    monkeypatch.setattr(tensor, "_times_pack", ttr._emul_times_pack)
    monkeypatch.setattr(tensor, "_valid_pack", _forbidden("_valid_pack"))
    monkeypatch.setattr(tensor, "_roll_windows", ttr._emul_roll_windows)
    monkeypatch.setattr(tensor, "_to_device", lambda t, device: t)
    monkeypatch.setattr(tensor, "_synchronize", lambda torch_, device: None)
    x = ttr._x()
    n = len(MinimalFCParameters())
    for kw in ({}, dict(nan_policy="raise")):
        del CALLS[:]
        tsfresh_amd.extract_features_tensor(x, lengths=[9, 1, 2, 6], kinds=["u", "v"], default_fc_parameters=MinimalFCParameters(), device=0, **kw)
        assert CALLS == [("_dense_pack", (4, 2, 9), [9, 1, 2, 6], 0), ("extract_into", None, None, 0, None), ("extract_into", None, None, n, None)]
        del CALLS[:]
        tsfresh_amd.extract_rolled_features_tensor(x, kinds=["u", "v"], default_fc_parameters=MinimalFCParameters(), max_timeshift=3, device=0, **kw)
        assert CALLS == [("_dense_pack", (4, 2, 9), None, 0), ("extract_windows_into", 0), ("extract_windows_into", n)]
    # and a NaN still raises, under either value of check_nan's sibling
    xn, _ = _batch()
    with pytest.raises(ValueError, match="Column must not contain NaN values: 0$"):
        tsfresh_amd.extract_features_tensor(xn, default_fc_parameters=MinimalFCParameters(), nan_policy="raise")


def test_a_bad_policy_name_is_a_value_error(emulated):
    x, _ = _batch()
    y = np.array([0, 1, 0, 1])
    for bad in ("omit", "propagate", None, True, "Drop"):
        for call in (lambda: tsfresh_amd.extract_features_tensor(x, nan_policy=bad),
                     lambda: tsfresh_amd.extract_rolled_features_tensor(x, max_timeshift=2, nan_policy=bad),
                     lambda: tsfresh_amd.extract_relevant_features_tensor(x, y, nan_policy=bad)):
            with pytest.raises(ValueError, match="nan_policy must be one of 'raise', 'drop'"):
                call()
    assert not CALLS   # refused before anything moved


def test_an_empty_series_is_a_value_error_with_its_index(emulated):
    x, t = _batch()
    x[2, 1, :2] = np.nan                     # series 2 has two steps
    for entry, kw in ((tsfresh_amd.extract_features_tensor, {}), (tsfresh_amd.extract_rolled_features_tensor, dict(max_timeshift=2))):
        with pytest.raises(ValueError, match="series 2 has no step left"):
            entry(x, lengths=LENGTHS, default_fc_parameters=MinimalFCParameters(), nan_policy="drop", **kw)
    # by the stamps alone
    x, t = _batch()
    t[1, :5] = NAT
    with pytest.raises(ValueError, match="series 1 has no step left.*NaT"):
        tsfresh_amd.extract_features_tensor(x, lengths=LENGTHS, default_fc_parameters=MinimalFCParameters(), nan_policy="drop", times=t)
    # a bad length is reported first, as under the default policy
    with pytest.raises(ValueError, match=r"lengths must lie in \[1, 9\]"):
        tsfresh_amd.extract_features_tensor(x, lengths=[9, 0, 2, 6], default_fc_parameters=MinimalFCParameters(), nan_policy="drop")


def test_nan_policy_stands_before_times_in_the_signatures():
    import inspect
    for entry in (tensor.extract_features_tensor, tensor.extract_rolled_features_tensor, tensor_selection.extract_relevant_features_tensor):
        names = list(inspect.signature(entry).parameters)
        assert names[-3:] == ["nan_policy", "times", "time_unit"]
        assert inspect.signature(entry).parameters["nan_policy"].default == "raise"


def test_the_constant_is_the_header_s():
    assert _native.TSFA_DENSE_EMPTY_SERIES == 32 and "tsfa_pack_dense_valid" in _native.EXPORTS
