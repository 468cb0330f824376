"""Input adapters: pandas containers -> ragged buffers (one per kind) for the C-ABI.

The reference wraps its three input formats in iterables of single `pd.Series`
(tsfresh/feature_extraction/data.py: WideTsFrameAdapter :181, LongTsFrameAdapter :233, TsDictAdapter :294,
to_tsdata :447) and then walks them one series at a time.  Here the same formats, checks and error messages
produce, per kind, ONE contiguous value buffer plus an offsets array: the `[n_ids x n_kinds x max_len]` ragged
layout the kernels consume.  Everything is vectorised (factorize + lexsort); no per-series Python.

A frame whose rows are NOT grouped by ascending id with every group in sort order (a sensor log written in time order, the
long format, a shuffled frame) can be packed on the device instead (`pack="device"` / `"auto"`, `_native.DevicePack`): the
columns are uploaded as they are, sorted and gathered there, and the ragged buffer goes to the kernels without returning.
A frame of several kinds -- a long frame whose kinds interleave, a wide frame with several value columns -- is sorted ONCE
(`_native.DevicePackSet`) and every kind is a view of that one sort.
"""
import warnings

import numpy as np
import pandas as pd

from tsfresh_amd import _native

_NATIVE_SCAN_MIN_ROWS = 1 << 18  # below this the numpy passes are as fast as spawning the scan threads
# pack="auto": rows of one kind from which a frame that is not in packed order is packed on the device: the smallest measured
# power of two at which the device route's median is below the host route's (profiles/pack_device_timing.md: 4.7 ms against
# 6.5 ms at 2^18 rows, 34 ms against 0.80 s at 2^24)
_DEVICE_PACK_MIN_ROWS = 1 << 18
# extract_rolled_features(pack="auto"): rows of the frame from which the device route (device packer + windows built on the
# device) is taken.  None: not measured end to end yet (profiles/roll_device_timing.md), "auto" keeps the
# host route; to be set to the smallest measured power of two at which the device median is below the host median.
_DEVICE_ROLL_MIN_ROWS = None
PACK_MODES = ("auto", "host", "device")


class _LazyHostValues:
    """The ragged buffer of a DevicePack, fetched from the device the first time the host looks at it (the data-dependent
    exceptions of the reference, a user's own calculators): an extraction that needs neither never copies the samples back."""

    def __init__(self, pack):
        self._pack, self._host = pack, None
        self.dtype = pack.values_dtype

    def _get(self):
        if self._host is None:
            self._host = self._pack.values_host()
        return self._host

    def __len__(self):
        return self._pack.n_rows

    def __getitem__(self, item):
        return self._get()[item]

    def __array__(self, dtype=None, copy=None):
        a = self._get()
        return a if dtype is None else a.astype(dtype, copy=False)


class PackedKind:
    """All series of one kind: `values[offsets[i]:offsets[i+1]]` is the series of `ids[i]` (ids sorted).
    With `device_pack` (a `_native.DevicePack`) the samples and the offsets live on the device: `values` is a lazy host view
    and `offsets` is fetched on first use."""

    def __init__(self, kind, ids, values, offsets, times=None, sort=None, device_pack=None):
        self.kind = kind
        self.ids = ids
        self.device_pack = device_pack
        self.values = values if device_pack is None else _LazyHostValues(device_pack)
        self._offsets = offsets
        self.times = times  # float64 hours since each series' first timestamp (DatetimeIndex input only)
        self.sort = sort    # the sort column in packed order (None without column_sort); names rolled windows
        self.sort_dtype = None   # device_pack made with keep_sort: the sort column's dtype (the pack keeps datetimes as ticks)

    @property
    def offsets(self):
        if self._offsets is None and self.device_pack is not None:
            self._offsets = self.device_pack.offsets
        return self._offsets

    @offsets.setter
    def offsets(self, value):
        self._offsets = value

    @property
    def n_series(self):
        if self.device_pack is not None:
            return self.device_pack.n_series
        return len(self.offsets) - 1


def _check_colname(*columns):
    # data.py:124-145
    for col in columns:
        if str(col).endswith("_"):
            raise ValueError("Dict keys are not allowed to end with '_': {}".format(col))
        if "__" in str(col):
            raise ValueError("Dict keys are not allowed to contain '__': {}".format(col))


def _check_nan(df, *columns, defer=()):
    # data.py:148-167.  Integer / boolean columns cannot hold NaN (no 20 M-row isnull() pass for an int64 id column);
    # columns in `defer` are checked by _pack (in the same native pass that finds the group boundaries).
    for col in columns:
        if col not in df.columns:
            raise ValueError("Column not found: {}".format(col))
        if col in defer or df[col].dtype.kind in "iub":
            continue
        if df[col].isnull().any():
            raise ValueError("Column must not contain NaN values: {}".format(col))


def _raise_if_nan(values, name):
    if name is not None and values.dtype.kind == "f" and bool(np.isnan(values).any()):
        raise ValueError("Column must not contain NaN values: {}".format(name))


def _get_value_columns(df, *other_columns):
    # data.py:170-178
    value_columns = [col for col in df.columns if col not in other_columns]
    if len(value_columns) == 0:
        raise ValueError("Could not guess the value column! Please hand it to the function as an argument.")
    return value_columns


def _as_values(column):
    arr = np.asarray(column)
    if arr.dtype == np.float32 or arr.dtype == np.float64:
        return arr   # read only from here on: no copy
    return arr.astype(np.float64)


def _hours_since_first(index, order, offsets):
    """Per sample: hours since the first timestamp of its series, with the arithmetic of the reference's
    linear_trend_timewise (feature_calculators.py:2291-2296): (ix - ix[0]).total_seconds() / 3600.0."""
    ix = index[order]
    counts = np.diff(offsets)
    first = ix[np.repeat(offsets[:-1], counts)]
    return np.ascontiguousarray(np.asarray((ix - first).total_seconds() / float(3600)), dtype=np.float64)


def _pack_presorted(kind, ids, values, sort_values, index, nan_name=None):
    """The usual layout of a long frame -- numeric ids already non-decreasing, every group already in sort order --
    needs no hashing and no permutation: the group boundaries are where the id changes (three linear passes over the
    rows instead of `factorize` + `bincount` + the element-wise sortedness test: 4x less packing time on 20 M rows).
    Returns None when the layout is anything else (the general path then sorts)."""
    if ids.dtype.kind not in "iuf" or len(ids) < 2:
        return None
    if len(ids) >= _NATIVE_SCAN_MIN_ROWS:
        # one multi-threaded native pass: layout proof + group boundaries + the NaN check of the value column
        # (a float32 / float64 column as it is; float16 / longdouble -- which CAN hold a NaN -- converted first, so that
        # the scan sees them; integer and bool columns cannot hold one and are only converted -- a full copy -- once the
        # layout is proven, so an unsorted integer frame is not converted twice)
        raw = np.asarray(values)
        if raw.dtype.kind == "f" and raw.dtype.itemsize not in (4, 8):
            raw = _as_values(raw)
        scanned = raw if raw.dtype.kind == "f" and raw.dtype.itemsize in (4, 8) else None
        sv = None if sort_values is None else np.asarray(sort_values)
        res = _native.pack_scan(ids, sv, scanned)
        if res is not None:
            flags, offsets = res
            if flags & _native.TSFA_PACK_VALUE_NAN and nan_name is not None:
                raise ValueError("Column must not contain NaN values: {}".format(nan_name))
            if offsets is None:
                return None
            vals = scanned if scanned is not None else _as_values(raw)
            times = _hours_since_first(index, slice(None), offsets) if index is not None else None
            return PackedKind(str(kind), ids[offsets[:-1]], np.ascontiguousarray(vals), offsets, times, sv)
    if not bool(np.all(ids[1:] >= ids[:-1])):  # also False for NaN ids
        return None
    cuts = np.flatnonzero(ids[1:] != ids[:-1]) + 1
    sv = None
    if sort_values is not None:
        sv = np.asarray(sort_values)
        try:
            bad = np.flatnonzero(sv[1:] < sv[:-1]) + 1  # descents are only allowed where a new id starts
        except TypeError:
            return None
        if len(bad) > len(cuts) or not bool(np.all(np.isin(bad, cuts, assume_unique=True))):
            return None
    offsets = np.empty(len(cuts) + 2, dtype=np.int64)
    offsets[0] = 0
    offsets[1:-1] = cuts
    offsets[-1] = len(ids)
    uniques = ids[offsets[:-1]]
    times = _hours_since_first(index, slice(None), offsets) if index is not None else None
    vals = np.ascontiguousarray(_as_values(values))
    _raise_if_nan(vals, nan_name)
    return PackedKind(str(kind), uniques, vals, offsets, times, sv)


def _device_key_columns(ids, sort_values, index=None):
    """The id and sort columns as the device packer reads them: -> (None, (ids column, unique labels or None, sort column or
    None)) or (reason, None); see `_device_pack_columns`."""
    ids = np.asarray(ids)
    if index is not None:
        return "the frame has a DatetimeIndex (linear_trend_timewise's times are computed on the host)", None
    if len(ids) < 1:
        return "the frame holds no rows", None
    labels = None
    if ids.dtype.kind in "OUS":
        codes, labels = pd.factorize(ids, sort=True)
        ids = np.ascontiguousarray(codes, dtype=np.int64)
        labels = np.asarray(labels)
    elif ids.dtype.kind not in "iu":
        return "the id column has dtype {} (integers, strings or objects are packed on the device)".format(ids.dtype), None
    id_col = _native.pack_column(ids)
    if id_col is None:
        return "the id column has dtype {}".format(ids.dtype), None
    sort_col = None
    if sort_values is not None:
        sv = np.asarray(sort_values)
        if sv.dtype.kind not in "iufmM" or (sv.dtype.kind == "f" and sv.dtype.itemsize not in (4, 8)):
            return "the sort column has dtype {} (integers, float32 / float64, datetime64 / timedelta64 are packed on " \
                   "the device)".format(sv.dtype), None
        sort_col = _native.pack_column(sv)
        if sort_col is None:
            return "the sort column has dtype {}".format(sv.dtype), None
    return None, (id_col, labels, sort_col)


def _device_value_column(values):
    """A value column as the device packer reads it: -> (None, column) or (reason, None)."""
    raw = np.asarray(values)
    if raw.dtype.kind not in "biuf" or (raw.dtype.kind == "f" and raw.dtype.itemsize not in (4, 8)):
        return "the value column has dtype {} (bool, integers, float32 / float64 are packed on the device)".format(
            raw.dtype), None
    val_col = _native.pack_column(raw)
    if val_col is None:
        return "the value column has dtype {}".format(raw.dtype), None
    return None, val_col


def _device_pack_columns(ids, values, sort_values, index=None):
    """What tsfa_pack_device would read for these columns: -> (None, (ids column, unique labels or None, sort column or
    None, value column)), each column as `_native.pack_column` returns it, or (reason, None) when the frame keeps the host
    route.  Eligible: integer ids (strings / objects are factorized to codes on the host first: that still leaves the
    lexsort and the gather to the device); a sort column of an integer type, float32 / float64, datetime64 / timedelta64,
    or none; a value column of bool, an integer type, float32 or float64.  NOT eligible, and follow-ups rather than part of
    the device packer: float ids, float16 / longdouble values, sort values that do not compare element-wise (objects),
    and frames with a DatetimeIndex (the `times` of linear_trend_timewise are pandas arithmetic, `_hours_since_first`).
    `extract_rolled_features` packs here as well (`keep_sort=True`: the packed sort column stays in HBM and only the stamps
    that name the windows come back, `_native.DeviceWindows.shift_values`)."""
    reason, keys = _device_key_columns(ids, sort_values, index)
    if reason is not None:
        return reason, None
    reason, val_col = _device_value_column(values)
    if reason is not None:
        return reason, None
    return None, keys + (val_col,)


def _pack_on_device(kind, columns, nan_name, device, sort_dtype=None):
    """sort_dtype: the sort column's dtype when the pack is to keep the packed sort column (keep_sort), else None."""
    id_col, labels, sort_col, val_col = columns
    dp = _native.DevicePack(id_col, sort_col, val_col, device=device, keep_sort=sort_dtype is not None)
    if dp.value_nan and nan_name is not None:
        dp.close()
        raise ValueError("Column must not contain NaN values: {}".format(nan_name))
    return _view_kind(kind, dp, labels, sort_dtype)


def _kept_sort_dtype(keep_sort, sort_values):
    return np.asarray(sort_values).dtype if keep_sort and sort_values is not None else None


def _pack(kind, ids, values, sort_values, index=None, nan_name=None, pack="host", device=0, keep_sort=False):
    """Group `values` by `ids` (ascending), each group ordered by `sort_values` (stable).  `index`: the frame's
    DatetimeIndex (row-aligned with `values`) or None.  nan_name: the value column's name if its NaN check
    (data.py:148-167) has been left to this function.
    pack: "host" -- factorize + lexsort + gather in numpy; "device" -- a frame that is not already in packed order is
    sorted and gathered on HIP device `device` (ValueError naming the reason when it is not eligible, see
    `_device_pack_columns`); "auto" -- the device for eligible frames of at least _DEVICE_PACK_MIN_ROWS rows when a device
    is visible, the host otherwise and (with one warning) when the device allocation fails.  The proof that a frame is
    already in packed order (`_pack_presorted`) always runs first: that layout costs what it cost before.
    keep_sort: the caller (`extract_rolled_features`) wants the samples, the offsets AND the packed sort column in HBM: where
    the device route is taken it is taken for a frame in packed order too (the packer proves the order itself and sorts
    nothing), the pack keeps the sort column, and the proof on the host only runs when the device does not take the frame."""
    ids = np.asarray(ids)
    postponed = keep_sort and _takes_device(pack, len(ids), True)
    fast = None if postponed else _pack_presorted(kind, ids, values, sort_values, index, nan_name)
    if fast is not None:
        return fast
    if postponed or (not keep_sort and _takes_device(pack, len(ids))):
        sort_dtype = _kept_sort_dtype(keep_sort, sort_values)
        reason, columns = _device_pack_columns(ids, values, sort_values, index)
        if reason is not None:
            if pack == "device":
                raise ValueError("pack='device': kind {!r} cannot be packed on the device: {}".format(str(kind), reason))
        elif pack == "device":
            return _pack_on_device(kind, columns, nan_name, device, sort_dtype)
        else:
            try:
                return _pack_on_device(kind, columns, nan_name, device, sort_dtype)
            except _native.NativeError as exc:
                if exc.code != _native.TSFA_ERR_HIP:
                    raise
                warnings.warn("kind {!r}: packing on the device failed ({}); packing on the host instead".format(
                    str(kind), exc), RuntimeWarning, stacklevel=2)
        if postponed:   # the device did not take the frame: the proof it was spared
            fast = _pack_presorted(kind, ids, values, sort_values, index, nan_name)
            if fast is not None:
                return fast
    _raise_if_nan(_as_values(values), nan_name)
    codes, uniques = pd.factorize(ids, sort=True)
    order = None
    if len(codes) > 1 and np.all(codes[1:] >= codes[:-1]):
        # already grouped by id in ascending order (the usual layout of a long frame): if every group is also in sort
        # order the permutation is the identity, and the 20M-row lexsort (90 % of the packing time) is skipped
        if sort_values is None:
            order = slice(None)
        else:
            try:
                sv = np.asarray(sort_values)
                if np.all((sv[1:] >= sv[:-1]) | (codes[1:] != codes[:-1])):
                    order = slice(None)
            except TypeError:  # sort values that do not compare element-wise
                order = None
    if order is None:
        if sort_values is not None:
            order = np.lexsort((np.asarray(sort_values), codes))
        else:
            order = np.argsort(codes, kind="stable")
    counts = np.bincount(codes, minlength=len(uniques))
    offsets = np.zeros(len(uniques) + 1, dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    times = _hours_since_first(index, order, offsets) if index is not None and len(codes) else None
    return PackedKind(str(kind), np.asarray(uniques), np.ascontiguousarray(_as_values(values)[order]), offsets, times,
                      None if sort_values is None else np.asarray(sort_values)[order])


def _takes_device(pack, n_rows, keep_sort=False):
    """The rule of `_pack` for a frame of n_rows rows that is not in packed order.  keep_sort (the rolled extraction, where
    the device route also builds the windows and takes frames in packed order): its own threshold."""
    min_rows = _DEVICE_ROLL_MIN_ROWS if keep_sort else _DEVICE_PACK_MIN_ROWS
    return pack == "device" or (pack == "auto" and min_rows is not None and n_rows >= min_rows and _native.device_count() > 0)


def _view_kind(kind, dp, labels, sort_dtype=None):
    pk = PackedKind(str(kind), dp.ids if labels is None else labels[dp.ids], None, None, None, None, device_pack=dp)
    pk.sort_dtype = sort_dtype
    return pk


def _close_all(kinds):
    for pk in kinds:
        if pk is not None and pk.device_pack is not None:
            pk.device_pack.close()


def _pack_long_on_device(kuniq, kcodes, ids, values, sort_values, index, pack, device, keep_sort=False):
    """A long frame whose kinds interleave, sorted ONCE on the device by (kind, id, sort) (`_native.DevicePackSet`): no
    per-kind selection on the host, one upload, one sort, one gather; every kind is a view into the one gathered buffer.
    -> [PackedKind per kind of kuniq], or None when the frame keeps the per-kind route (not eligible under "auto"; a device
    allocation that failed, after one warning)."""
    reason, columns = _device_pack_columns(ids, values, sort_values, index)
    if reason is not None:
        if pack == "device":
            raise ValueError("pack='device': kind {!r} cannot be packed on the device: {}".format(str(kuniq[0]), reason))
        return None
    id_col, labels, sort_col, val_col = columns
    n_kinds = len(kuniq)   # dense codes 0 .. n_kinds - 1 in the narrowest type: one radix pass per byte
    kind_col = _native.pack_column(kcodes.astype(np.uint8 if n_kinds <= 1 << 8 else np.uint16 if n_kinds <= 1 << 16 else np.int64))
    try:
        with _native.DevicePackSet(id_col, sort_col, kind_col, device=device, keep_sort=keep_sort) as pack_set:
            packs = pack_set.values(val_col)
    except _native.NativeError as exc:
        if pack == "device" or exc.code != _native.TSFA_ERR_HIP:
            raise
        warnings.warn("packing the frame's {} kinds on the device failed ({}); packing on the host instead".format(
            n_kinds, exc), RuntimeWarning, stacklevel=3)
        return None
    sort_dtype = _kept_sort_dtype(keep_sort, sort_values)
    return [_view_kind(kind, dp, labels, sort_dtype) for kind, dp in zip(kuniq, packs)]


def _pack_wide(columns, ids, sort_values, index, pack, device, keep_sort=False):
    """The value columns of a wide frame: `columns` is [(name, values, nan_name or None)].  With at least two columns the
    device packer takes and rows that are not in packed order, the id and sort columns are uploaded, keyed, sorted and
    boundary-scanned ONCE (`_native.DevicePackSet` without a kind column) and every value column is one gather through the
    stored permutation; the packs share the set's offsets and ids.  Everything else is `_pack` per column, as before.
    keep_sort: as in `_pack` -- the set keeps the packed sort column and a frame in packed order goes to the device as well."""
    ids = np.asarray(ids)

    def per_column(todo, mode):
        return [_pack(name, ids, values, sort_values, index, nan_name=nan_name, pack=mode, device=device, keep_sort=keep_sort)
                for name, values, nan_name in todo]

    if len(columns) < 2 or pack == "host" or not _takes_device(pack, len(ids), keep_sort):
        return per_column(columns, pack)
    name0, values0, nan_name0 = columns[0]
    first = None if keep_sort else _pack_presorted(name0, ids, values0, sort_values, index, nan_name0)
    if first is not None:   # the frame is in packed order: every column costs what it cost before
        return [first] + per_column(columns[1:], pack)
    reason, keys = _device_key_columns(ids, sort_values, index)
    value_cols = [_device_value_column(values) for _, values, _ in columns]
    if reason is not None or sum(r is None for r, _ in value_cols) < 2:
        return per_column(columns, pack)   # (raises under "device" where a column is not eligible)
    id_col, labels, sort_col = keys
    sort_dtype = _kept_sort_dtype(keep_sort, sort_values)
    packed = []
    try:
        with _native.DevicePackSet(id_col, sort_col, None, device=device, keep_sort=keep_sort) as pack_set:
            for (name, values, nan_name), (why, val_col) in zip(columns, value_cols):
                if why is not None:
                    if pack == "device":
                        raise ValueError("pack='device': kind {!r} cannot be packed on the device: {}".format(str(name), why))
                    packed.append(_pack(name, ids, values, sort_values, index, nan_name=nan_name, pack="host"))
                    continue
                dp = pack_set.values(val_col)[0]
                packed.append(_view_kind(name, dp, labels, sort_dtype))
                if dp.value_nan and nan_name is not None:
                    raise ValueError("Column must not contain NaN values: {}".format(nan_name))
    except _native.NativeError as exc:
        _close_all(packed)
        if pack == "device" or exc.code != _native.TSFA_ERR_HIP:
            raise
        warnings.warn("packing the frame's {} value columns on the device failed ({}); packing on the host instead".format(
            len(columns), exc), RuntimeWarning, stacklevel=3)
        return per_column(columns, "host")
    except Exception:
        _close_all(packed)
        raise
    return packed


def _arrow_to_frame(table):
    """A pyarrow Table / RecordBatch as a DataFrame, column by column through numpy (no Python objects for primitive
    columns; pandas still consolidates the columns into its own blocks): the checks and the packing below then see an
    ordinary long / wide frame."""
    cols = {}
    for name in table.schema.names:
        col = table.column(name)
        if hasattr(col, "combine_chunks"):
            col = col.combine_chunks()
        try:
            cols[name] = col.to_numpy(zero_copy_only=True)
        except Exception:  # strings, nulls, chunk boundaries: Arrow has to materialise a copy
            cols[name] = col.to_numpy(zero_copy_only=False)
    return pd.DataFrame(cols, copy=False)


def _pack_arrow_wide(table, column_id, column_kind, column_value, column_sort, pack="host", device=0, keep_sort=False):
    """Wide-format pyarrow Table / RecordBatch with primitive, null-free columns: the Arrow buffers go to the packer as
    numpy views (zero copy) -- no pandas frame, no block consolidation.  None -> the caller converts to a DataFrame
    and takes the general route (strings, nulls, chunked columns that need a copy, the long format)."""
    if column_id is None or column_kind is not None:
        return None
    names = list(table.schema.names)
    if column_id not in names or (column_sort is not None and column_sort not in names):
        return None
    value_columns = [column_value] if column_value is not None else [c for c in names if c not in (column_id, column_sort)]
    if not value_columns or any(c not in names for c in value_columns):
        return None
    arrays = {}
    for name in [column_id] + ([column_sort] if column_sort is not None else []) + value_columns:
        col = table.column(name)
        if getattr(col, "null_count", 0):
            return None
        if hasattr(col, "num_chunks"):
            if col.num_chunks != 1:
                return None
            col = col.chunk(0)
        try:
            arrays[name] = col.to_numpy(zero_copy_only=True)
        except Exception:
            return None
        if arrays[name].dtype.kind not in "iuf":
            return None
    _check_colname(*value_columns)
    for name in [column_id] + ([column_sort] if column_sort is not None else []):
        _raise_if_nan(arrays[name], name)
    ids = arrays[column_id]
    sort_all = arrays[column_sort] if column_sort is not None else None
    packed = _pack_wide([(c, arrays[c], c) for c in value_columns], ids, sort_all, None, pack, device, keep_sort)
    return packed, ids.dtype, False


def pack_timeseries(container, column_id=None, column_kind=None, column_value=None, column_sort=None, pack="host",
                    device=0, keep_sort=False):
    """-> (list[PackedKind] in output-column order, dtype of the id column, has_datetime_index).
    pack / device: see `_pack` ("host": every kind is packed in numpy, as before the device packer existed).
    keep_sort: see `_pack` (only `extract_rolled_features` asks for it; the default leaves every route as it was)."""
    if pack not in PACK_MODES:
        raise ValueError("pack must be one of {}, not {!r}".format(", ".join(repr(m) for m in PACK_MODES), pack))
    if type(container).__module__.startswith("pyarrow") and hasattr(container, "schema"):
        direct = _pack_arrow_wide(container, column_id, column_kind, column_value, column_sort, pack, device, keep_sort)
        if direct is not None:
            return direct
        container = _arrow_to_frame(container)
    if isinstance(container, pd.DataFrame):
        df = container
        if column_id is None:
            raise ValueError("A value for column_id needs to be supplied")
        if column_kind is not None:
            # long format (data.py:233-291)
            if column_value is None:
                possible = _get_value_columns(df, column_id, column_sort, column_kind)
                if len(possible) != 1:
                    raise ValueError(
                        "Could not guess the value column, as the number of unused columns os not equal to 1."
                        "These columns where currently unused: {}"
                        "Please hand it to the function as an argument.".format(",".join(map(str, possible))))
                column_value = possible[0]
            _check_nan(df, column_id, column_kind, column_value)
            if column_sort is not None:
                _check_nan(df, column_sort)
            kinds = df[column_kind].to_numpy()
            dt_index = df.index if isinstance(df.index, pd.DatetimeIndex) else None
            kcodes, kuniq = pd.factorize(kinds, sort=True)
            packed = []
            ids_all = df[column_id].to_numpy()
            vals_all = df[column_value].to_numpy()
            sort_all = df[column_sort].to_numpy() if column_sort is not None else None
            interleaved = len(kcodes) > 1 and not bool(np.all(kcodes[1:] >= kcodes[:-1]))
            if interleaved and pack != "host" and _takes_device(pack, len(kcodes), keep_sort):
                # kinds that interleave (rows in (id, time) or time order): one sort of the whole frame on the device.
                # A frame whose kinds come in blocks keeps the per-kind route below, where a packed block costs a proof.
                views = _pack_long_on_device(kuniq, kcodes, ids_all, vals_all, sort_all, dt_index, pack, device, keep_sort)
                if views is not None:
                    return views, df[column_id].dtype, False
                pack = "host"   # "auto": not eligible, or the allocation failed and the warning is out
            for k, kind in enumerate(kuniq):
                sel = np.nonzero(kcodes == k)[0]
                packed.append(_pack(kind, ids_all[sel], vals_all[sel], None if sort_all is None else sort_all[sel],
                                    None if dt_index is None else dt_index[sel], pack=pack, device=device,
                                    keep_sort=keep_sort))
            return packed, df[column_id].dtype, isinstance(df.index, pd.DatetimeIndex)
        # wide format (data.py:181-230)
        _check_nan(df, column_id)
        value_columns = [column_value] if column_value is not None else _get_value_columns(df, column_id, column_sort)
        deferred = [c for c in value_columns if c in df.columns and df[c].dtype.kind == "f"]
        _check_nan(df, *value_columns, defer=deferred)
        _check_colname(*value_columns)
        if column_sort is not None:
            _check_nan(df, column_sort)
        ids_all = df[column_id].to_numpy()
        sort_all = df[column_sort].to_numpy() if column_sort is not None else None
        dt_index = df.index if isinstance(df.index, pd.DatetimeIndex) else None
        packed = _pack_wide([(col, df[col].to_numpy(), col if col in deferred else None) for col in value_columns],
                            ids_all, sort_all, dt_index, pack, device, keep_sort)
        return packed, df[column_id].dtype, isinstance(df.index, pd.DatetimeIndex)
    if isinstance(container, dict):
        # dict of frames, one per kind (data.py:294-338)
        _check_colname(*list(container.keys()))
        for frame in container.values():
            _check_nan(frame, column_id, column_value)
        if column_sort is not None:
            for frame in container.values():
                _check_nan(frame, column_sort)
        packed, id_dtype, has_dt = [], None, False
        for kind, frame in container.items():
            sort_vals = frame[column_sort].to_numpy() if column_sort is not None else None
            packed.append(_pack(kind, frame[column_id].to_numpy(), frame[column_value].to_numpy(), sort_vals,
                                frame.index if isinstance(frame.index, pd.DatetimeIndex) else None, pack=pack, device=device,
                                keep_sort=keep_sort))
            id_dtype = frame[column_id].dtype
            has_dt = has_dt or isinstance(frame.index, pd.DatetimeIndex)
        return packed, id_dtype, has_dt
    raise ValueError("df must be a DataFrame or a dict of DataFrames. "
                     "See https://tsfresh.readthedocs.io/en/latest/text/data_formats.html")
