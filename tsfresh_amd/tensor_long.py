"""`extract_features_long_tensor`: features of a frame held as COLUMN tensors -- tsfresh's own container, one row per
(id, sort, kind, value) with the ids interleaved -- without pandas.

`extract_features_tensor` takes rectangular batches.  A decoded log, a simulation, the output of another GPU stage is a table:
an id column, maybe a sort column, and either several value columns (the wide form) or a kind column and one value column
(the long form).  Here those columns go to the device packer as they lie in HBM (`tsfa_pack_set_create` with TSFA_DEVICE
pointers: one stable radix sort by (kind, id, sort)); the values follow through the stored permutation -- the wide form's
`[N, C]` matrix in ONE pass (`tsfa_pack_set_rows`), the long form's column with `tsfa_pack_set_values` --; with `times=` the
stamps become hours since each series' first stamp in the same order (`tsfa_pack_set_hours`); and the kinds' packs go to the
kernels `extract_features` runs, through the same FCParameters handling, plan cache and composite plans.  The feature matrix
and the ids of its rows stay on the device.

Scratch of the pack while the call runs: 40 bytes per row (two buffers of 16-byte composite key + 4-byte row index), as for
`extract_features(pack="device")`; the set keeps 4 bytes per row (the permutation) until the call returns.

Not offered: `nan_policy="drop"` (drop the rows with torch first), a rolled twin, an enqueue-only mode, string or float ids
(factorize them first: the codes are integer ids).
"""
import numpy as np

from tsfresh_amd import _native
from tsfresh_amd.tensor import _kind_jobs, _synchronize, _times_argument, _to_device

# torch dtype name -> (tsfa_dtype, numpy dtype); the names are compared as strings: torch is imported inside the function,
# and an older torch simply lacks the wider unsigned names
_INT_TYPES = {"torch.int8": (_native.TSFA_I8, np.int8), "torch.int16": (_native.TSFA_I16, np.int16),
              "torch.int32": (_native.TSFA_I32, np.int32), "torch.int64": (_native.TSFA_I64, np.int64),
              "torch.uint8": (_native.TSFA_U8, np.uint8), "torch.uint16": (_native.TSFA_U16, np.uint16),
              "torch.uint32": (_native.TSFA_U32, np.uint32), "torch.uint64": (_native.TSFA_U64, np.uint64)}
_FLOAT_TYPES = {"torch.float32": (_native.TSFA_F32, np.float32), "torch.float64": (_native.TSFA_F64, np.float64)}
_VALUE_TYPES = dict(_INT_TYPES, **_FLOAT_TYPES)
_VALUE_TYPES["torch.bool"] = (_native.TSFA_BOOL, np.bool_)
_SORT_TYPES = dict(_INT_TYPES, **_FLOAT_TYPES)

_MAX_ROWS = 2 ** 32 - 1   # the permutation's row indices are 32 bits wide

_INSTEAD = "build a DataFrame and call extract_features on it"


def _column(torch, a, what, types, allowed):
    """`a` as a torch tensor whose dtype is in `types` -> tensor; TypeError naming the dtype otherwise.  A numpy array
    becomes a tensor over the same memory (a view with negative strides or foreign byte order is copied once)."""
    if isinstance(a, np.ndarray):
        if a.dtype.kind not in "biuf":
            raise TypeError("{} must be {}, not {}".format(what, allowed, a.dtype))
        if any(s < 0 for s in a.strides) or not a.dtype.isnative:
            a = np.ascontiguousarray(a, dtype=a.dtype.newbyteorder("="))
        try:
            a = torch.from_numpy(a)
        except TypeError:
            raise TypeError("{} must be {}, not {}".format(what, allowed, a.dtype)) from None
    if not isinstance(a, torch.Tensor):
        raise TypeError("{} must be a torch.Tensor or a numpy array, not {}".format(what, type(a).__name__))
    if str(a.dtype) not in types:
        raise TypeError("{} must be {}, not {}".format(what, allowed, a.dtype))
    return a


def _long_arguments(torch, ids, values, sort, kinds, kind_names, times, time_unit, default_fc_parameters,
                    kind_to_fc_parameters, device):
    """Every check that needs no device -> (ids, values [N, C] or [N], sort, kinds, names, times, default_fc_parameters,
    device).  names: the wide form's C kind names, or for the long form a function code -> name.  Nothing has moved yet."""
    from tsfresh_amd.feature_extraction import extraction
    from tsfresh_amd.feature_extraction.data import _check_colname
    from tsfresh_amd.feature_extraction.plan import compile_fc_parameters
    from tsfresh_amd.feature_extraction.registry import UnsupportedFeature
    from tsfresh_amd.feature_extraction.settings import ComprehensiveFCParameters

    ids = _column(torch, ids, "ids", _INT_TYPES, "of an integer dtype (factorize string or float ids first)")
    values = _column(torch, values, "values", _VALUE_TYPES, "float32, float64, bool or of an integer dtype")
    if sort is not None:
        sort = _column(torch, sort, "sort", _SORT_TYPES, "float32, float64 or of an integer dtype")
    if kinds is not None:
        kinds = _column(torch, kinds, "kinds", _INT_TYPES, "integer codes")
    if ids.ndim != 1:
        raise ValueError("ids must be one-dimensional: got {} dimensions".format(ids.ndim))
    N = int(ids.shape[0])
    if N < 1:
        raise ValueError("the frame must hold at least one row")
    if N > _MAX_ROWS:
        raise ValueError("more than 4 294 967 295 rows (the packer's row indices are 32 bits wide)")
    if kinds is not None and values.ndim != 1:
        raise ValueError("kinds goes with one value column (the long form): values has {} dimensions".format(values.ndim))
    if values.ndim not in (1, 2):
        raise ValueError("values must have shape (N,) or (N, C): got {} dimensions".format(values.ndim))
    for what, col in (("values", values), ("sort", sort), ("kinds", kinds)):
        if col is not None and (col.shape[0] != N or (what != "values" and col.ndim != 1)):
            raise ValueError("{} must have one entry per row ({}): got shape {}".format(what, N, tuple(col.shape)))
    if values.ndim == 2 and values.shape[1] < 1:
        raise ValueError("values must hold at least one column: got shape {}".format(tuple(values.shape)))

    if kinds is None:
        C = 1 if values.ndim == 1 else int(values.shape[1])
        names = [str(c) for c in range(C)] if kind_names is None else [str(k) for k in kind_names]
        if len(names) != C:
            raise ValueError("kind_names must name the {} value columns: got {} names".format(C, len(names)))
        if len(set(names)) != C:
            raise ValueError("kind_names must be distinct")
        _check_colname(*names)
    elif kind_names is None:
        names = str
    else:
        pairs = kind_names.items() if hasattr(kind_names, "keys") else enumerate(kind_names)
        table = {int(code): str(name) for code, name in pairs if name is not None}
        if len(set(table.values())) != len(table):
            raise ValueError("kind_names must be distinct")
        names = table.get

    if times is not None:
        times = _times_argument(torch, times, time_unit, 1, N)
        if times[0].ndim != 1:
            raise ValueError("times must have one stamp per row, shape ({},): got {}".format(N, tuple(times[0].shape)))

    if default_fc_parameters is None and kind_to_fc_parameters is None:
        default_fc_parameters = ComprehensiveFCParameters()
    elif default_fc_parameters is None:
        default_fc_parameters = {}
    # the long form learns its kinds from the pack: a callable calculator anywhere in the settings is refused before it
    for fc_parameters in [default_fc_parameters] + list((kind_to_fc_parameters or {}).values()):
        if any(callable(key) for key in fc_parameters) and compile_fc_parameters(fc_parameters, has_datetime_index=times is not None).host_calls:
            raise UnsupportedFeature("custom (callable) calculators are evaluated per series on the host: " + _INSTEAD)
    if device is None:
        on_device = [t for t in (ids, values) if t.is_cuda]
        device = on_device[0].device.index if on_device else extraction._default_device()
    return ids, values, sort, kinds, names, times, default_fc_parameters, int(device)


def _key_column(t):
    """A contiguous 1-D tensor as `_native.DevicePackSet(space=TSFA_DEVICE)` takes a key column."""
    code, np_dtype = _VALUE_TYPES[str(t.dtype)]
    return t.data_ptr(), code, np_dtype


def _pack_set(ids, sort, kinds, device):
    """The columns (contiguous, on `device`) sorted once by (kind, id, sort) where they lie -> `_native.DevicePackSet`."""
    return _native.DevicePackSet(_key_column(ids), None if sort is None else _key_column(sort),
                                 None if kinds is None else _key_column(kinds), device=device, space=_native.TSFA_DEVICE,
                                 n_rows=int(ids.shape[0]))


class _DeviceArray:
    """n elements of a numpy dtype at a device pointer, as `torch.as_tensor` reads an array that already lives in HBM."""

    def __init__(self, ptr, n, dtype, owner):
        self.owner = owner
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": np.dtype(dtype).str, "data": (int(ptr), False),
                                         "version": 2, "strides": None}


_SIGNED = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}


def _ids_tensor(torch, pack, dtype, device):
    """The unique ids of a pack as a tensor of `dtype` on the device: a copy made in HBM from the pack's own buffer
    (`tsfa_pack_device_ids`), read as the signed type of its width and viewed back."""
    raw = _DeviceArray(pack.ids_ptr, pack.n_series, _SIGNED[np.dtype(pack.ids_dtype).itemsize], pack)
    return torch.as_tensor(raw, device="cuda:%d" % device).clone().view(dtype)


def _order_key(torch, t):
    """ids -> int64 keys that sort like them (torch sorts and searches signed types): the value itself, for uint64 the bit
    pattern with the top bit flipped."""
    if str(t.dtype) == "torch.uint64":
        return t.view(torch.int64) ^ (-2 ** 63)
    return t.to(torch.int64)


def _from_order_key(torch, key, dtype):
    if str(dtype) == "torch.uint64":
        return (key ^ (-2 ** 63)).view(dtype)
    return key.to(dtype)


def _union_rows(torch, id_sets, dtype):
    """The ascending id sets of the kinds -> (ids_out: their ascending union, rows: None when every kind holds every id of
    the union in the same rows, else per kind the rows of the union its series go to)."""
    first = id_sets[0]
    if all(s.shape[0] == first.shape[0] for s in id_sets[1:]) and all(bool(torch.equal(s, first)) for s in id_sets[1:]):
        return first, None
    keys = [_order_key(torch, s) for s in id_sets]
    union = torch.unique(torch.cat(keys))   # (sorted)
    return _from_order_key(torch, union, dtype), [torch.searchsorted(union, k) for k in keys]


def extract_features_long_tensor(ids, values, sort=None, kinds=None, kind_names=None, times=None, time_unit="ns",
                                 default_fc_parameters=None, kind_to_fc_parameters=None, device=None, check_nan=True,
                                 show_warnings=False):
    """Extract features from a frame held as column tensors, rows in any order; the feature matrix stays on the GPU.

    :param ids: `[N]` tensor or numpy array of an integer dtype: the id of every row.  bool, float and string ids raise
        `TypeError` (factorize them first).
    :param values: the WIDE form (`kinds=None`): `[N]` or `[N, C]`, float32, float64, bool or an integer dtype, any strides
        torch can hold -- a row-major matrix, a column-major one, sliced and expanded views are read in place.  The
        equivalent frame has the columns id, sort and C value columns named `kind_names` (default "0" ... "C-1").  The
        LONG form (`kinds` given): `[N]`; the equivalent frame has `column_kind` holding the names and `column_value`.
        float32 stays float32, float64 stays float64, everything else becomes float64 as `astype(float64)` does.
    :param sort: None, or `[N]` integer / float32 / float64 sort keys.  Rows with equal keys keep their order (the sort is
        stable); with None the order inside an id is the row order, as for a frame without `column_sort`.
    :param kinds: None, or `[N]` integer kind codes.  Kinds may have different id sets.
    :param kind_names: wide form: C names.  Long form: a mapping or a sequence from code to name (default `str(code)`; None in a
        sequence: no name); a code that occurs and has no name raises `ValueError`.
    :param times: None, or `[N]` row-aligned stamps, as `extract_features_tensor` takes them: int64 ticks counted in
        `time_unit`, numpy `datetime64[ns|us|ms|s]`, or float64 seconds.  This is the frame's `DatetimeIndex`: the plans
        are the timed ones and `linear_trend_timewise` is served, on hours written on the device with pandas' arithmetic.
    :param default_fc_parameters, kind_to_fc_parameters, device, show_warnings: as in `extract_features_tensor`.  Custom
        calculators (callable keys) raise `UnsupportedFeature`.
    :param check_nan: True (default): after the pack, from one read-back, a NaN value raises the reference's
        `ValueError("Column must not contain NaN values: <kind>")`, a NaN in a float `sort` the same error naming `sort`,
        a NaT / NaN stamp `ValueError("times must not contain NaT / NaN")`.  False skips the checks and the read-back.
    :return: `(features, columns, ids_out)`: `features` `torch.float64` `[U, number of columns]` on the device; `columns`
        the names ``"{kind}__{feature}"`` in exactly the order `extract_features` gives for the equivalent frame (the wide
        form's kinds in `kind_names` order, the long form's in the sorted order of their NAMES); `ids_out` `[U]` on the
        device in `ids`' dtype: the ascending union of the ids over the kinds.  Cells of a kind that lacks an id are NaN.
        The values are bit-equal to `extract_features(frame, pack="host")`.

    Host tensors and numpy arrays are moved to `device` with torch.  Ordering: synchronous, like `extract_features_tensor`
    -- the inputs are read after everything queued on torch's current stream has finished, and the results are complete
    when the call returns.

    Memory: the sort's scratch is 40 bytes per row while the call runs (more than 2^32 - 1 rows raise `ValueError`); the
    packed samples are one more copy of `values` in its output type.

    Not offered: `nan_policy="drop"`, a rolled twin, an enqueue-only mode, string or float ids.  Not mirrored, as in
    `extract_features_tensor`: the reference's exceptions that depend on the samples.
    """
    import torch

    from tsfresh_amd.feature_extraction import extraction

    ids, values, sort, kinds, names, times, default_fc_parameters, device = _long_arguments(
        torch, ids, values, sort, kinds, kind_names, times, time_unit, default_fc_parameters, kind_to_fc_parameters, device)
    N, wide, timed = int(ids.shape[0]), kinds is None, times is not None
    id_dtype = ids.dtype

    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("default" if show_warnings else "ignore")
        pins = set()
        jobs = None
        if wide:   # the kinds are known: a settings object the kernels do not serve fails before anything moves
            jobs = _kind_jobs(names, default_fc_parameters, kind_to_fc_parameters, device, pins, _INSTEAD, timed=timed)
        ids = _to_device(ids, device).contiguous()
        values = _to_device(values, device)
        sort = None if sort is None else _to_device(sort, device).contiguous()
        hours = flag = None
        if timed:
            stamps = _to_device(times[0], device)
            hours = torch.empty(N, dtype=torch.float64, device=ids.device)
            flag = torch.zeros(1, dtype=torch.int32, device=ids.device)
        if wide:
            v2 = values if values.ndim == 2 else values.unsqueeze(1)
        else:
            kinds = _to_device(kinds, device).contiguous()
            values = values.contiguous()
        _synchronize(torch, device)   # the producers of the columns, the copies and the fill of the flag word are done

        pack_set = _pack_set(ids, sort, kinds, device)
        packs = []
        try:
            if wide:
                packs = pack_set.rows(v2.data_ptr(), _VALUE_TYPES[str(v2.dtype)][0], v2.shape[1], v2.stride(0), v2.stride(1))
                kind_of = list(names)
            else:
                packs = pack_set.values((values.data_ptr(), _VALUE_TYPES[str(values.dtype)][0]))
                kind_of = [names(int(code)) for code in pack_set.kinds]
                missing = [int(code) for code, name in zip(pack_set.kinds, kind_of) if name is None]
                if missing:
                    raise ValueError("kind code {} has no name in kind_names".format(missing[0]))
            if timed:
                pack_set.hours(stamps.data_ptr(), times[1], times[2], stamps.stride(0), hours.data_ptr(), flag.data_ptr())
            if check_nan:
                _raise_for_nan(torch, packs, kind_of, values, kinds, pack_set, sort, flag)

            # the frame's column order: a wide frame's kinds as given, a long frame's in the sorted order of their names
            order = list(range(len(packs))) if wide else sorted(range(len(packs)), key=lambda k: kind_of[k])
            if jobs is None:
                jobs = _kind_jobs([kind_of[k] for k in order], default_fc_parameters, kind_to_fc_parameters, device, pins,
                                  _INSTEAD, timed=timed)
            jobs, n_cols, columns = jobs
            row0 = np.concatenate([[0], np.cumsum([p.n_rows for p in packs])]) if not wide else np.zeros(len(packs) + 1, dtype=np.int64)

            id_sets = [_ids_tensor(torch, packs[0], id_dtype, device)] if wide else \
                [_ids_tensor(torch, pack, id_dtype, device) for pack in packs]
            ids_out, rows = _union_rows(torch, id_sets, id_dtype)
            U = int(ids_out.shape[0])
            if rows is None:
                features = torch.empty((U, n_cols), dtype=torch.float64, device=ids.device)
            else:
                features = torch.full((U, n_cols), float("nan"), dtype=torch.float64, device=ids.device)
            _synchronize(torch, device)   # (the fill, and whatever the allocator's memory was last used for)
            matrix = _native.BorrowedMatrix(features.data_ptr(), U, n_cols, device, owner=features) if n_cols else None
            for c, kind, fplan, nplan, col0 in jobs:
                k = order[c]
                pack = packs[k]
                timed_kw = {} if hours is None else {"times_ptr": hours.data_ptr() + 8 * int(row0[k])}
                if rows is None:
                    # (one native call per kind: the calls are synchronous, the plan's own stream runs the kernels)
                    nplan.extract_into(None, None, matrix, col0=col0, pack=pack, **timed_kw)
                    continue
                width = len(fplan.names)
                block = torch.empty((pack.n_series, width), dtype=torch.float64, device=ids.device)
                _synchronize(torch, device)
                nplan.extract_into(None, None, _native.BorrowedMatrix(block.data_ptr(), pack.n_series, width, device, owner=block),
                                   col0=0, pack=pack, **timed_kw)
                features[rows[k], col0:col0 + width] = block   # the device row scatter
            _synchronize(torch, device)
        finally:
            for pack in packs:
                pack.close()
            pack_set.close()
        extraction._trim_cache(extraction._thread_cache())
    return features, columns, ids_out


def _raise_for_nan(torch, packs, kind_of, values, kinds, pack_set, sort, flag):
    """The errors of `check_nan=True`.  The value columns' flags came back with the pack; the sort column's NaN test and the
    hours' flag word come back in ONE read."""
    if any(pack.value_nan for pack in packs):
        if kinds is None:
            bad = next(k for k, pack in enumerate(packs) if pack.value_nan)
        else:   # the long form's packs share one flag: find the first kind that holds the NaN (only on the way to the error)
            codes = torch.unique(kinds[torch.isnan(values)]).tolist()
            bad = min(k for k, code in enumerate(pack_set.kinds) if int(code) in codes)
        raise ValueError("Column must not contain NaN values: {}".format(kind_of[bad]))
    words = []
    if sort is not None and sort.is_floating_point():
        words.append(torch.isnan(sort).any().reshape(1).to(torch.int32))
    if flag is not None:
        words.append(flag)
    if not words:
        return
    read = torch.cat(words).tolist()   # one read-back
    if sort is not None and sort.is_floating_point() and read[0]:
        raise ValueError("Column must not contain NaN values: sort")
    if flag is not None and read[-1] & _native.TSFA_DENSE_BAD_TIME:
        raise ValueError("times must not contain NaT / NaN")
