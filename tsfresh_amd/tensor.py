"""`extract_features_tensor` and `extract_rolled_features_tensor`: features of a batch that already is a tensor, without pandas.

`extract_features` takes the reference's containers: a batch held as `[B, C, n]`, `[B, n, C]` or a right-padded `[B, n_max]`
with `lengths[B]` on the GPU would have to be copied to the host, written out as a DataFrame and sorted back into the layout
it already had.  Here the tensor goes to the dense packer (`tsfa_pack_dense`: one fused copy / transpose / convert kernel,
include/tsfresh_amd.h) and from there to the kernels `extract_features` runs, through the same FCParameters handling, the
same plan cache and the same composite plans (feature_extraction/extraction.py); the feature matrix stays on the device.
The rolled entry adds the window builder between the two (`tsfa_roll_count` / `tsfa_roll_fill` on the packer's offsets) and
hands the kernels `(start, end)` views instead of whole series (`tsfa_extract_windows` with device pointers).
With `times=` the batch brings its clock as an array: `tsfa_pack_times` writes the hours since each series' first stamp next
to the packed samples, and the plans hold the `linear_trend_timewise` columns a frame with a `DatetimeIndex` gets.
"""
import numpy as np

from tsfresh_amd import _native

# torch dtype name -> tsfa_dtype (the names are compared as strings: torch is imported inside the function)
_X_TYPES = {"torch.float64": _native.TSFA_F64, "torch.float32": _native.TSFA_F32, "torch.float16": _native.TSFA_F16,
            "torch.bfloat16": _native.TSFA_BF16}


def _to_device(t, device):
    """`t` on HIP device `device` (torch calls it cuda:<device>); a tensor that is there already is returned as it is."""
    if t.is_cuda and t.device.index == device:
        return t
    return t.to("cuda:%d" % device)


def _synchronize(torch, device):
    """Wait for everything queued on torch's current stream of `device`."""
    torch.cuda.current_stream(device).synchronize()


def _pack_outputs(torch, x3, lengths, device):
    """What `_dense_pack` and `_valid_pack` both make for a (B, C, n) tensor on `device` -> (tsfa_dtype of x3, values, offsets,
    flag, lengths pointer, lengths type, views).  values: (C, B * n) float64 or float32, offsets: B + 1 int64, flag: one
    zeroed int32 -- torch allocations made here, before the caller's `_synchronize`.  views(): after the library call, one
    `_native.DensePack` per channel; they keep the three buffers, x3 and lengths alive."""
    B, C, n = x3.shape
    x_type = _X_TYPES[str(x3.dtype)]
    vtype = _native.TSFA_F64 if x_type == _native.TSFA_F64 else _native.TSFA_F32
    values = torch.empty((C, B * n), dtype=torch.float64 if vtype == _native.TSFA_F64 else torch.float32, device=x3.device)
    offsets = torch.empty(B + 1, dtype=torch.int64, device=x3.device)
    flag = torch.zeros(1, dtype=torch.int32, device=x3.device)
    lptr, ltype = None, 0
    if lengths is not None:
        lptr, ltype = lengths.data_ptr(), (_native.TSFA_I32 if lengths.dtype == torch.int32 else _native.TSFA_I64)

    def views():
        owner = (values, offsets, flag, x3, lengths)
        return [_native.DensePack(values.data_ptr() + c * B * n * values.element_size(), vtype, offsets.data_ptr(), B, device,
                                  owner=owner) for c in range(C)]
    return x_type, values, offsets, flag, lptr, ltype, views


def _dense_pack(torch, x3, lengths, device):
    """(B, C, n) tensor on `device` -> ([one `_native.DensePack` per channel], flag tensor of one int32).  The packed
    samples, the offsets and the flag word are torch allocations the packs keep alive."""
    B, C, n = x3.shape
    x_type, values, offsets, flag, lptr, ltype, views = _pack_outputs(torch, x3, lengths, device)
    _synchronize(torch, device)   # the producer of x, and the fill of the flag word, are done before another stream reads
    _native.pack_dense(x3.data_ptr(), x_type, (B, C, n), x3.stride(), values.data_ptr(), B * n, offsets.data_ptr(),
                       flag.data_ptr(), device=device, lengths_ptr=lptr, lengths_type=ltype)
    return views(), flag


# time_unit -> ticks per second (numpy's datetime64 units of the same names)
_TIME_UNITS = {"s": 1, "ms": 10 ** 3, "us": 10 ** 6, "ns": 10 ** 9}


def _times_argument(torch, times, time_unit, B, n):
    """The checks on `times` -> (stamps: an int64 or float64 tensor of shape (n,) or (B, n), tsfa_dtype, ticks per second).
    Nothing has moved to the device yet."""
    tps = None
    if isinstance(times, np.ndarray):
        if times.dtype.kind == "M":
            unit, count = np.datetime_data(times.dtype)
            if unit not in _TIME_UNITS or count != 1:
                raise TypeError("times must be datetime64[ns], [us], [ms] or [s], int64 ticks or float64 seconds, not {}".format(
                    times.dtype))
            tps = _TIME_UNITS[unit]   # the dtype names the unit: time_unit is not looked at
            times = times.view(np.int64)
        if times.dtype not in (np.int64, np.float64):
            raise TypeError("times must be int64 ticks, datetime64 or float64 seconds, not {}".format(times.dtype))
        if any(s < 0 for s in times.strides) or not times.dtype.isnative:
            times = np.ascontiguousarray(times, dtype=times.dtype.newbyteorder("="))
        times = torch.from_numpy(times)
    if not isinstance(times, torch.Tensor):
        raise TypeError("times must be a torch.Tensor or a numpy array, not {}".format(type(times).__name__))
    if times.dtype not in (torch.int64, torch.float64):
        raise TypeError("times must be int64 ticks, datetime64 or float64 seconds, not {}".format(times.dtype))
    if times.dtype == torch.float64:
        t_type, tps = _native.TSFA_F64, 1
    else:
        t_type = _native.TSFA_I64
        if tps is None:
            if time_unit not in _TIME_UNITS:
                raise ValueError("time_unit must be one of 'ns', 'us', 'ms', 's': got {!r}".format(time_unit))
            tps = _TIME_UNITS[time_unit]
    if tuple(times.shape) not in ((n,), (B, n)):
        raise ValueError("times must have shape ({n},) (one clock for the batch) or ({B}, {n}) (one per series): got {got}".format(
            n=n, B=B, got=tuple(times.shape)))
    return times, t_type, tps


def _times_pack(torch, times, pack, flag, device):
    """The hours of the batch's clock in the layout of `pack` (one channel of `_dense_pack`'s result; the channels share
    their offsets) -> a float64 tensor the caller keeps alive while the kernels read it.  times: what `_times_argument`
    returned, on `device` and of logical shape (B, n).  ORs TSFA_DENSE_BAD_TIME into the pack's flag word.  Runs after `_dense_pack`'s
    synchronisation, on the library's stream, and returns when the hours are written."""
    t, t_type, tps = times
    B, n = t.shape
    hours = torch.empty(B * n, dtype=torch.float64, device=t.device)   # [0, T) is written, T <= B * n
    _native.pack_times(t.data_ptr(), t_type, tps, (B, n), t.stride(), pack.offsets_ptr, hours.data_ptr(), flag.data_ptr(),
                       device=device)
    return hours


def _batch_arguments(torch, x, lengths, kinds, channels_last, default_fc_parameters, kind_to_fc_parameters, device):
    """The checks both entries make on their batch -> (x3: the (B, C, n) view of x, lengths: None or a contiguous int32 /
    int64 tensor, kinds, default_fc_parameters, device).  Nothing has moved to the device yet."""
    from tsfresh_amd.feature_extraction import extraction
    from tsfresh_amd.feature_extraction.data import _check_colname
    from tsfresh_amd.feature_extraction.settings import ComprehensiveFCParameters

    if isinstance(x, np.ndarray):
        if x.dtype not in (np.float64, np.float32, np.float16):
            raise TypeError("x must be float64, float32, float16 or bfloat16, not {}".format(x.dtype))
        x = torch.from_numpy(x)
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch.Tensor or a numpy array, not {}".format(type(x).__name__))
    if str(x.dtype) not in _X_TYPES:
        raise TypeError("x must be float64, float32, float16 or bfloat16, not {}".format(x.dtype))
    if x.ndim == 2:
        x3 = x.unsqueeze(1)
    elif x.ndim == 3:
        x3 = x.permute(0, 2, 1) if channels_last else x
    else:
        raise ValueError("x must have shape (B, n), (B, C, n) or, with channels_last=True, (B, n, C): got {} dimensions".format(x.ndim))
    B, C, n = x3.shape
    if B < 1 or C < 1 or n < 1:
        raise ValueError("x must hold at least one series, one kind and one sample: got shape {}".format(tuple(x.shape)))
    if lengths is not None:
        if isinstance(lengths, np.ndarray):
            lengths = torch.from_numpy(np.ascontiguousarray(lengths))
        if not isinstance(lengths, torch.Tensor):
            lengths = torch.as_tensor(lengths)
        if lengths.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
            raise TypeError("lengths must be integers, not {}".format(lengths.dtype))
        if lengths.ndim != 1 or lengths.shape[0] != B:
            raise ValueError("lengths must be one-dimensional with one entry per series ({}): got shape {}".format(
                B, tuple(lengths.shape)))
        if lengths.dtype != torch.int32:
            lengths = lengths.to(torch.int64)
        lengths = lengths.contiguous()
    kinds = [str(c) for c in range(C)] if kinds is None else [str(k) for k in kinds]
    if len(kinds) != C:
        raise ValueError("kinds must name the {} kinds of x: got {} names".format(C, len(kinds)))
    if len(set(kinds)) != C:
        raise ValueError("kinds must be distinct")
    _check_colname(*kinds)

    if default_fc_parameters is None and kind_to_fc_parameters is None:
        default_fc_parameters = ComprehensiveFCParameters()
    elif default_fc_parameters is None:
        default_fc_parameters = {}
    if device is None:
        device = x.device.index if x.is_cuda else extraction._default_device()
    return x3, lengths, kinds, default_fc_parameters, int(device)


def _kind_jobs(kinds, default_fc_parameters, kind_to_fc_parameters, device, pins, instead, timed=False):
    """The plans of the kinds that have columns -> ([(channel, kind, fplan, native plan, first column)], number of columns,
    column names).  A settings object the kernels do not serve, or a box without a device, fails here, before anything
    moves.  instead: what the UnsupportedFeature of a callable calculator tells the caller to do.  timed: the batch brings
    its clock, so the plans keep linear_trend_timewise as those of a frame with a DatetimeIndex do."""
    from tsfresh_amd.feature_extraction import extraction
    from tsfresh_amd.feature_extraction.plan import compile_fc_parameters
    from tsfresh_amd.feature_extraction.registry import UnsupportedFeature

    plan_cache, jobs, n_cols = {}, [], 0
    for c, kind in enumerate(kinds):
        fc_parameters = kind_to_fc_parameters[kind] if kind_to_fc_parameters and kind in kind_to_fc_parameters \
            else default_fc_parameters
        key = id(fc_parameters)
        if key not in plan_cache:
            fplan = compile_fc_parameters(fc_parameters, has_datetime_index=bool(timed))
            if fplan.host_calls:
                raise UnsupportedFeature("custom (callable) calculators are evaluated per series on the host: " + instead)
            plan_cache[key] = (fplan, extraction._acquire_plan(fplan, device, pins) if fplan.names else None)
        fplan, nplan = plan_cache[key]
        if nplan is None:
            continue
        jobs.append((c, kind, fplan, nplan, n_cols))
        n_cols += len(fplan.names)
    columns = [kind + "__" + name for _, kind, fplan, _, _ in jobs for name in fplan.names]
    return jobs, n_cols, columns


def _batch_to_device(x3, lengths, times, device):
    """The head of `_pack_checked` and `_pack_dropped`: x3, lengths and the stamps of `times` (None, or what
    `_times_argument` returned) on `device` -> (x3, lengths, times), the stamps of logical shape (B, n)."""
    x3 = _to_device(x3, device)
    if lengths is not None:
        lengths = _to_device(lengths, device)
    if times is not None:
        t = _to_device(times[0], device)   # (before the pack: its synchronisation covers the copy)
        if t.ndim == 1:
            t = t.unsqueeze(0).expand(x3.shape[0], x3.shape[2])   # one clock for the batch: batch stride 0, n stamps on the device
        times = (t,) + tuple(times[1:])
    return x3, lengths, times


def _pack_checked(torch, x3, lengths, kinds, device, check_nan, want_steps=False, times=None):
    """`_dense_pack` of the batch on `device` and its flag word's errors -> (x3 and lengths on the device, packs, steps,
    hours).  steps (want_steps): the longest series, n without lengths -- with lengths their maximum, which comes back in
    the same read as the flag word.  times: None or what `_times_argument` returned; hours: None or `_times_pack`'s tensor,
    whose flag bit travels in the same word."""
    n = x3.shape[2]
    x3, lengths, times = _batch_to_device(x3, lengths, times, device)
    packs, flag = _dense_pack(torch, x3, lengths, device)
    hours = _times_pack(torch, times, packs[0], flag, device) if times is not None else None
    steps = n
    if lengths is not None or check_nan:
        if want_steps and lengths is not None:
            # one read for both words, before any extraction kernel is launched
            flags, steps = torch.stack([flag.reshape(()).to(torch.int64), lengths.max().to(torch.int64)]).tolist()
        else:
            flags = int(flag.item())   # one word back, before any extraction kernel is launched
        if flags & _native.TSFA_DENSE_BAD_LENGTH:
            raise ValueError("lengths must lie in [1, {}] (the samples per series of x)".format(n))
        if check_nan and flags & _native.TSFA_PACK_VALUE_NAN:
            raise ValueError("Column must not contain NaN values: {}".format(_first_nan_kind(torch, x3, lengths, kinds)))
        if check_nan and flags & _native.TSFA_DENSE_BAD_TIME:
            raise ValueError("times must not contain NaT / NaN")
    return x3, lengths, packs, int(steps), hours


_NAN_POLICIES = ("raise", "drop")


def _check_nan_policy(nan_policy):
    if nan_policy not in _NAN_POLICIES:
        raise ValueError("nan_policy must be one of 'raise', 'drop': got {!r}".format(nan_policy))
    return nan_policy == "drop"


def _valid_pack(torch, x3, lengths, times, device):
    """(B, C, n) tensor on `device` without the steps a wide frame loses to `dropna()` (`tsfa_pack_dense_valid`: a step of a
    series goes for every kind when any kind's sample is NaN, or its stamp NaT / NaN) -> ([one `_native.DensePack` per
    channel], flag tensor of one int32, hours, steps, offsets).  times: None or what `_times_argument` returned, on
    `device` and of logical shape (B, n).  hours: None, or `tsfa_pack_times`' float64 tensor for the kept stamps (hours since
    each series' first kept stamp).  steps: int32 tensor over the packed layout, the original step index of every kept
    sample.  offsets: the int64 tensor of B + 1 offsets the channels share.  The buffers are torch allocations the packs
    keep alive."""
    B, C, n = x3.shape
    x_type, values, offsets, flag, lptr, ltype, views = _pack_outputs(torch, x3, lengths, device)
    steps = torch.empty(B * n, dtype=torch.int32, device=x3.device)   # [0, T) is written, T <= B * n
    scratch_bytes = _native.pack_dense_valid_scratch_bytes(B, n)
    scratch = torch.empty(scratch_bytes // 8, dtype=torch.int64, device=x3.device)
    timed, stamps = {}, None
    if times is not None:
        t, t_type, tps = times
        stamps = torch.empty((B, n), dtype=t.dtype, device=x3.device)
        timed = dict(t_ptr=t.data_ptr(), t_type=t_type, t_strides=t.stride(), stamps_ptr=stamps.data_ptr())
    _synchronize(torch, device)   # the producer of x, and the fill of the flag word, are done before another stream reads
    _native.pack_dense_valid(x3.data_ptr(), x_type, (B, C, n), x3.stride(), values.data_ptr(), B * n, offsets.data_ptr(),
                             steps.data_ptr(), scratch.data_ptr(), scratch_bytes, flag.data_ptr(), device=device,
                             lengths_ptr=lptr, lengths_type=ltype, **timed)
    hours = None
    if times is not None:
        # the kept stamps are a right-padded (B, n) batch with the new offsets: the times packer's own arithmetic
        hours = torch.empty(B * n, dtype=torch.float64, device=x3.device)
        _native.pack_times(stamps.data_ptr(), t_type, tps, (B, n), (n, 1), offsets.data_ptr(), hours.data_ptr(), flag.data_ptr(),
                           device=device)
    return views(), flag, hours, steps, offsets


def _pack_dropped(torch, x3, lengths, device, want_steps=False, times=None):
    """`_valid_pack` of the batch on `device` and its flag word's errors -> (x3 on the device, packs, the longest kept length
    (want_steps; it comes back in the same read as the flag word), hours, steps).  The flag word is always read: a length
    outside [1, n] and a series without a kept step are errors whatever `check_nan` says."""
    n = x3.shape[2]
    x3, lengths, times = _batch_to_device(x3, lengths, times, device)
    packs, flag, hours, steps, offsets = _valid_pack(torch, x3, lengths, times, device)
    longest = n
    if want_steps:
        # one read for both words, before any extraction kernel is launched
        flags, longest = torch.stack([flag.reshape(()).to(torch.int64), (offsets[1:] - offsets[:-1]).max()]).tolist()
    else:
        flags = int(flag.item())
    if flags & _native.TSFA_DENSE_BAD_LENGTH:
        raise ValueError("lengths must lie in [1, {}] (the samples per series of x)".format(n))
    if flags & _native.TSFA_DENSE_EMPTY_SERIES:
        empty = int(torch.nonzero(offsets[1:] == offsets[:-1])[0].item())
        raise ValueError("series {} has no step left after nan_policy='drop': every step holds a NaN sample{}".format(
            empty, "" if times is None else " or a NaT / NaN stamp"))
    return x3, packs, int(longest), hours, steps


def extract_features_tensor(x, lengths=None, kinds=None, channels_last=False, default_fc_parameters=None,
                            kind_to_fc_parameters=None, device=None, check_nan=True, show_warnings=False, nan_policy="raise",
                            times=None, time_unit="ns"):
    """Extract features from a batch of equally sampled series held as a tensor; the feature matrix stays on the GPU.

    :param x: `torch.Tensor` (on the GPU or on the CPU) or numpy array of dtype float64, float32, float16 or bfloat16 and
        shape `(B, n)` (one kind), `(B, C, n)`, or `(B, n, C)` with `channels_last=True`: B series of n samples for each of C
        kinds.  Any strides are taken as they are (sliced, stepped, permuted and expanded views are not copied first).  A CPU
        tensor or a numpy array is moved to `device` with torch.  float16 and bfloat16 samples are converted to float32
        (exactly) on the way into the packed layout, and the result equals that of the float32 samples.
    :param lengths: optional 1-D integer tensor or array of B entries: series b is its first `lengths[b]` samples (a
        right-padded batch), 1 <= lengths[b] <= n.  What lies beyond a series' length is never read.
    :param kinds: C names, default "0" ... "C-1"; the rules of a wide frame's value columns apply (no "__", no trailing "_").
    :param default_fc_parameters, kind_to_fc_parameters: as in `extract_features` (default `ComprehensiveFCParameters()`).
        Custom calculators (callable keys) are evaluated on the host per series and raise `UnsupportedFeature` here.
    :param device: HIP device ordinal.  Default: the device `x` lives on; for a CPU tensor or an array the rule of
        `extract_features` ($TSFRESH_AMD_DEVICE, else $LOCAL_RANK, else 0).
    :param check_nan: True (default): a NaN among the samples raises the reference's
        `ValueError("Column must not contain NaN values: <kind>")`; False skips the check and its read-back of one word.
    :param nan_policy: "raise" (default): the behaviour above, under either value of `check_nan`.  "drop": the result is
        what the call returns for the equivalent wide frame after `dropna()`: step t of series b is dropped for every kind
        when any kind's sample `x[b, :, t]` is NaN and, with `times`, when its stamp is NaT (`INT64_MIN`) or NaN
        (`tsfa_pack_dense_valid` compacts the batch on the device; the hours count from each series' first kept stamp).
        +-inf is a value and stays.  Steps at or beyond `lengths[b]` are never read.  `check_nan` is irrelevant: nothing that
        is NaN reaches the kernels, and the one flag word is always read -- a series with no kept step has no row in that
        frame and raises `ValueError` with its batch index.  Anything else raises `ValueError`.  Not offered: a
        user-supplied validity mask, per-kind lengths (a kind dropping steps on its own), the frame entries (use
        `frame.dropna()`), an enqueue-only mode.
    :param times: optional time stamps of the samples, for an irregularly sampled batch: a `torch.Tensor` or numpy array of
        shape `(n,)` (one clock for the batch) or `(B, n)` (one per series), any strides (expanded and stepped views are not
        copied first); the kinds share the clock, as the value columns of a frame share its index.  dtype int64 (ticks,
        counted in `time_unit`), numpy `datetime64[ns|us|ms|s]` (the unit comes from the dtype) or float64 seconds; anything
        else raises `TypeError` (float32 seconds lack the precision).  A CPU tensor or an array is moved to `device` with
        torch.  With `times` the plans are those of a frame with a `DatetimeIndex`: `linear_trend_timewise` is served (788
        columns per kind under `ComprehensiveFCParameters` instead of 783), regressing on the hours since each series'
        first stamp, which `tsfa_pack_times` writes on the device with pandas' arithmetic (bit-equal to `extract_features`
        on the frame that carries the same stamps as its index).  Stamps beyond a series' length are never read.  With
        `check_nan=True` a NaT (`INT64_MIN`) or NaN stamp inside a length raises
        `ValueError("times must not contain NaT / NaN")` (the same read-back of one word); with `check_nan=False` the
        hours of that sample -- of the whole series, when it is its first stamp -- are NaN.
    :param time_unit: "ns" (default), "us", "ms" or "s": what one tick of an int64 `times` counts.
    :return: `(features, columns)`: a `torch.float64` tensor `[B, number of columns]` on the device and the list of column
        names ``"{kind}__{feature}"``, in exactly the order `extract_features` gives for the equivalent wide frame.

    Ordering (this version is synchronous): `x` is read only after everything queued on torch's current stream at the time of
    the call has finished -- the call synchronises with that stream explicitly, because the library's streams do not
    synchronise with it implicitly -- and when the call returns `features` is complete and safe to use on any stream.
    Enqueue-only operation on the caller's stream is a follow-up.

    Not mirrored: the reference's exceptions that depend on the samples -- an infinite sample under `binned_entropy` or
    `ar_coefficient`, a `query_similarity_count` query longer than a series (feature_extraction/reference_errors.py raises
    them for `extract_features`).  Finding them needs the samples on the host; here those cells hold the kernels' NaN.
    """
    import torch

    from tsfresh_amd.feature_extraction import extraction

    drop = _check_nan_policy(nan_policy)
    x3, lengths, kinds, default_fc_parameters, device = _batch_arguments(
        torch, x, lengths, kinds, channels_last, default_fc_parameters, kind_to_fc_parameters, device)
    B = x3.shape[0]
    if times is not None:
        times = _times_argument(torch, times, time_unit, B, x3.shape[2])

    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("default" if show_warnings else "ignore")
        pins = set()
        jobs, n_cols, columns = _kind_jobs(kinds, default_fc_parameters, kind_to_fc_parameters, device, pins,
                                           "build a DataFrame and call extract_features on it", timed=times is not None)
        x3 = _to_device(x3, device)
        features = torch.empty((B, n_cols), dtype=torch.float64, device=x3.device)
        if drop:
            x3, packs, _, hours, _ = _pack_dropped(torch, x3, lengths, device, times=times)
        else:
            x3, lengths, packs, _, hours = _pack_checked(torch, x3, lengths, kinds, device, check_nan, times=times)
        if n_cols:
            matrix = _native.BorrowedMatrix(features.data_ptr(), B, n_cols, device, owner=features)
            timed = {} if hours is None else {"times_ptr": hours.data_ptr()}
            for c, kind, fplan, nplan, col0 in jobs:
                # (one native call per kind: the calls are synchronous, the plan's own stream runs the kernels)
                nplan.extract_into(None, None, matrix, col0=col0, pack=packs[c], **timed)
        for pack in packs:
            pack.close()
        extraction._trim_cache(extraction._thread_cache())
    return features, columns


def _roll_windows(torch, pack, series_len, rolling_direction, max_timeshift, min_timeshift, steps):
    """The rolled windows of a dense-packed batch, built on the device from the offsets its channels share -> (starts, ends,
    series, timeshifts): four int64 tensors of n_windows entries on the pack's device, in (series, ascending timeshift)
    order; starts / ends index every channel's own value buffer.  series_len: the samples of every series of a batch
    without `lengths` (the closed form: one launch, nothing read back), or None for a ragged batch (count, scan, fill: the
    window count comes back).  With no window nothing is launched."""
    dev = "cuda:%d" % pack.device
    B = pack.n_series
    roll = dict(rolling_direction=rolling_direction, max_timeshift=max_timeshift, min_timeshift=min_timeshift, steps=steps,
                device=pack.device)
    scanned = None
    if series_len is None:
        scanned = torch.empty(B, dtype=torch.int32, device=dev)   # (uint32 to the library: 4 bytes per series)
        roll["scanned_ptr"] = scanned.data_ptr()
        _synchronize(torch, pack.device)   # (the allocator may hand out memory that work queued on torch's stream still uses)
    else:
        roll["series_len"] = series_len
    n_windows = _native.roll_count(pack.offsets_ptr, B, **roll)
    out = torch.empty((4, n_windows), dtype=torch.int64, device=dev)
    _synchronize(torch, pack.device)
    _native.roll_fill(pack.offsets_ptr, B, n_windows, *(out[k].data_ptr() for k in range(4)), **roll)
    return out[0], out[1], out[2], out[3]


def extract_rolled_features_tensor(x, lengths=None, kinds=None, channels_last=False, rolling_direction=1, max_timeshift=None,
                                   min_timeshift=0, default_fc_parameters=None, kind_to_fc_parameters=None, device=None,
                                   check_nan=True, show_warnings=False, nan_policy="raise", times=None, time_unit="ns"):
    """`extract_rolled_features` for a batch that already is a tensor: sliding-window (forecasting) features of every series,
    without pandas; the windows are built in HBM and the feature matrix stays there.

    :param x, lengths, kinds, channels_last, default_fc_parameters, kind_to_fc_parameters, device, check_nan: exactly as in
        `extract_features_tensor`.  Custom calculators (callable keys) raise `UnsupportedFeature` here as well.
    :param rolling_direction, max_timeshift, min_timeshift: as in `roll_time_series` / `extract_rolled_features`; the
        reference's three `ValueError`s for them are raised before anything moves.  A window of w samples at every step is
        `max_timeshift=w - 1, min_timeshift=w - 1`.
    :param times, time_unit: as in `extract_features_tensor`.  The hours are written once for the batch; the kernel rebases
        them on each window's first stamp, as the reference does for the rolled frame.
    :param nan_policy: as in `extract_features_tensor`.  With "drop" the windows are rolled over the KEPT steps of every
        series (the result of `extract_rolled_features` on the wide frame after `dropna()`, its sort column the step
        index): they come from the ragged route (count, scan, fill on the compacted offsets; the longest kept length comes
        back with the flag word), and `positions` holds ORIGINAL step indices -- of the window's last kept step for a
        positive direction, of its first for a negative one -- gathered on the device from the packer's step array.  The
        same things are not offered (a validity mask, per-kind lengths, the frame entries, an enqueue-only mode).
    :return: `(features, columns, series, positions)`, all tensors on the device:
        `features` `torch.float64` `[n_windows, number of columns]`; `columns` the names ``"{kind}__{feature}"`` in exactly the
        order `extract_rolled_features` gives for the equivalent wide frame; `series` `torch.int64` `[n_windows]`, the batch
        index of each window; `positions` `torch.int64` `[n_windows]`, `timeshift - 1`: the second half of the reference's
        window id `(id, shift)` when the sort column is `0 .. len - 1` -- the index of the window's last sample for a positive
        direction, of its first sample for a negative one.  Rows are in `(series, ascending position)` order, the sorted order
        of the reference's `(id, shift)` index for integer ids.  For a batch without `lengths` every series has the same
        windows, so `features.view(B, n_windows // B, -1)` is the dense `[B, W, F]` form.  With no window at all (for example
        `min_timeshift` at or above every length) the tensors are empty, of shapes `(0, number of columns)` and `(0,)`, and
        nothing is launched.

    The windows are built once for all kinds (the channels share their offsets): for a batch without `lengths` in one launch
    from a closed form, with nothing read back; with `lengths` the longest length comes back with the packer's flag word
    (`ts = steps (mod |rolling_direction|)` decides the shifts, so the true maximum is needed) and the window count after a
    count and a scan.

    Memory: the result matrix is allocated whole, `n_windows * number of columns * 8` bytes, and is the caller's to budget.
    1000 series of 1024 samples at window 128 are 1000 * (1024 - 127) = 897 000 windows: with the 777 columns of
    `EfficientFCParameters` 5.58 GB, next to 4 * 8 bytes per window of starts, ends, series and positions (28.7 MB).  Roll a
    slice of the batch at a time when that is too much.

    Ordering: synchronous, like `extract_features_tensor` -- `x` is read after everything queued on torch's current stream
    has finished, and the results are complete when the call returns.

    Not mirrored, as in `extract_features_tensor`: the reference's exceptions that depend on the samples (an infinite sample
    under `binned_entropy` or `ar_coefficient`, a `query_similarity_count` query longer than a window); those cells hold the
    kernels' NaN.
    """
    import torch

    from tsfresh_amd.feature_extraction import extraction
    from tsfresh_amd.utilities.dataframe_functions import check_roll_arguments

    check_roll_arguments(rolling_direction, max_timeshift, min_timeshift)
    drop = _check_nan_policy(nan_policy)
    x3, lengths, kinds, default_fc_parameters, device = _batch_arguments(
        torch, x, lengths, kinds, channels_last, default_fc_parameters, kind_to_fc_parameters, device)
    n = x3.shape[2]
    if times is not None:
        times = _times_argument(torch, times, time_unit, x3.shape[0], n)

    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("default" if show_warnings else "ignore")
        pins = set()
        jobs, n_cols, columns = _kind_jobs(kinds, default_fc_parameters, kind_to_fc_parameters, device, pins,
                                           "build a DataFrame, roll it with roll_time_series and call extract_features on it",
                                           timed=times is not None)
        kept_steps = None
        if drop:
            # the kept lengths are ragged whatever `lengths` is: the count / scan / fill route on the new offsets
            x3, packs, steps, hours, kept_steps = _pack_dropped(torch, x3, lengths, device, want_steps=True, times=times)
            series_len = None
        else:
            x3, lengths, packs, steps, hours = _pack_checked(torch, x3, lengths, kinds, device, check_nan, want_steps=True,
                                                             times=times)
            series_len = n if lengths is None else None
        # once for all kinds: the channels share their offsets, and starts / ends count from each channel's own base
        starts, ends, series, shifts = _roll_windows(torch, packs[0], series_len, int(rolling_direction),
                                                     max_timeshift, int(min_timeshift), steps)
        n_windows = int(series.shape[0])
        features = torch.empty((n_windows, n_cols), dtype=torch.float64, device=x3.device)
        if n_windows and n_cols:
            matrix = _native.BorrowedMatrix(features.data_ptr(), n_windows, n_cols, device, owner=features)
            _synchronize(torch, device)
            timed = {} if hours is None else {"times_ptr": hours.data_ptr()}
            for c, kind, fplan, nplan, col0 in jobs:
                nplan.extract_windows_into(packs[c].values_ptr, packs[c].values_type, starts.data_ptr(), ends.data_ptr(),
                                           n_windows, matrix, col0=col0, **timed)
        if kept_steps is None:
            positions = shifts - 1
        else:
            # the original step index of the sample that names the window: one gather on the device
            named = ends - 1 if rolling_direction > 0 else starts
            positions = kept_steps[named].to(torch.int64)
        _synchronize(torch, device)
        for pack in packs:
            pack.close()
        extraction._trim_cache(extraction._thread_cache())
    return features, columns, series, positions


def _first_nan_kind(torch, x3, lengths, kinds):
    """The first kind that holds a NaN inside its series' lengths (only on the way to the ValueError)."""
    nan = torch.isnan(x3)
    if lengths is not None:
        inside = torch.arange(x3.shape[2], device=x3.device)[None, :] < lengths[:, None]
        nan = nan & inside[:, None, :]
    per_kind = nan.any(dim=2).any(dim=0).tolist()
    return next((k for k, bad in zip(kinds, per_kind) if bad), kinds[0])
