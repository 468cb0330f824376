"""`extract_features_tensor`: features of a batch that already is a tensor, without pandas.

`extract_features` takes the reference's containers: a batch held as `[B, C, n]`, `[B, n, C]` or a right-padded `[B, n_max]`
with `lengths[B]` on the GPU would have to be copied to the host, written out as a DataFrame and sorted back into the layout
it already had.  Here the tensor goes to the dense packer (`tsfa_pack_dense`: one fused copy / transpose / convert kernel,
include/tsfresh_amd.h) and from there to the kernels `extract_features` runs, through the same FCParameters handling, the
same plan cache and the same composite plans (feature_extraction/extraction.py); the feature matrix stays on the device.
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


def _dense_pack(torch, x3, lengths, device):
    """(B, C, n) tensor on `device` -> ([one `_native.DensePack` per channel], flag tensor of one int32).  The packed
    samples, the offsets and the flag word are torch allocations the packs keep alive."""
    B, C, n = x3.shape
    x_type = _X_TYPES[str(x3.dtype)]
    out_dtype = torch.float64 if x_type == _native.TSFA_F64 else torch.float32
    values = torch.empty((C, B * n), dtype=out_dtype, device=x3.device)
    offsets = torch.empty(B + 1, dtype=torch.int64, device=x3.device)
    flag = torch.zeros(1, dtype=torch.int32, device=x3.device)
    _synchronize(torch, device)   # the producer of x, and the fill of the flag word, are done before another stream reads
    lptr, ltype = None, 0
    if lengths is not None:
        lptr, ltype = lengths.data_ptr(), (_native.TSFA_I32 if lengths.dtype == torch.int32 else _native.TSFA_I64)
    _native.pack_dense(x3.data_ptr(), x_type, (B, C, n), x3.stride(), values.data_ptr(), B * n, offsets.data_ptr(),
                       flag.data_ptr(), device=device, lengths_ptr=lptr, lengths_type=ltype)
    owner = (values, offsets, flag, x3, lengths)
    vtype = _native.TSFA_F64 if x_type == _native.TSFA_F64 else _native.TSFA_F32
    packs = [_native.DensePack(values.data_ptr() + c * B * n * values.element_size(), vtype, offsets.data_ptr(), B, device,
                               owner=owner) for c in range(C)]
    return packs, flag


def extract_features_tensor(x, lengths=None, kinds=None, channels_last=False, default_fc_parameters=None,
                            kind_to_fc_parameters=None, device=None, check_nan=True, show_warnings=False):
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
    from tsfresh_amd.feature_extraction.data import _check_colname
    from tsfresh_amd.feature_extraction.plan import compile_fc_parameters
    from tsfresh_amd.feature_extraction.registry import UnsupportedFeature
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
    device = int(device)

    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("default" if show_warnings else "ignore")
        # plans first: a settings object the kernels do not serve, or a box without a device, fails before anything moves
        plan_cache, pins, jobs, n_cols = {}, set(), [], 0
        for c, kind in enumerate(kinds):
            fc_parameters = kind_to_fc_parameters[kind] if kind_to_fc_parameters and kind in kind_to_fc_parameters \
                else default_fc_parameters
            key = id(fc_parameters)
            if key not in plan_cache:
                fplan = compile_fc_parameters(fc_parameters, has_datetime_index=False)
                if fplan.host_calls:
                    raise UnsupportedFeature("custom (callable) calculators are evaluated per series on the host: build a "
                                             "DataFrame and call extract_features on it")
                plan_cache[key] = (fplan, extraction._acquire_plan(fplan, device, pins) if fplan.names else None)
            fplan, nplan = plan_cache[key]
            if nplan is None:
                continue
            jobs.append((c, kind, fplan, nplan, n_cols))
            n_cols += len(fplan.names)
        columns = [kind + "__" + name for _, kind, fplan, _, _ in jobs for name in fplan.names]

        x3 = _to_device(x3, device)
        if lengths is not None:
            lengths = _to_device(lengths, device)
        features = torch.empty((B, n_cols), dtype=torch.float64, device=x3.device)
        packs, flag = _dense_pack(torch, x3, lengths, device)
        if lengths is not None or check_nan:
            flags = int(flag.item())   # one word back, before any extraction kernel is launched
            if flags & _native.TSFA_DENSE_BAD_LENGTH:
                raise ValueError("lengths must lie in [1, {}] (the samples per series of x)".format(n))
            if check_nan and flags & _native.TSFA_PACK_VALUE_NAN:
                raise ValueError("Column must not contain NaN values: {}".format(_first_nan_kind(torch, x3, lengths, kinds)))
        if n_cols:
            matrix = _native.BorrowedMatrix(features.data_ptr(), B, n_cols, device, owner=features)
            for c, kind, fplan, nplan, col0 in jobs:
                # (one native call per kind: the calls are synchronous, the plan's own stream runs the kernels)
                nplan.extract_into(None, None, matrix, col0=col0, pack=packs[c])
        for pack in packs:
            pack.close()
        extraction._trim_cache(extraction._thread_cache())
    return features, columns


def _first_nan_kind(torch, x3, lengths, kinds):
    """The first kind that holds a NaN inside its series' lengths (only on the way to the ValueError)."""
    nan = torch.isnan(x3)
    if lengths is not None:
        inside = torch.arange(x3.shape[2], device=x3.device)[None, :] < lengths[:, None]
        nan = nan & inside[:, None, :]
    per_kind = nan.any(dim=2).any(dim=0).tolist()
    return next((k for k, bad in zip(kinds, per_kind) if bad), kinds[0])
