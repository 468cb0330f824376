"""Test helper: the batches of the valid-step packer's grid (tsfa_pack_dense_valid), shared by the emulation test and the GPU
test, and the numpy statement of `dropna()` both are compared with.

A case is a batch whose series carry one validity pattern each, so one call covers every pattern at one series length,
layout and element type.  Storage is described as (flat base array, element offset, shape, element strides), so that numpy
and torch build the SAME strided view of it.

TEST INFRASTRUCTURE ONLY.  The product never imports this.
"""
import numpy as np

NAT = np.iinfo(np.int64).min
CHUNK = 1024                     # steps of one work item (asserted against the emulation's constant by the tests)
N_GRID = (1, 63, 64, 65, 1023, 1024, 1025, 2049)
DTYPES = ("float64", "float32", "float16", "bfloat16")
LAYOUTS = ("bcn", "cl3", "cl33", "stepped", "expanded")
PATTERNS = ("all kept", "every other", "only first", "only last", "run of 64 across the chunk edge", "last channel only",
            "beyond the length", "NaT stamp")
UNITS = ("ns", "us", "ms", "s")

# NaN bit patterns that are NOT the canonical quiet NaN of their type (two per type, either sign)
_NANS = {"float64": (0x7ff0000000000001, 0xfff8000000000123), "float32": (0x7f800001, 0xffc00055),
         "float16": (0x7c01, 0xfe05), "bfloat16": (0x7f81, 0xffc3)}
_BITS = {"float64": np.uint64, "float32": np.uint32, "float16": np.uint16, "bfloat16": np.uint16}


def channels_of(layout):
    return {"bcn": 3, "cl3": 3, "cl33": 33, "stepped": 2, "expanded": 3}[layout]


def to_bits(values32, dtype):
    """float32 values -> the bit patterns of `dtype` (bfloat16: the upper half, truncated)."""
    if dtype == "float64":
        return values32.astype(np.float64).view(np.uint64)
    if dtype == "float32":
        return values32.view(np.uint32)
    if dtype == "float16":
        return values32.astype(np.float16).view(np.uint16)
    return (values32.view(np.uint32) >> 16).astype(np.uint16)


def from_bits(bits, dtype):
    """The bit patterns of `dtype` -> the values in the packer's output dtype (float64 stays, the others become float32)."""
    if dtype == "float64":
        return bits.view(np.float64)
    if dtype == "float32":
        return bits.view(np.float32)
    if dtype == "float16":
        return bits.view(np.float16).astype(np.float32)   # exact; NaN payloads are not compared (no NaN is kept)
    return (bits.astype(np.uint32) << 16).view(np.float32)


class Case:
    """x_base / x_off / x_strides: the storage of the (B, C, n) batch as bit patterns (`as_view`); lengths: int64[B] or
    None; t_base / t_off / t_strides: the storage of the (B, n) int64 stamps, or None; logical: the (B, C, n) bit patterns
    as a plain array; stamps: the (B, n) stamps as a plain array."""

    def __init__(self, name, dtype, shape, x_base, x_off, x_strides, lengths, t_base=None, t_off=0, t_strides=None):
        self.name, self.dtype, self.shape = name, dtype, shape
        self.x_base, self.x_off, self.x_strides = x_base, x_off, x_strides
        self.lengths = lengths
        self.t_base, self.t_off, self.t_strides = t_base, t_off, t_strides

    def x_view(self):
        """The strided numpy view the emulation takes (float16 / float64 / float32 as floats, bfloat16 as uint16)."""
        v = as_view(self.x_base, self.x_off, self.shape, self.x_strides)
        return v if self.dtype == "bfloat16" else v.view({"float64": np.float64, "float32": np.float32, "float16": np.float16}[self.dtype])

    def t_view(self):
        return None if self.t_base is None else as_view(self.t_base, self.t_off, (self.shape[0], self.shape[2]), self.t_strides)

    def logical(self):
        return np.ascontiguousarray(as_view(self.x_base, self.x_off, self.shape, self.x_strides))

    def stamps(self):
        return None if self.t_base is None else np.ascontiguousarray(self.t_view())


def as_view(base, off, shape, strides):
    return np.lib.stride_tricks.as_strided(base[off:], shape=shape, strides=tuple(s * base.itemsize for s in strides), writeable=False)


def _lay_out(bits, layout, nan):
    """The (B, C, n) bit patterns in the storage of `layout` -> (base, offset, element strides).  Cells the view does not
    own hold NaN, so a load outside the view would show."""
    B, C, n = bits.shape
    if layout == "bcn":
        return bits.reshape(-1).copy(), 0, (C * n, n, 1)
    if layout in ("cl3", "cl33"):
        return np.ascontiguousarray(bits.transpose(0, 2, 1)).reshape(-1), 0, (n * C, 1, C)
    if layout == "stepped":
        big = np.full((B, C, 3 * n + 2), nan, dtype=bits.dtype)
        big[:, :, 2:2 + 3 * n:3] = bits
        return big.reshape(-1), 2, (C * (3 * n + 2), 3 * n + 2, 3)
    assert layout == "expanded" and (bits == bits[:, :1, :]).all()
    return bits[:, 0, :].reshape(-1).copy(), 0, (n, 0, 1)


def make_case(dtype, layout, n, with_stamps, unit="ns", seed=0):
    """One batch of len(PATTERNS) series of up to n steps, one pattern per series."""
    rng = np.random.default_rng(seed * 1000003 + n * 131 + LAYOUTS.index(layout) * 17 + DTYPES.index(dtype))
    B, C = len(PATTERNS), channels_of(layout)
    vals = rng.standard_normal((B, C, n)).astype(np.float32) * 37.0
    vals[rng.random((B, C, n)) < 0.02] = np.inf        # a value: kept
    vals[rng.random((B, C, n)) < 0.02] = -np.inf
    if layout == "expanded":
        vals[:] = vals[:, :1, :]
    bits = to_bits(vals, dtype)
    nans = np.array(_NANS[dtype], dtype=_BITS[dtype])
    lengths = np.full(B, n, dtype=np.int64)
    lengths[6] = max(1, n - n // 3)
    drop = np.zeros((B, C, n), dtype=bool)
    t = np.arange(n)
    drop[1, t % C, t] = (t % 2 == 1)
    drop[2, 0, 1:] = True
    drop[3, C - 1, :n - 1] = True
    run = (t >= CHUNK - 30) & (t < CHUNK + 34)
    drop[4, 0, run] = True
    drop[5, C - 1, 1:] = rng.random(n - 1) < 0.3
    drop[6, :, lengths[6]:] = True                      # padding: never read
    if layout == "expanded":
        drop[:] = drop.any(axis=1, keepdims=True)
    bits = np.where(drop, nans[rng.integers(0, 2, size=drop.shape)], bits)
    if layout == "expanded":
        bits[:] = bits[:, :1, :]
    x_base, x_off, x_strides = _lay_out(bits, layout, nans[0])
    case = Case("%s %s n=%d%s" % (dtype, layout, n, " stamps" if with_stamps else ""), dtype, (B, C, n), x_base, x_off, x_strides, lengths)
    if with_stamps:
        tps = {"s": 1, "ms": 10 ** 3, "us": 10 ** 6, "ns": 10 ** 9}[unit]
        stamps = 1_600_000_000 * tps + np.cumsum(rng.integers(1, 7_000 * tps + 1, size=(B, n)), axis=1)
        missing = rng.random(n - 1) < 0.25
        if layout == "expanded":
            missing[-1:] = False                          # (the shared clock: the series that keeps only its last step keeps it)
        stamps[7, 1:][missing] = NAT
        stamps[6, lengths[6]:] = NAT
        if layout == "expanded":                          # one clock for the batch: batch stride 0
            case.t_base, case.t_off, case.t_strides = stamps[7].copy(), 0, (0, 1)
        elif layout == "stepped":
            big = np.full((B, 2 * n + 1), NAT, dtype=np.int64)
            big[:, 1::2] = stamps
            case.t_base, case.t_off, case.t_strides = big.reshape(-1), 1, (2 * n + 1, 2)
        else:
            case.t_base, case.t_off, case.t_strides = stamps.reshape(-1).copy(), 0, (n, 1)
    return case


def many_series_case(dtype, B=70000, n=3, seed=5):
    """More work items than a launch has workgroups, and more scanned entries than one trip of the scan takes."""
    rng = np.random.default_rng(seed)
    vals = rng.standard_normal((B, 1, n)).astype(np.float32)
    bits = to_bits(vals, dtype)
    drop = rng.random((B, 1, n)) < 0.3
    drop[:, :, 0] = False
    bits = np.where(drop, np.array(_NANS[dtype][1], dtype=_BITS[dtype]), bits)
    lengths = rng.integers(1, n + 1, size=B).astype(np.int64)
    return Case("%s many series" % dtype, dtype, (B, 1, n), bits.reshape(-1).copy(), 0, (n, 0, 1), lengths)


def dropna_reference(case):
    """What the wide frame of the batch holds after dropna(), in the packer's layout -> (values [C, T] in the output dtype,
    offsets int64[B + 1], steps int32[T], kept stamps int64[T] or None)."""
    bits = case.logical()
    B, C, n = bits.shape
    x = from_bits(bits.reshape(-1), case.dtype).reshape(B, C, n)
    lengths = np.full(B, n) if case.lengths is None else np.clip(case.lengths, 0, n)
    keep = (np.arange(n)[None, :] < lengths[:, None]) & ~np.isnan(x).any(axis=1)
    stamps = case.stamps()
    if stamps is not None:
        keep &= stamps != NAT
    offsets = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    values = np.stack([x[:, c, :][keep] for c in range(C)])
    steps = np.broadcast_to(np.arange(n, dtype=np.int32), (B, n))[keep]
    return values, offsets, steps, None if stamps is None else stamps[keep]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view("u%d" % a.dtype.itemsize), b.view("u%d" % b.dtype.itemsize))
