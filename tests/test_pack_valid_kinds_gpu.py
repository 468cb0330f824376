"""tsfa_pack_dense_valid_kinds on the device against the rule stated in numpy: a boolean keep mask per (series, kind), the
kept samples concatenated, `np.cumsum` of the kept counts for every kind's offsets.  One batch holds a series of every
length on a round edge (of 64 steps, and of the 128, 256 and 512 a 16-byte load per lane would make) and on the chunk edge; values, offsets, step indices, kept stamps and the flag word
are compared exactly, and every output cell beyond what a kind keeps must still hold its sentinel."""
import numpy as np
import pytest
import torch

from tsfresh_amd import _native

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LENGTHS = np.array([1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049], dtype=np.int64)
B, N = len(LENGTHS), 2056                      # rows of 2056 samples start on 16 bytes in every element type
NAT = np.iinfo(np.int64).min
SENTINEL = -77
# dtype -> (tsfa_dtype, storage bits, two NaN patterns that are not the canonical one, bits -> float64)
DTYPES = {
    "float64": (_native.TSFA_F64, np.uint64, (0x7ff8000000000001, 0xfff0000000000001), lambda u: u.view(np.float64)),
    "float32": (_native.TSFA_F32, np.uint32, (0x7fc00001, 0xff800001), lambda u: u.view(np.float32).astype(np.float64)),
    "float16": (_native.TSFA_F16, np.uint16, (0x7e01, 0xfc01), lambda u: u.view(np.float16).astype(np.float64)),
    "bfloat16": (_native.TSFA_BF16, np.uint16, (0x7fc1, 0xff81), lambda u: (u.astype(np.uint32) << 16).view(np.float32).astype(np.float64)),
}
# layout -> (storage elements, offset of x[0, 0, 0], element strides) of a (B, C, N) view
LAYOUTS = {
    "bcn": lambda C: (B * C * N, 0, (C * N, N, 1)),                          # rows that start on 16 bytes
    "offset": lambda C: (B * C * (N + 1), 1, (C * (N + 1), N + 1, 1)),       # x[..., 1:]: rows that do not
    "channels_last": lambda C: (B * N * C, 0, (N * C, 1, C)),
    "stepped": lambda C: (B * C * 2 * N, 0, (2 * C * N, 2 * N, 2)),          # x[..., ::2]
}
PATTERNS = ("all", "alternate", "first", "last", "edge64", "empty_kind", "beyond", "nat", "bad_length")
TIMED = ("alternate", "last", "nat")


def _case(pattern, C):
    """-> (drop: (B, C, N) bool, the samples to make NaN; lengths as passed; stamps (B, N) or None)."""
    t = np.arange(N)[None, None, :]
    c = np.arange(C)[None, :, None]
    last = (LENGTHS - 1)[:, None, None]
    drop = np.zeros((B, C, N), dtype=bool)
    lengths = LENGTHS.copy()
    if pattern == "alternate":
        drop |= ((t + c) % 2 == 1) & (t > 0)                       # phase-shifted per kind; step 0 stays, so no pair is emptied
    elif pattern == "first":
        drop |= t > 0
    elif pattern == "last":
        drop |= t != last
    elif pattern == "edge64":
        drop |= (t >= 992) & (t < 1056)                            # across the chunk edge at 1024
    elif pattern == "empty_kind":
        drop[5, C - 1, :] = True                                   # the other kinds of series 5 are intact
    elif pattern == "beyond":
        drop |= t > last                                           # never read
    elif pattern == "bad_length":
        lengths[[2, 4]] = 0, N + 5
    stamps = None
    if pattern in TIMED:
        stamps = 10 ** 18 + np.cumsum(np.full((B, N), 10 ** 9, dtype=np.int64), axis=1)
        if pattern == "nat":
            stamps[:, 3::7] = NAT                                  # the values of these steps are fine
    return drop, lengths, stamps


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", (1, 3))
def test_packer_equals_the_numpy_rule(gpu, C, dtype, layout, pattern):
    x_type, bits, nans, to_f64 = DTYPES[dtype]
    rng = np.random.default_rng(5)
    drop, lengths, stamps = _case(pattern, C)
    x = rng.standard_normal((B, C, N)).astype(np.float32)
    x[0, 0, 0], x[13, C - 1, 1] = np.inf, -np.inf                  # values: they stay
    u = {"float64": lambda: x.astype(np.float64).view(np.uint64), "float32": lambda: x.view(np.uint32),
         "float16": lambda: x.astype(np.float16).view(np.uint16), "bfloat16": lambda: (x.view(np.uint32) >> 16).astype(np.uint16)}[dtype]()
    u = np.where(drop, np.where(np.arange(N) % 2 == 0, bits(nans[0]), bits(nans[1])), u).astype(bits)
    size, off, strides = LAYOUTS[layout](C)
    storage = np.full(size, nans[0], dtype=bits)                   # what lies between the samples is NaN
    np.lib.stride_tricks.as_strided(storage[off:], (B, C, N), tuple(s * storage.itemsize for s in strides))[...] = u

    # the rule, in float64
    clamped = np.clip(lengths, 0, N)
    keep = ~drop & (np.arange(N)[None, None, :] < clamped[:, None, None])
    if stamps is not None:
        keep &= (stamps != NAT)[:, None, :]
    counts = keep.sum(axis=2).T                                                       # (C, B)
    want_offsets = np.concatenate([np.zeros((C, 1), dtype=np.int64), np.cumsum(counts, axis=1)], axis=1)
    want_flags = (_native.TSFA_DENSE_BAD_LENGTH if ((lengths < 1) | (lengths > N)).any() else 0) | \
        (_native.TSFA_DENSE_EMPTY_SERIES if (counts == 0).any() else 0)
    assert bool(want_flags & _native.TSFA_DENSE_EMPTY_SERIES) == (pattern in ("empty_kind", "bad_length"))

    xd = torch.from_numpy(storage.view({8: np.int64, 4: np.int32, 2: np.int16}[storage.itemsize])).to(DEV)
    od = torch.float64 if dtype == "float64" else torch.float32
    values = torch.full((C, B * N), SENTINEL, dtype=od, device=DEV)
    offsets = torch.full((C, B + 1), SENTINEL, dtype=torch.int64, device=DEV)
    steps = torch.full((C, B * N), SENTINEL, dtype=torch.int32, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    nbytes = _native.pack_dense_valid_scratch_bytes(B * C, N)
    scratch = torch.empty(nbytes // 8, dtype=torch.int64, device=DEV)
    lengths_d = torch.from_numpy(lengths).to(DEV)
    kw, kept_stamps = {}, None
    if stamps is not None:
        td = torch.from_numpy(stamps).to(DEV)
        kept_stamps = torch.full((C, B, N), SENTINEL, dtype=torch.int64, device=DEV)
        kw = dict(t_ptr=td.data_ptr(), t_type=_native.TSFA_I64, t_strides=(N, 1), stamps_ptr=kept_stamps.data_ptr())
    torch.cuda.synchronize()
    _native.pack_dense_valid_kinds(xd.data_ptr() + off * xd.element_size(), x_type, (B, C, N), strides, values.data_ptr(), B * N,
                                   offsets.data_ptr(), steps.data_ptr(), scratch.data_ptr(), nbytes, flag.data_ptr(), device=0,
                                   lengths_ptr=lengths_d.data_ptr(), lengths_type=_native.TSFA_I64, **kw)
    assert int(flag.item()) == want_flags
    assert np.array_equal(offsets.cpu().numpy(), want_offsets)
    with np.errstate(invalid="ignore"):   # (widening a signalling NaN)
        values, steps, x64 = values.cpu().numpy().astype(np.float64), steps.cpu().numpy(), to_f64(u)
    for c in range(C):
        T = int(want_offsets[c, -1])
        assert np.array_equal(values[c, :T], x64[:, c][keep[:, c]])
        assert np.array_equal(steps[c, :T], np.nonzero(keep[:, c])[1])
        assert (values[c, T:] == SENTINEL).all() and (steps[c, T:] == SENTINEL).all()   # the padding is untouched
        if kept_stamps is not None:
            got = kept_stamps[c].cpu().numpy()
            inside = np.arange(N)[None, :] < counts[c][:, None]
            assert np.array_equal(got[inside], np.broadcast_to(stamps, keep[:, c].shape)[keep[:, c]])
            assert (got[~inside] == SENTINEL).all()
