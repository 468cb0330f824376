"""tsfa_pack_dense_valid on the device against its emulation (tests/emul_pack_valid_lib.py), compared exactly: the grid of
tests/test_pack_valid_emul.py -- every validity pattern at every series length, layout and element type, with and without
stamps -- values, offsets, original step indices, kept stamps, hours and flags, with sentinel cells around every buffer.  This
is what the emulation cannot see: the hardware ballot and the prefix below a lane, the rounds of a work item split over four
wavefronts, the barriers around the count's LDS words, the 1024-thread scan with its carry, and a launch whose work items
outnumber its workgroups.  The emulation itself is held against numpy's dropna and pandas' hours by the emulation test."""
import numpy as np
import pytest
import torch

import emul_pack_valid_lib as epv
import pack_valid_cases as pvc
from tsfresh_amd import _native

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
X_TYPES = {"float64": _native.TSFA_F64, "float32": _native.TSFA_F32, "float16": _native.TSFA_F16, "bfloat16": _native.TSFA_BF16}
TORCH_BITS = {"float64": torch.int64, "float32": torch.int32, "float16": torch.int16, "bfloat16": torch.int16}
TPS = {"s": 1, "ms": 10 ** 3, "us": 10 ** 6, "ns": 10 ** 9}
VALUE_SENTINEL, STEP_SENTINEL, STAMP_SENTINEL, OFFSET_SENTINEL, HOURS_SENTINEL = -777.25, -77, -5555555555, -12345, -7.25


def _signed(base):
    return base.view({8: np.int64, 4: np.int32, 2: np.int16}[base.itemsize])


class Packed:
    """One tsfa_pack_dense_valid call (and tsfa_pack_times on its stamps) on the device copy of a case's storage, through the
    same strides."""

    def __init__(self, case, unit="ns", flags=0):
        B, C, n = case.shape
        xb = torch.from_numpy(_signed(case.x_base)).to(DEV)             # the storage as bit patterns: no conversion on the way
        x_ptr = xb.data_ptr() + case.x_off * xb.element_size()
        od = torch.float64 if case.dtype == "float64" else torch.float32
        cso = B * n
        raw = torch.full((C * cso + 2 * GUARD,), VALUE_SENTINEL, dtype=od, device=DEV)
        offs = torch.full((B + 1 + 2 * GUARD,), OFFSET_SENTINEL, dtype=torch.int64, device=DEV)
        steps = torch.full((cso + 2 * GUARD,), STEP_SENTINEL, dtype=torch.int32, device=DEV)
        word = torch.tensor([0, flags, 0], dtype=torch.int32, device=DEV)
        nbytes = _native.pack_dense_valid_scratch_bytes(B, n)
        scratch = torch.empty(nbytes // 8 + 2 * GUARD, dtype=torch.int64, device=DEV).fill_(OFFSET_SENTINEL)
        kw = {}
        if case.lengths is not None:
            lengths = torch.from_numpy(case.lengths).to(DEV)
            kw.update(lengths_ptr=lengths.data_ptr(), lengths_type=_native.TSFA_I64)
        stamps = None
        if case.t_base is not None:
            tb = torch.from_numpy(case.t_base).to(DEV)
            stamps = torch.full((B * n + 2 * GUARD,), STAMP_SENTINEL, dtype=torch.int64, device=DEV)
            kw.update(t_ptr=tb.data_ptr() + 8 * case.t_off, t_type=_native.TSFA_I64, t_strides=case.t_strides,
                      stamps_ptr=stamps.data_ptr() + 8 * GUARD)
        torch.cuda.synchronize()
        _native.pack_dense_valid(x_ptr, X_TYPES[case.dtype], (B, C, n), case.x_strides, raw.data_ptr() + GUARD * raw.element_size(), cso,
                                 offs.data_ptr() + 8 * GUARD, steps.data_ptr() + 4 * GUARD, scratch.data_ptr() + 8 * GUARD, nbytes,
                                 word.data_ptr() + 4, device=0, **kw)
        self.offsets = offs[GUARD:GUARD + B + 1].cpu().numpy()
        T = int(self.offsets[-1])
        body = raw[GUARD:GUARD + C * cso].view(C, cso)
        self.values = body[:, :T].cpu().numpy()
        self.steps = steps[GUARD:GUARD + T].cpu().numpy()
        ok = ((raw[:GUARD] == VALUE_SENTINEL).all() and (raw[GUARD + C * cso:] == VALUE_SENTINEL).all() and (body[:, T:] == VALUE_SENTINEL).all()
              and (offs[:GUARD] == OFFSET_SENTINEL).all() and (offs[GUARD + B + 1:] == OFFSET_SENTINEL).all()
              and (steps[:GUARD] == STEP_SENTINEL).all() and (steps[GUARD + T:] == STEP_SENTINEL).all()
              and (scratch[:GUARD] == OFFSET_SENTINEL).all() and (scratch[-GUARD:] == OFFSET_SENTINEL).all())
        self.stamps = self.hours = None
        if stamps is not None:
            kept = torch.from_numpy(np.diff(self.offsets)).to(DEV)
            rows = stamps[GUARD:GUARD + B * n].view(B, n)
            beyond = torch.arange(n, device=DEV)[None, :] >= kept[:, None]
            ok = ok and (stamps[:GUARD] == STAMP_SENTINEL).all() and (stamps[GUARD + B * n:] == STAMP_SENTINEL).all() \
                and (rows[beyond] == STAMP_SENTINEL).all()
            self.stamps = rows.cpu().numpy()
            hours = torch.full((cso + 2 * GUARD,), HOURS_SENTINEL, dtype=torch.float64, device=DEV)
            torch.cuda.synchronize()
            _native.pack_times(rows.data_ptr(), _native.TSFA_I64, TPS[unit], (B, n), (n, 1), offs.data_ptr() + 8 * GUARD,
                               hours.data_ptr() + 8 * GUARD, word.data_ptr() + 4, device=0)
            ok = ok and (hours[:GUARD] == HOURS_SENTINEL).all() and (hours[GUARD + T:] == HOURS_SENTINEL).all()
            self.hours = hours[GUARD:GUARD + T].cpu().numpy()
        word = word.cpu().numpy()
        self.flags = int(word[1])
        self.guards_intact = bool(ok) and word[0] == 0 and word[2] == 0


def _emulated(case, unit="ns"):
    return epv.EmulValid(case.x_view(), lengths=case.lengths, t=case.t_view(), unit=unit, bf16=case.dtype == "bfloat16")


def _check(case, unit="ns", flags=0):
    want = _emulated(case, unit)
    got = Packed(case, unit)
    assert want.status == 0 and want.guards_intact and got.guards_intact, case.name
    assert got.flags == want.flags == flags, case.name
    assert np.array_equal(got.offsets, want.offsets), case.name
    assert np.array_equal(got.steps, want.steps), case.name
    assert pvc.same_bits(got.values, want.values), case.name
    if want.stamps is not None:
        kept = np.diff(want.offsets)
        inside = np.arange(case.shape[2])[None, :] < kept[:, None]
        assert np.array_equal(got.stamps[inside], want.stamps[inside]), case.name
        assert pvc.same_bits(got.hours, want.hours), case.name
    return got


@pytest.mark.parametrize("layout", pvc.LAYOUTS)
@pytest.mark.parametrize("dtype", pvc.DTYPES)
def test_every_pattern_at_every_length(gpu, dtype, layout):
    assert epv.row_chunk() == pvc.CHUNK
    for n in pvc.N_GRID:
        _check(pvc.make_case(dtype, layout, n, with_stamps=False))
        _check(pvc.make_case(dtype, layout, n, with_stamps=True))


@pytest.mark.parametrize("unit", pvc.UNITS)
def test_hours_in_every_unit(gpu, unit):
    for layout in ("bcn", "stepped", "expanded"):
        _check(pvc.make_case("float32", layout, 1025, with_stamps=True, unit=unit), unit=unit)


@pytest.mark.parametrize("dtype", ("float32", "bfloat16"))
def test_many_series_carry_the_scan_and_stride_the_grid(gpu, dtype):
    """70 000 work items: more than the 65 536 workgroups of a launch and more than the 4096 entries of one trip of the scan."""
    case = pvc.many_series_case(dtype)
    got = _check(case)
    values, offsets, steps, _ = pvc.dropna_reference(case)
    assert np.array_equal(got.offsets, offsets) and np.array_equal(got.steps, steps) and pvc.same_bits(got.values, values)


def test_the_flags_and_the_clamping(gpu):
    n = 1025
    for layout in ("bcn", "cl3", "stepped"):
        case = pvc.make_case("float32", layout, n, with_stamps=True)
        good = case.lengths.copy()
        for bad, pos in ((0, 0), (-3, 4), (n + 1, 7), (2 ** 40, 4)):
            case.lengths = good.copy()
            case.lengths[pos] = bad
            _check(case, flags=_native.TSFA_DENSE_BAD_LENGTH | (_native.TSFA_DENSE_EMPTY_SERIES if bad <= 0 else 0))
        case.lengths = good
    # an empty series alone: every step of series 3 holds a NaN in one kind
    case = pvc.make_case("float64", "bcn", 65, with_stamps=False)
    x = case.logical().copy()
    x[3, 1, :] = x[6, 0, -1]                              # (a NaN of the padding)
    case.x_base, case.x_off, case.x_strides = x.reshape(-1), 0, (3 * 65, 65, 1)
    got = _check(case, flags=_native.TSFA_DENSE_EMPTY_SERIES)
    assert np.flatnonzero(np.diff(got.offsets) == 0).tolist() == [3]
    # the bits are ORed into what the word held
    assert Packed(case, flags=_native.TSFA_PACK_IN_ORDER).flags == _native.TSFA_PACK_IN_ORDER | _native.TSFA_DENSE_EMPTY_SERIES


def test_refused_arguments(gpu):
    buf = torch.zeros(8 * 128, dtype=torch.int64, device=DEV)
    x, out, offs, steps_, scr, flag, p, q = (buf.data_ptr() + 1024 * k for k in range(8))   # eight regions of 1 KiB, none shared

    def call(x_type=_native.TSFA_F32, shape=(2, 3, 4), strides=(12, 4, 1), cso=8, scratch=scr, nbytes=2 * 200, steps=steps_, device=0, **kw):
        _native.pack_dense_valid(x, x_type, shape, strides, out, cso, offs, steps, scratch, nbytes, flag, device=device, **kw)
    call()
    assert buf[256:259].tolist() == [0, 4, 8] and int(buf[640]) == 0
    call(t_ptr=p, t_type=_native.TSFA_I64, t_strides=(4, 1), stamps_ptr=q)
    for kw, code in ((dict(x_type=_native.TSFA_I32), _native.TSFA_ERR_INVALID), (dict(strides=(12, -4, 1)), _native.TSFA_ERR_INVALID),
                     (dict(shape=(2, 0, 4)), _native.TSFA_ERR_INVALID), (dict(cso=7), _native.TSFA_ERR_INVALID),
                     (dict(nbytes=2 * 200 - 1), _native.TSFA_ERR_INVALID), (dict(scratch=scr + 4), _native.TSFA_ERR_INVALID),
                     (dict(scratch=0), _native.TSFA_ERR_INVALID),
                     (dict(t_ptr=p, t_type=_native.TSFA_I64, t_strides=(4, 1)), _native.TSFA_ERR_INVALID),   # no stamps_ptr
                     (dict(t_ptr=p, t_type=_native.TSFA_F32, t_strides=(4, 1), stamps_ptr=p), _native.TSFA_ERR_INVALID),
                     (dict(shape=(1, 1, 33554432), strides=(0, 0, 0), cso=33554432, nbytes=2 ** 40), _native.TSFA_ERR_TOO_LONG),
                     (dict(device=4096), _native.TSFA_ERR_NO_DEVICE)):
        with pytest.raises(_native.NativeError) as ei:
            call(**kw)
        assert ei.value.code == code, kw
