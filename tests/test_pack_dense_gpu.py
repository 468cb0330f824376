"""tsfa_pack_dense on the device against torch indexing, compared exactly: the grid of tests/test_pack_dense_emul.py (shapes
that straddle the tile edges, the four layouts, the four element types, every form of `lengths`), the three routes, several
channel tiles, more work items than one launch has workgroups, and the two flags with sentinel cells around the buffers."""
import numpy as np
import pytest
import torch

import emul_pack_dense_lib as epd
from tsfresh_amd import _native

pytestmark = pytest.mark.gpu

TC = epd.tile_c()
TT = epd.tile_t(TC)   # (of a full channel tile; fewer channels: epd.tile_t(C), longer)
B_GRID = (1, 3)
C_GRID = (1, 2, 5, TC - 1, TC, TC + 1)
DTYPES = (torch.float64, torch.float32, torch.float16, torch.bfloat16)
LAYOUTS = ("bcn", "bnc", "slice", "expand")
X_TYPES = {torch.float64: _native.TSFA_F64, torch.float32: _native.TSFA_F32, torch.float16: _native.TSFA_F16,
           torch.bfloat16: _native.TSFA_BF16}
GUARD = 64
DEV = "cuda:0"


def _out_dtype(dtype):
    return torch.float64 if dtype == torch.float64 else torch.float32


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _view(gen, layout, B, C, n, dtype):
    def rnd(shape):
        return (torch.randn(shape, generator=gen, device=DEV, dtype=torch.float32) * 37.0).to(dtype)
    if layout == "bcn":
        return rnd((B, C, n))
    if layout == "bnc":
        return rnd((B, n, C)).permute(0, 2, 1)
    if layout == "expand":
        return rnd((1, C, n)).expand(B, C, n)
    big = torch.full((2 * B + 1, C + 2, 3 * n + 2), float("nan"), device=DEV, dtype=dtype)   # a load of a gap would raise the NaN flag
    view = big[1::2, 1:C + 1, 2:2 + 3 * n:3]
    view.copy_(rnd((B, C, n)))
    return view


class Packed:
    def __init__(self, x, lengths=None):
        B, C, n = x.shape
        od = _out_dtype(x.dtype)
        cso = B * n
        sent = -777.25
        raw = torch.full((C * cso + 2 * GUARD,), sent, dtype=od, device=DEV)
        offs = torch.full((B + 1 + 2 * GUARD,), -12345, dtype=torch.int64, device=DEV)
        flags = torch.zeros(3, dtype=torch.int32, device=DEV)
        lptr, ltype = None, 0
        if lengths is not None:
            lptr, ltype = lengths.data_ptr(), (_native.TSFA_I32 if lengths.dtype == torch.int32 else _native.TSFA_I64)
        torch.cuda.synchronize()
        _native.pack_dense(x.data_ptr(), X_TYPES[x.dtype], (B, C, n), x.stride(), raw.data_ptr() + GUARD * raw.element_size(), cso,
                           offs.data_ptr() + 8 * GUARD, flags.data_ptr() + 4, device=0, lengths_ptr=lptr, lengths_type=ltype)
        self.offsets = offs[GUARD:GUARD + B + 1].cpu()
        T = int(self.offsets[-1])
        body = raw[GUARD:GUARD + C * cso].view(C, cso)
        self.values = body[:, :T]
        self.flags = int(flags[1])
        self.guards_intact = bool((raw[:GUARD] == sent).all() and (raw[GUARD + C * cso:] == sent).all() and (body[:, T:] == sent).all()
                                  and (offs[:GUARD] == -12345).all() and (offs[GUARD + B + 1:] == -12345).all()
                                  and flags[0] == 0 and flags[2] == 0)


def _expected(x, lens):
    od = _out_dtype(x.dtype)
    return torch.cat([x[b, :, :int(lens[b])].to(od) for b in range(x.shape[0])], dim=1)


def _check(x, lengths, where):
    lens = [x.shape[2]] * x.shape[0] if lengths is None else lengths.tolist()
    res = Packed(x, lengths)
    assert res.flags == 0, where
    assert res.offsets.tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist(), where
    assert torch.equal(_bits(res.values), _bits(_expected(x, lens))), where
    assert res.guards_intact, where


def _length_forms(gen, B, n):
    ragged = torch.randint(1, n + 1, (B,), generator=gen, device=DEV)
    ragged[0] = 1
    ragged[-1] = n
    forms = [None]
    for dt in (torch.int32, torch.int64):
        forms += [torch.full((B,), n, dtype=dt, device=DEV), ragged.to(dt)]
    return forms


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).replace("torch.", ""))
def test_shape_grid(gpu, dtype, layout):
    gen = torch.Generator(device=DEV).manual_seed(11)
    for B in B_GRID:
        for C in C_GRID:
            for n in epd.n_grid(C):
                x = _view(gen, layout, B, C, n, dtype)
                for lengths in _length_forms(gen, B, n):
                    _check(x, lengths, (dtype, layout, B, C, n, None if lengths is None else (lengths.dtype, lengths.tolist())))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).replace("torch.", ""))
def test_several_channel_tiles_long_rows_and_more_work_than_workgroups(gpu, dtype):
    gen = torch.Generator(device=DEV).manual_seed(3)
    # 2 * tile_c + 1 channels, channels-last: three channel tiles per time tile, the last of one channel
    x = _view(gen, "bnc", 3, 2 * TC + 1, 2 * TT + 3, dtype)
    for lengths in _length_forms(gen, 3, 2 * TT + 3):
        _check(x, lengths, ("channel tiles", dtype))
    # rows longer than one work item of the rows routes, unit stride and stepped
    n = 2 * epd.row_chunk() + 5
    lengths = torch.tensor([epd.row_chunk() + 1, n], device=DEV)
    for layout in ("bcn", "slice"):
        _check(_view(gen, layout, 2, 2, n, dtype), lengths, ("long rows", layout, dtype))
    # 70 000 work items: beyond the 65 536 workgroups of a launch, every route strides
    B = 70000
    lengths = torch.randint(1, 4, (B,), generator=gen, device=DEV)
    for layout, C in (("bcn", 1), ("bnc", 2), ("slice", 1)):
        x = _view(gen, layout, B, C, 3, dtype)
        res = Packed(x, lengths)
        assert res.flags == 0 and res.guards_intact
        keep = (torch.arange(3, device=DEV)[None, :] < lengths[:, None])
        want = torch.stack([x[:, c, :][keep] for c in range(C)]).to(_out_dtype(dtype))
        assert torch.equal(_bits(res.values), _bits(want))
        res = Packed(x)
        assert torch.equal(_bits(res.values), _bits(x.permute(1, 0, 2).reshape(C, -1).to(_out_dtype(dtype))))


@pytest.mark.parametrize("layout", ("bcn", "bnc", "slice"))
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).replace("torch.", ""))
def test_nan_and_bad_length_flags(gpu, dtype, layout):
    gen = torch.Generator(device=DEV).manual_seed(9)
    B, C, n = 3, 5, TT + 1
    x = _view(gen, layout, B, C, n, dtype)
    for bad in (0, -1, n + 1):
        for pos in range(B):
            for ldt in (torch.int32, torch.int64):
                lengths = torch.tensor([n, 1, n // 2 + 1], dtype=ldt, device=DEV)
                lengths[pos] = bad
                res = Packed(x, lengths)
                assert res.flags == _native.TSFA_DENSE_BAD_LENGTH and res.guards_intact   # (no NaN flag: no gap was loaded)
                lens = lengths.clamp(0, n).tolist()
                assert res.offsets.tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist()
                assert torch.equal(_bits(res.values), _bits(_expected(x, lens)))
    x[1, 3, n - 1] = float("nan")
    assert Packed(x).flags == _native.TSFA_PACK_VALUE_NAN
    assert Packed(x, torch.tensor([n, n - 1, n], device=DEV)).flags == 0          # beyond the length: padding, never read
    assert Packed(x, torch.tensor([n, n, n + 1], device=DEV)).flags == _native.TSFA_PACK_VALUE_NAN | _native.TSFA_DENSE_BAD_LENGTH
    x[1, 3, n - 1] = float("-inf")
    res = Packed(x)
    assert res.flags == 0 and torch.equal(_bits(res.values), _bits(_expected(x, [n] * B)))


def test_half_subnormals_and_infinities_keep_their_value(gpu):
    for dtype, np_bits in ((torch.float16, np.arange(65536, dtype=np.uint16)), (torch.bfloat16, np.arange(65536, dtype=np.uint16))):
        t = torch.from_numpy(np_bits.view(np.int16)).to(DEV).view(dtype)
        finite_or_inf = ~torch.isnan(t)
        x = t[finite_or_inf].reshape(1, 1, -1)
        res = Packed(x)
        assert res.flags == 0 and torch.equal(_bits(res.values), _bits(x[0].to(torch.float32)))
        assert Packed(t.reshape(1, 1, -1)).flags == _native.TSFA_PACK_VALUE_NAN


def test_refused_arguments(gpu):
    x = torch.zeros((2, 3, 4), device=DEV)
    out = torch.zeros(64, device=DEV)
    offs = torch.zeros(8, dtype=torch.int64, device=DEV)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)

    def call(x_type=_native.TSFA_F32, shape=(2, 3, 4), strides=(12, 4, 1), cso=8, device=0):
        _native.pack_dense(x.data_ptr(), x_type, shape, strides, out.data_ptr(), cso, offs.data_ptr(), flags.data_ptr(), device=device)
    call()
    for kw, code in ((dict(x_type=_native.TSFA_I32), _native.TSFA_ERR_INVALID), (dict(strides=(12, -4, 1)), _native.TSFA_ERR_INVALID),
                     (dict(shape=(2, 0, 4)), _native.TSFA_ERR_INVALID), (dict(cso=7), _native.TSFA_ERR_INVALID),
                     (dict(shape=(1, 1, 33554432), strides=(0, 0, 0), cso=33554432), _native.TSFA_ERR_TOO_LONG),
                     (dict(device=4096), _native.TSFA_ERR_NO_DEVICE)):
        with pytest.raises(_native.NativeError) as ei:
            call(**kw)
        assert ei.value.code == code, kw
