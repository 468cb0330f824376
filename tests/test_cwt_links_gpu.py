"""number_cwt_peaks on the device: the column linker (widths up to 5, the default) against the general linker for every
width (plan option cwt_links = 0), bit for bit, on one ragged batch.  The lengths lie on both sides of 1 / 2 / 4 / 5
columns per thread and of the 256- / 1024-thread instantiations of k_cwtpeaks; the series are white noise, a random walk,
a sine in noise and integer-quantised noise (ties) at every length, one constant series and one ramp.  The oracle tests
(test_cwt_peaks_tiles_gpu.py, the short ladder, parity) pin the default route to the reference."""
import numpy as np
import pytest

import route_cases as rc
from engines import hip_engine

LENGTHS = (3, 7, 11, 64, 255, 256, 257, 1023, 1024, 1025, 2048, 2049)
KINDS = ("noise", "walk", "sine", "ties")
WIDTHS = (1, 2, 3, 4, 5, 6, 8)


def _series(n, kind):
    rng = np.random.default_rng([20261021, n, KINDS.index(kind)])
    if kind == "noise":
        x = rng.standard_normal(n)
    elif kind == "walk":
        x = np.cumsum(rng.standard_normal(n))
    elif kind == "sine":
        x = np.sin(np.arange(n) * 0.37) + 0.3 * rng.standard_normal(n)
    else:
        x = rng.integers(-3, 4, n).astype(np.float64)
    return x.astype(np.float32)


_cache = {}


def _batch():
    """-> (float32 values, offsets): built once."""
    if "batch" not in _cache:
        xs = [_series(n, kind) for n in LENGTHS for kind in KINDS]
        xs += [np.full(300, 2.5, dtype=np.float32), np.arange(700, dtype=np.float32) * 0.25]
        values = np.concatenate(xs)
        offsets = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
        values.setflags(write=False)
        _cache["batch"] = (values, offsets)
    return _cache["batch"]


def _extract_by_group(params, values, offsets, options):
    """A batch of this size is ONE launch, sized by its longest series: the series up to 64 samples, those up to 2048 and the
    2049-sample ones are extracted in a call each.  -> (names, matrix, threads of the CWT launch of every call)"""
    lens = np.diff(offsets)
    got, threads, names = None, [], None
    for lo, hi in ((0, 64), (64, 2048), (2048, 1 << 30)):
        rows = np.nonzero((lens > lo) & (lens <= hi))[0]
        xs = [values[offsets[i]:offsets[i + 1]] for i in rows]
        offs = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
        launches = []
        names, out = hip_engine(params, np.concatenate(xs), offs, options=options, launches=launches)
        threads.append(rc.record_of(launches, "CWT")["threads"])
        if got is None:
            got = np.full((len(lens), out.shape[1]), np.nan)
        got[rows] = out
    return names, got, threads


# every width in one plan (n = 1 then rides along with n = 8, on the general linker), and n = 1 beside each narrow width
# (it rides along with that width: the column linker leaves the marks of the lines that end on row 0)
PLANS = {"all": WIDTHS, "1+2": (1, 2), "1+3": (1, 3), "1+4": (1, 4), "1+5": (1, 5)}


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("plan", list(PLANS))
def test_column_links_and_general_links_count_alike(plan, dtype):
    values, offsets = _batch()
    params = {"number_cwt_peaks": [{"n": w} for w in PLANS[plan]]}
    names, got, threads = _extract_by_group(params, values.astype(dtype), offsets, None)
    names0, got0, threads0 = _extract_by_group(params, values.astype(dtype), offsets, {"cwt_links": 0})
    assert names == names0 and got.shape == (len(offsets) - 1, len(PLANS[plan]))
    # one wavefront, the 256-thread instantiation, and the 1024-thread one (512 threads at 2049 samples)
    assert threads == threads0 and threads[0] == 64 and threads[1] == 256 and threads[2] > 256, threads
    differ = ~((got == got0) | (np.isnan(got) & np.isnan(got0)))
    assert np.array_equal(got, got0, equal_nan=True), [
        (names[j], int(offsets[i + 1] - offsets[i]), got[i, j], got0[i, j]) for i, j in zip(*np.nonzero(differ))][:10]
    assert (np.nanmax(got, axis=0) > 0).all()   # (every width finds peaks somewhere: the comparison is not one of zeros)


@pytest.mark.gpu
def test_cwt_links_takes_zero_or_one():
    from tsfresh_amd import _native
    from tsfresh_amd.feature_extraction.plan import compile_fc_parameters
    fplan = compile_fc_parameters({"number_cwt_peaks": [{"n": 5}]})
    plan = _native.Plan(fplan.native_specs(_native.calc_id), device=0)
    try:
        plan.set_option("cwt_links", 0)
        plan.set_option("cwt_links", 1)
        for v in (2, 0.5, -1):
            with pytest.raises(Exception):
                plan.set_option("cwt_links", v)
    finally:
        plan.close()
