"""matrix_profile with an explicit window on the device: k_mprofile (tsfresh_amd/csrc/fam_mprofile.h) through the C ABI against
the brute force of the definition (tests/mprofile_ref.py), against the g++ build of the same body bit for bit, alone and in
a batch, in LDS and in HBM scratch, through extract_features, and for what a destroyed plan leaves behind."""
import functools

import numpy as np
import pytest

import emul_mprofile_lib
import mprofile_cases as cases
import mprofile_ref
from engines import hip_engine

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _device_small(length_classes=True):
    values, offsets = cases.small_batch()
    names, out = hip_engine(cases.fc_parameters(), values, offsets, options={"length_classes": 1.0 if length_classes else 0.0})
    return names, np.array(out)


def test_small_batch_against_the_brute_force(gpu):
    values, offsets = cases.small_batch()
    cols = cases.columns()
    names, got = _device_small()
    assert names == ['value__matrix_profile__feature_"%s"__windows_%d' % (f, w) for w, f in cols]
    bad = cases.mismatches(got, cases.small_reference(), cols, offsets)
    assert not bad, (len(bad), bad[:8])


def test_small_batch_equals_the_emulation_bit_for_bit(gpu):
    """Both builds use -ffp-contract=off; division and square root are correctly rounded on both sides, the maxima are
    order-free and the sums run in one order: the bits agree."""
    values, offsets = cases.small_batch()
    want = emul_mprofile_lib.emul_mprofile(cases.columns(), values, offsets)
    _, got = _device_small()
    diff = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    assert len(diff) == 0, (len(diff), [(int(s), int(c), got[s, c], want[s, c]) for s, c in diff[:6]])


def test_float32_batch(gpu):
    values, offsets = cases.small_batch_f32()
    cols = cases.columns()
    _, got = hip_engine(cases.fc_parameters(), values, offsets)
    bad = cases.mismatches(got, cases.small_reference_f32(), cols, offsets)
    assert not bad, (len(bad), bad[:8])
    want = emul_mprofile_lib.emul_mprofile(cols, values, offsets)
    assert np.array_equal(got, want, equal_nan=True)


def test_a_series_gives_the_same_bits_alone_as_in_the_batch(gpu):
    """... with the length classes on and off, and from the HBM-scratch build (force_long) as from LDS."""
    values, offsets = cases.small_batch()
    _, batch = _device_small()
    _, flat = _device_small(False)
    assert np.array_equal(batch, flat, equal_nan=True)
    _, long_build = hip_engine(cases.fc_parameters(), values, offsets, options={"force_long": 1.0})
    assert np.array_equal(batch, long_build, equal_nan=True)
    from tsfresh_amd import _native
    from tsfresh_amd.feature_extraction.plan import compile_fc_parameters
    plan = _native.Plan(compile_fc_parameters(cases.fc_parameters()).native_specs(_native.calc_id))
    try:
        for s in range(len(offsets) - 1):
            x = values[offsets[s]:offsets[s + 1]]
            alone = plan.extract_host(x, np.array([0, len(x)], dtype=np.int64))
            assert np.array_equal(np.asarray(alone)[0], batch[s], equal_nan=True), (s, len(x))
    finally:
        plan.close()


def test_longer_series_and_a_window_of_200(gpu):
    """300 and 1024 and 2048 samples in LDS, 4096 from HBM scratch, in one ragged batch; w in {8, 36, 200}."""
    rng = np.random.default_rng(77)
    parts = [cases.series(kind, n, rng) for n, kind in ((300, "noise"), (1024, "repeat"), (2048, "walk"), (4096, "round1"))]
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    values = np.concatenate(parts)
    windows = (8, 36, 200)
    cols = cases.columns(windows)
    _, got = hip_engine(cases.fc_parameters(windows), values, offsets)
    bad = cases.mismatches(got, cases.reference(values, offsets, cols), cols, offsets)
    assert not bad, (len(bad), bad[:8])


def test_21000_samples_take_the_hbm_scratch_route(gpu):
    n, w = 21000, 36
    assert n > emul_mprofile_lib.longest_in_lds(8)
    x = np.random.default_rng(21).standard_normal(n)
    x[15000:15100] = x[400:500]
    offsets = np.array([0, n], dtype=np.int64)
    cols = cases.columns((w,))
    _, got = hip_engine(cases.fc_parameters((w,)), x, offsets)
    bad = cases.mismatches(got, cases.reference(x, offsets, cols), cols, offsets)
    assert not bad, bad


def test_extract_features_end_to_end(gpu):
    import pandas as pd

    from tsfresh_amd import extract_features
    rng = np.random.default_rng(8)
    lengths = [40, 64, 100]
    df = pd.DataFrame({"id": np.repeat(np.arange(len(lengths)), lengths),
                       "time": np.concatenate([np.arange(n) for n in lengths]),
                       "value": np.round(rng.standard_normal(sum(lengths)), 2)})
    mp = [{"windows": 12, "feature": f} for f in mprofile_ref.FEATURES]
    with_mp = extract_features(df, column_id="id", column_sort="time",
                               default_fc_parameters={"mean": None, "matrix_profile": mp, "maximum": None})
    without = extract_features(df, column_id="id", column_sort="time", default_fc_parameters={"mean": None, "maximum": None})
    assert list(with_mp.columns) == (["value__mean"] + ['value__matrix_profile__feature_"%s"__windows_12' % f for f in mprofile_ref.FEATURES]
                                     + ["value__maximum"])
    assert list(with_mp.index) == [0, 1, 2]
    for c in ("value__mean", "value__maximum"):
        assert np.array_equal(with_mp[c].to_numpy(), without[c].to_numpy())
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    cols = [(12, f) for f in mprofile_ref.FEATURES]
    want = cases.reference(df["value"].to_numpy(), offsets, cols)
    bad = cases.mismatches(with_mp.iloc[:, 1:7].to_numpy(), want, cols, offsets)
    assert not bad, bad


_FREE_MEMORY_SCRIPT = r"""
import sys
import numpy as np
import torch   # first: torch ships its own HIP runtime and must be the one that opens the device in this process
torch.cuda.init()
sys.path.insert(0, %(root)r)
from tsfresh_amd import _native
rng = np.random.default_rng(4)
lengths = [64, 1000, 5000]            # the last one: HBM scratch
values = rng.standard_normal(sum(lengths))
offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
cid = _native.calc_id("matrix_profile")
specs = [(cid, (36.0, float(k), 0.0, 0.0)) for k in range(6)] + [(_native.calc_id("lempel_ziv_complexity"), (10.0, 0.0, 0.0, 0.0))]

def once():
    plan = _native.Plan(specs)
    out = np.array(plan.extract_host(values, offsets))
    plan.close()
    torch.cuda.synchronize()
    return out

first = once()                        # loads the code objects
before = torch.cuda.mem_get_info()[0]
for _ in range(10):
    assert np.array_equal(once(), first, equal_nan=True)
after = torch.cuda.mem_get_info()[0]
print("FREE", before, after)
assert after == before, (before, after)
print("MPROFILE_MEMORY_OK")
"""


def test_destroying_a_plan_frees_its_device_memory(gpu):
    """A plan with matrix_profile columns (one series long enough for the HBM scratch) created, run and destroyed ten times:
    the free device memory after the loop equals the value before it (a fresh child process, as in tests/test_pack_device.py)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", _FREE_MEMORY_SCRIPT % {"root": root}], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "MPROFILE_MEMORY_OK" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]
