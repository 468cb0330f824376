"""Two lanes: by default the latency-bound families of a batch run on a side stream beside the others,
forked after k_basic and joined before run_batch returns.  The lanes run the same kernels on the same data, so every test
here asks for bit identity with the one-lane schedule (plan option side_lane = 0).  The option parser's refusals need no GPU."""
import ctypes
import warnings

import numpy as np
import pytest
import torch   # at collection: torch's HIP runtime is then the one this process opens the device with

from engines import hip_engine
from tsfresh_amd import _native
from tsfresh_amd.feature_extraction import settings
from tsfresh_amd.feature_extraction.plan import compile_fc_parameters

# family bits of the side_lane mask (enum tsfa_family)
SPECTRAL, AR, CWT, SEQ, TREND = 1 << 2, 1 << 3, 1 << 5, 1 << 6, 1 << 7
EVERY_SIDE_FAMILY = SPECTRAL | AR | CWT | SEQ | TREND

_RAGGED = {}


def _ragged(dtype):
    """200 ragged series of 20 .. 1100 samples (several launch groups' worth of lengths) plus 40 of exactly 1024, and their
    one-lane matrix, computed once per sample type."""
    if dtype not in _RAGGED:
        rng = np.random.default_rng(91)
        lens = list(rng.integers(20, 1101, size=200)) + [1024] * 40
        series = [(rng.standard_normal(n) if i % 2 else np.cumsum(rng.standard_normal(n))).astype(dtype) for i, n in enumerate(lens)]
        values = np.concatenate(series)
        offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            names, one_lane = hip_engine(settings.ComprehensiveFCParameters(), values, offsets, options={"side_lane": 0})
        one_lane.setflags(write=False)
        _RAGGED[dtype] = (values, offsets, names, one_lane)
    return _RAGGED[dtype]


def _differing(names, a, b):
    return [names[j] for j in np.nonzero(~((a == b) | (np.isnan(a) & np.isnan(b))).all(axis=0))[0]][:8]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("lanes", ["default", "every_family"])
def test_two_lanes_change_no_bit(gpu, dtype, lanes):
    """The default schedule, and the widest one the parser admits, against side_lane = 0."""
    values, offsets, names, one_lane = _ragged(dtype)
    options = {"side_lane": EVERY_SIDE_FAMILY} if lanes == "every_family" else {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        names2, two_lanes = hip_engine(settings.ComprehensiveFCParameters(), values, offsets, options=options)
    assert names == names2
    assert np.array_equal(one_lane, two_lanes, equal_nan=True), _differing(names, one_lane, two_lanes)


def _comprehensive_plan():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fplan = compile_fc_parameters(settings.ComprehensiveFCParameters())
    return fplan, _native.Plan(fplan.native_specs(_native.calc_id), device=0)


@pytest.mark.gpu
def test_back_to_back_calls_on_one_stream(gpu):
    """Six extract_device calls on one plan and one caller stream with no synchronisation in between (the length hint skips
    the length scan and its host sync): three 64 x 1024 batches into three output buffers, A B C A B C.  Every result, of
    the first round (copied aside on the same stream) and of the second, must equal the batch's single-call result: a
    missing join, or a buffer of the side lane's kernels reused while they run, shows here."""
    dev = torch.device("cuda", 0)
    fplan, plan = _comprehensive_plan()
    n, length, n_cols = 64, 1024, len(fplan)
    try:
        plan.set_length_hint(length, length)
        rng = np.random.default_rng(5)
        batches = [rng.standard_normal((n, length)).astype(np.float32), np.cumsum(rng.standard_normal((n, length)), axis=1).astype(np.float32),
                   np.round(rng.standard_normal((n, length)), 1).astype(np.float32)]
        xs = [torch.from_numpy(b.reshape(-1)).to(dev) for b in batches]
        offsets = torch.arange(n + 1, dtype=torch.int64, device=dev) * length
        stream = torch.cuda.Stream(device=dev)
        single = []
        for x in xs:
            out = torch.full((n, n_cols), -7.0, device=dev, dtype=torch.float64)
            torch.cuda.synchronize(dev)
            plan.extract_device(x.data_ptr(), _native.TSFA_F32, offsets.data_ptr(), n, out.data_ptr(), n_cols, stream.cuda_stream)
            stream.synchronize()
            single.append(out.cpu().numpy())
        outs = [torch.full((n, n_cols), -7.0, device=dev, dtype=torch.float64) for _ in xs]
        first_round = []
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(stream):
            for rnd in range(2):
                for x, out in zip(xs, outs):
                    plan.extract_device(x.data_ptr(), _native.TSFA_F32, offsets.data_ptr(), n, out.data_ptr(), n_cols, stream.cuda_stream)
                    if rnd == 0:
                        first_round.append(out.clone())   # a copy on the same stream: no host sync
        stream.synchronize()
        for i in range(3):
            assert np.array_equal(single[i], first_round[i].cpu().numpy(), equal_nan=True), ("first round", i)
            assert np.array_equal(single[i], outs[i].cpu().numpy(), equal_nan=True), ("second round", i)
    finally:
        plan.close()


@pytest.mark.gpu
def test_profiling_keeps_one_lane_and_names_every_kernel_once(gpu):
    """With profiling on the batch is launched on one lane: the same bits, and last_timings() names every kernel once, in the
    one-lane order."""
    values, offsets, names, one_lane = _ragged(np.float32)
    timed = {}
    for side_lane in (None, 0):
        fplan, plan = _comprehensive_plan()
        try:
            if side_lane is not None:
                plan.set_option("side_lane", side_lane)
            plan.set_profiling(True)
            got = plan.extract_host(values, offsets)
            timed[side_lane] = [name for name, _ in plan.last_timings()]
        finally:
            plan.close()
        assert np.array_equal(one_lane, got, equal_nan=True), _differing(names, one_lane, got)
    assert timed[None] == timed[0] and len(set(timed[None])) == len(timed[None]), timed
    assert {"k_basic", "k_entropy", "k_ar", "k_sort", "k_perm", "k_cwtpeaks", "k_seq", "k_spectral", "k_trend",
            "k_cwt_gemm"} <= set(timed[None]), timed


@pytest.mark.gpu
@pytest.mark.parametrize("family", [6, 3, 1])   # SEQ (the side lane's first launch), AR (main lane, side lane busy), SORT (k_perm)
def test_an_error_after_the_fork_leaves_the_plan_usable(gpu, family):
    """run_batch leaves with an error after the launches of one family (plan option fail_after, a test hook) while the side lane
    holds work: the join is still enqueued, so the next call on the plan returns the reference bits."""
    values, offsets, names, one_lane = _ragged(np.float32)
    fplan, plan = _comprehensive_plan()
    try:
        plan.set_option("fail_after", family)
        with pytest.raises(_native.NativeError, match="fail_after"):
            plan.extract_host(values, offsets)
        plan.set_option("fail_after", -1)
        got = plan.extract_host(values, offsets)
    finally:
        plan.close()
    assert np.array_equal(one_lane, got, equal_nan=True), _differing(names, one_lane, got)


def test_side_lane_mask_is_refused_for_the_sharing_families():
    """BASIC, SORT and ENTROPY carry the shared statistics and the shared sample order: a side_lane mask that names one of
    them is refused by the option parser, which looks at the mask before it looks at the plan -- so this runs without a
    device.  A mask it admits gets past that check (and is then refused for the missing plan)."""
    lib = _native.load()

    def refusal(value):
        rc = lib.tsfa_plan_set_option(None, b"side_lane", ctypes.c_double(value))
        return rc, lib.tsfa_last_error().decode()

    for bit, name in ((0, "BASIC"), (1, "SORT"), (4, "ENTROPY")):
        for mask in (1 << bit, (1 << bit) | SEQ, (1 << bit) | EVERY_SIDE_FAMILY):
            rc, why = refusal(mask)
            assert rc == _native.TSFA_ERR_INVALID and name in why and "main lane" in why, (mask, rc, why)
    for bad in (-1.0, 0.5, float(1 << 9), float(SEQ | (1 << 9)), float(1 << 10), float("nan")):
        rc, why = refusal(bad)
        assert rc == _native.TSFA_ERR_INVALID and "bit mask" in why, (bad, rc, why)
    for mask in (0, SEQ, EVERY_SIDE_FAMILY, 1 << 8):
        rc, why = refusal(mask)
        assert rc == _native.TSFA_ERR_INVALID and "unknown library option" in why, (mask, rc, why)
