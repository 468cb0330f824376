#!/usr/bin/env python
"""Timing of `times=` on the tensor entries, on one device, in one process: writes profiles/times_tensor_timing.md.

On 100 000 x 1024 float32 samples with a (B, n) int64 nanosecond clock:

1. The times packer (tsfa_pack_times) alone, next to the dense packer (tsfa_pack_dense) on a float64 [B, 1, n] batch of the
   same shape: both read 8 bytes and write 8 bytes per element; the times packer also converts and divides twice in
   float64.  Both legs are enqueued on torch's current stream between two HIP events, after a warm-up, alternating for
   --runs rounds; median and quartiles in milliseconds, and GB/s of the 16 bytes per element.
2. `extract_features_tensor(x, times=t)` against the same call without `times`, ComprehensiveFCParameters: the cost of the
   five linear_trend_timewise columns and the hours array (host clock around calls that end synchronised).
3. The entry against `extract_features` on the DataFrame that carries the same stamps as its DatetimeIndex: the route an
   irregularly sampled batch had before.

    python profiles/times_tensor_timing.py [--runs 21] [--e2e-runs 5] [--frame-runs 2] [--out profiles/times_tensor_timing.md]
"""
import argparse
import hashlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def quartiles(ms):
    q = statistics.quantiles(ms, n=4)
    return statistics.median(ms), q[0], q[2]


def pack_legs(torch, _native, t, runs):
    """t: (B, n) int64 ns on the device -> ([ms of tsfa_pack_times], [ms of tsfa_pack_dense on float64 [B, 1, n]])."""
    B, n = t.shape
    dev = t.device
    x64 = torch.randn((B, 1, n), device=dev, dtype=torch.float64)
    values = torch.empty((1, B * n), dtype=torch.float64, device=dev)
    offsets = torch.empty(B + 1, dtype=torch.int64, device=dev)
    hours = torch.empty(B * n, dtype=torch.float64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def dense():
        _native.pack_dense(x64.data_ptr(), _native.TSFA_F64, (B, 1, n), x64.stride(), values.data_ptr(), B * n, offsets.data_ptr(),
                           flag.data_ptr(), device=dev.index, stream=stream)

    def times():
        _native.pack_times(t.data_ptr(), _native.TSFA_I64, 10 ** 9, (B, n), t.stride(), offsets.data_ptr(), hours.data_ptr(),
                           flag.data_ptr(), device=dev.index, stream=stream)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for _ in range(3):
        timed(dense)
        timed(times)
    # the hours are pandas' (checked on the first series; tests/test_tensor_times_gpu.py holds the full comparison)
    k = min(B, 64)
    th = t[:k].cpu().numpy()
    want = ((th - th[:, :1]) / 10 ** 9 / 3600.0).reshape(-1)
    assert np.array_equal(hours[:k * n].cpu().numpy().view(np.uint64), want.view(np.uint64)), "the hours are not pandas'"
    assert int(flag.item()) == 0
    t_times, t_dense = [], []
    for _ in range(runs):
        t_times.append(timed(times))
        t_dense.append(timed(dense))
    return t_times, t_dense


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--e2e-runs", type=int, default=5)
    ap.add_argument("--frame-runs", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "times_tensor_timing.md"))
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the batch size (rehearsals)")
    args = ap.parse_args()
    if args.runs < 20:
        ap.error("--runs must be at least 20")
    import torch

    from tsfresh_amd import ComprehensiveFCParameters, _native, extract_features, extract_features_tensor
    if _native.device_count() < 1:
        raise SystemExit("times_tensor_timing.py needs a HIP device: nothing is measured without one")
    with open(_native.LIB_PATH, "rb") as f:
        build = hashlib.sha256(f.read()).hexdigest()[:16]
    dev = torch.device("cuda:0")
    B, n = int(100000 * args.scale), 1024
    torch.manual_seed(5)
    x = torch.randn((B, n), device=dev, dtype=torch.float32)
    t = 1_600_000_000 * 10 ** 9 + torch.randint(1, 2 * 10 ** 9, (B, n), device=dev, dtype=torch.int64).cumsum(dim=1)

    lines = ["# `times=` on the tensor entries: timing", "",
             "Written by `profiles/times_tensor_timing.py` on %s, one process, one device; library build id "
             "(sha256(libtsfresh_amd.so)[:16]) `%s`.  %d series x %d float32 samples, a (B, n) int64 nanosecond clock with "
             "irregular steps." % (torch.cuda.get_device_name(0), build, B, n), "",
             "## 1. tsfa_pack_times next to tsfa_pack_dense on a float64 [B, 1, n] batch", "",
             "HIP events on torch's current stream, 3 warm-up rounds, %d timed rounds with the two legs alternating; median "
             "(lower quartile .. upper quartile) in milliseconds; GB/s counts the 8 bytes read and the 8 bytes written per "
             "element." % args.runs, "",
             "| kernel | ms | GB/s |", "|---|---|---|"]
    t_times, t_dense = pack_legs(torch, _native, t, args.runs)
    (mt, lt, ht), (md, ld, hd) = quartiles(t_times), quartiles(t_dense)
    traffic = B * n * 16
    lines += ["| `tsfa_pack_times` (int64 ns -> float64 hours: one conversion, two divisions) | %.3f (%.3f .. %.3f) | %.0f |" % (
                  mt, lt, ht, traffic / mt / 1e6),
              "| `tsfa_pack_dense` (float64 -> float64: a copy with a NaN test) | %.3f (%.3f .. %.3f) | %.0f |" % (
                  md, ld, hd, traffic / md / 1e6), "",
              "The times packer runs at %.2f of the dense packer's rate." % (md / mt), ""]

    def wall(fn, runs):
        fn()
        out = []
        for _ in range(runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append(time.perf_counter() - t0)
        return out

    params = ComprehensiveFCParameters()
    res = {}

    def plain():
        res["plain"] = extract_features_tensor(x, default_fc_parameters=params)

    def timed():
        res["timed"] = extract_features_tensor(x, default_fc_parameters=params, times=t)

    plain()   # warm-up of each leg
    timed()
    t_plain, t_timed = [], []
    for _ in range(args.e2e_runs):   # alternating
        for fn, out in ((plain, t_plain), (timed, t_timed)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append(time.perf_counter() - t0)
    n_plain, n_timed = len(res["plain"][1]), len(res["timed"][1])
    mp, mtd = statistics.median(t_plain), statistics.median(t_timed)
    lines += ["## 2. The entry with and without `times`, ComprehensiveFCParameters", "",
              "Host clock around synchronised calls, a warm-up call of each leg, %d timed calls of each, alternating; median "
              "(min .. max)." % args.e2e_runs, "",
              "| call | columns | seconds | series / s |", "|---|---|---|---|",
              "| `extract_features_tensor(x)` | %d | %.4f (%.4f .. %.4f) | %.0f |" % (n_plain, mp, min(t_plain), max(t_plain), B / mp),
              "| `extract_features_tensor(x, times=t)` | %d | %.4f (%.4f .. %.4f) | %.0f |" % (
                  n_timed, mtd, min(t_timed), max(t_timed), B / mtd), "",
              "The clock costs %.1f ms per call (%+.1f %%): the hours array and five more columns." % (
                  (mtd - mp) * 1e3, (mtd / mp - 1) * 100), ""]

    if args.frame_runs > 0:
        import pandas as pd
        frame = pd.DataFrame({"id": np.repeat(np.arange(B, dtype=np.int64), n), "0": x.cpu().numpy().reshape(-1)},
                             index=pd.DatetimeIndex(t.cpu().numpy().reshape(-1).view("datetime64[ns]")))
        t_frame = wall(lambda: res.__setitem__("frame", extract_features(frame, column_id="id", default_fc_parameters=params, device=0)),
                       args.frame_runs)
        feats, cols = res["timed"]
        same = bool(cols == list(res["frame"].columns) and np.array_equal(feats.cpu().numpy(), res["frame"].to_numpy(), equal_nan=True))
        mf = statistics.median(t_frame)
        lines += ["## 3. Against the frame route on the DatetimeIndex frame of the same data", "",
                  "One warm-up call, median of %d (min .. max).  The frame route packs on the host (the device packer refuses a "
                  "DatetimeIndex) and computes the hours with pandas." % args.frame_runs, "",
                  "| route | seconds | series / s |", "|---|---|---|",
                  "| `extract_features_tensor(x, times=t)` (device tensors in, features stay on the device) | %.4f | %.0f |" % (mtd, B / mtd),
                  "| `extract_features(frame)` (DataFrame with a DatetimeIndex in, DataFrame out) | %.4f (%.4f .. %.4f) | %.0f |" % (
                      mf, min(t_frame), max(t_frame), B / mf), "",
                  "The tensor entry is %.1f times as fast; the two routes returned %s columns and cells." % (
                      mf / mtd, "the same" if same else "DIFFERENT"), ""]
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
