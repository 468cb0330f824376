#!/usr/bin/env python
"""Timing of the rolled tensor entry on one device, in one process: writes profiles/roll_tensor_timing.md.

Shape: 1000 series x 1024 float32 samples, a window of 128 samples at every step (max_timeshift = min_timeshift = 127:
897 000 windows), EfficientFCParameters.  Three numbers:

(a) `extract_rolled_features_tensor(x, ...)`, x on the device: the windows are built in HBM, the feature matrix stays there;
(b) `extract_rolled_features(frame, pack="device")` on the equivalent DataFrame: the fastest route the frame entry has for
    these samples (device packer, device window builder, chunked copy-out, pandas assembly);
(c) the kernels of (a) alone, from `Plan.last_timings` in a run of its own with the plan's event timing on.

(a) and (b) are timed by the host clock around calls that end synchronised, after one warm-up call each, in alternating
rounds; the document holds the median and the range of each, the gap between (a) and (c), and the build id of the library
(the first 16 hex digits of sha256(libtsfresh_amd.so)).

    python profiles/roll_tensor_timing.py [--runs 5] [--out profiles/roll_tensor_timing.md] [--series 1000]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--series", type=int, default=1000, help="B (rehearsals use fewer)")
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--window", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roll_tensor_timing.md"))
    args = ap.parse_args()
    import pandas as pd
    import torch

    from tsfresh_amd import EfficientFCParameters, _native, extract_rolled_features, extract_rolled_features_tensor
    from tsfresh_amd.feature_extraction import extraction
    from tsfresh_amd.feature_extraction.plan import compile_fc_parameters
    if _native.device_count() < 1:
        raise SystemExit("roll_tensor_timing.py needs a HIP device: nothing is measured without one")
    B, n, w = args.series, args.samples, args.window
    roll = dict(rolling_direction=1, max_timeshift=w - 1, min_timeshift=w - 1)
    params = EfficientFCParameters()
    x = torch.from_numpy(np.random.default_rng(11).standard_normal((B, n)).astype(np.float32)).to("cuda:0")
    frame = pd.DataFrame({"id": np.repeat(np.arange(B, dtype=np.int64), n), "t": np.tile(np.arange(n, dtype=np.int64), B),
                          "0": x.cpu().numpy().reshape(-1)})
    res = {}

    def tensor_route():
        res["t"] = extract_rolled_features_tensor(x, default_fc_parameters=params, **roll)

    def frame_route():
        res["f"] = extract_rolled_features(frame, column_id="id", column_sort="t", default_fc_parameters=params, pack="device",
                                           device=0, **roll)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    print("warm-up: tensor route %.3f s, frame route %.3f s" % (wall(tensor_route), wall(frame_route)), flush=True)
    feats, cols, series, positions = res["t"]
    want = res["f"]
    n_windows = int(feats.shape[0])
    same = bool(cols == list(want.columns) and list(zip(series.tolist(), positions.tolist())) == list(want.index))
    # the cells, in row blocks: the matrix is gigabytes, and the host copy of a block goes before the next is made
    equal = close = same
    for r0 in range(0, n_windows, 65536):
        got, ref = feats[r0:r0 + 65536].cpu().numpy(), want.iloc[r0:r0 + 65536].to_numpy()
        equal = equal and np.array_equal(got, ref, equal_nan=True)
        close = close and np.allclose(got, ref, rtol=1e-9, atol=1e-12, equal_nan=True)
    del want, got, ref
    res.clear()
    t_tensor, t_frame = [], []
    for r in range(args.runs):
        t_tensor.append(wall(tensor_route))
        res.clear()
        t_frame.append(wall(frame_route))
        res.clear()
        print("round %d: tensor route %.3f s, frame route %.3f s" % (r, t_tensor[-1], t_frame[-1]), flush=True)
    # (c) kernel-only time: a run of its own with the plan's event timing on
    plan = extraction._acquire_plan(compile_fc_parameters(params, has_datetime_index=False), 0)
    parts = [pl for pl, _ in plan.parts] if hasattr(plan, "parts") else [plan]
    for pl in parts:
        pl.set_profiling(True)
    tensor_route()
    timings = [(name, ms) for pl in parts for name, ms in pl.last_timings()]
    kernel_s = sum(ms for _, ms in timings) / 1e3
    for pl in parts:
        pl.set_profiling(False)
    res.clear()
    with open(_native.LIB_PATH, "rb") as f:
        build = hashlib.sha256(f.read()).hexdigest()[:16]
    ma, mb = statistics.median(t_tensor), statistics.median(t_frame)
    lines = ["# Rolling on tensors: timing", "",
             "Written by `profiles/roll_tensor_timing.py` on %s, one process, one device; library build id "
             "(sha256(libtsfresh_amd.so)[:16]) `%s`." % (torch.cuda.get_device_name(0), build), "",
             "%d series x %d float32 samples, window %d at stride 1 (`max_timeshift=%d, min_timeshift=%d`): %d windows, "
             "EfficientFCParameters (%d columns), a float64 result matrix of %.2f GB." % (
                 B, n, w, w - 1, w - 1, n_windows, len(cols), n_windows * len(cols) * 8 / 1e9), "",
             "Host clock around synchronised calls, one warm-up call per route, then %d rounds with the two routes alternating; "
             "median (min .. max) in seconds." % args.runs, "",
             "| | route | seconds | windows / s |", "|---|---|---|---|",
             "| (a) | `extract_rolled_features_tensor(x)` (x on the device; windows built in HBM; features stay on the device) | "
             "%.4f (%.4f .. %.4f) | %.0f |" % (ma, min(t_tensor), max(t_tensor), n_windows / ma),
             "| (b) | `extract_rolled_features(frame, pack=\"device\")` (DataFrame in, DataFrame out) | %.4f (%.4f .. %.4f) | %.0f |" % (
                 mb, min(t_frame), max(t_frame), n_windows / mb),
             "| (c) | kernels of (a) alone (`Plan.last_timings`, a profiling run of its own) | %.4f | %.0f |" % (
                 kernel_s, n_windows / kernel_s if kernel_s else float("nan")), "",
             "Rounds in order, seconds: (a) %s; (b) %s." % (", ".join("%.4f" % t for t in t_tensor),
                                                             ", ".join("%.4f" % t for t in t_frame)), "",
             "(a) / (b) = %.3f: the tensor route's median %s the frame route's.  (a) - (c) = %.4f s: the dense packer, the window "
             "builder, the allocation of the result, the length statistics of the batch and the launches' host side." % (
                 ma / mb, "does not exceed" if ma <= mb else "EXCEEDS", ma - kernel_s), "",
             "The two routes returned %s names and window index; their cells are %s." % (
                 "the same" if same else "DIFFERENT",
                 "bit-equal" if equal else ("equal to 1e-9 relative (the frame route extracts in row chunks, whose launches size their "
                                            "workgroups by their own windows)" if close else "DIFFERENT")), "",
             "Kernel families of (c), milliseconds: " + ", ".join("%s %.2f" % (name, ms) for name, ms in timings) + ".", ""]
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
