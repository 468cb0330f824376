#!/usr/bin/env python
"""Timing of the tensor front door on one device, in one process: writes profiles/dense_pack_timing.md.

1. The dense packer (tsfa_pack_dense) against torch doing the same job on the same tensor -- what a caller of
   `Plan.extract_device` had to do before the packer existed: `x.permute(0, 2, 1).contiguous()`, plus `.float()` for bfloat16.
   Shapes [B, n, C] = 100 000 x 1024 x 1 and 12 500 x 1024 x 8, bfloat16 and float32.  Both legs are enqueued on torch's
   current stream between two HIP events, after a warm-up, interleaved A / B for --runs rounds; the table holds the median
   and the quartiles of each leg.
2. End to end on 100 000 x 1024 float32 with ComprehensiveFCParameters: `extract_features_tensor` on the device tensor against
   `extract_features` on the equivalent DataFrame (host clock around calls that end synchronised), series per second for each
   route, and the kernel-only time `Plan.last_timings` reports for the tensor route (a run of its own, with profiling on).

    python profiles/dense_pack_timing.py [--runs 21] [--e2e-runs 5] [--out profiles/dense_pack_timing.md] [--skip-e2e]
"""
import argparse
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


def pack_legs(torch, _native, x, runs):
    """x: [B, n, C] on the device -> ([ms of the fused kernel], [ms of torch's passes]), interleaved."""
    B, n, C = x.shape
    x3 = x.permute(0, 2, 1)
    half = x.dtype == torch.bfloat16
    x_type = _native.TSFA_BF16 if half else _native.TSFA_F32
    values = torch.empty((C, B * n), dtype=torch.float32, device=x.device)
    offsets = torch.empty(B + 1, dtype=torch.int64, device=x.device)
    flag = torch.zeros(1, dtype=torch.int32, device=x.device)
    stream = torch.cuda.current_stream().cuda_stream

    def fused():
        _native.pack_dense(x3.data_ptr(), x_type, (B, C, n), x3.stride(), values.data_ptr(), B * n, offsets.data_ptr(),
                           flag.data_ptr(), device=x.device.index, stream=stream)

    def torch_passes():
        y = x.permute(0, 2, 1).contiguous()
        return y.float() if half else y

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for _ in range(3):
        timed(fused)
        timed(torch_passes)
    got = values.view(C, B, n).permute(1, 0, 2)
    assert torch.equal(got, torch_passes().float()), "the two legs disagree"
    t_fused, t_torch = [], []
    for _ in range(runs):
        t_fused.append(timed(fused))
        t_torch.append(timed(torch_passes))
    return t_fused, t_torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--e2e-runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_pack_timing.md"))
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the batch sizes (rehearsals)")
    args = ap.parse_args()
    if args.runs < 20:
        ap.error("--runs must be at least 20")
    import torch

    from tsfresh_amd import ComprehensiveFCParameters, _native, extract_features, extract_features_tensor
    from tsfresh_amd.feature_extraction import extraction
    from tsfresh_amd.feature_extraction.plan import compile_fc_parameters
    if _native.device_count() < 1:
        raise SystemExit("dense_pack_timing.py needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda:0")
    lines = ["# Dense packer and tensor entry: timing", "",
             "Written by `profiles/dense_pack_timing.py` on %s, one process, one device.  HIP events on torch's current "
             "stream, 3 warm-up rounds, %d timed rounds with the two legs alternating; median (lower quartile .. upper "
             "quartile) in milliseconds." % (torch.cuda.get_device_name(0), args.runs), "",
             "## 1. tsfa_pack_dense against torch's permute().contiguous() (+ .float() for bfloat16)", "",
             "| [B, n, C] | dtype | route | fused kernel ms | torch passes ms | fused / torch | GB/s of the fused kernel |",
             "|---|---|---|---|---|---|---|"]
    for B, n, C in ((int(100000 * args.scale), 1024, 1), (int(12500 * args.scale), 1024, 8)):
        for dtype in (torch.bfloat16, torch.float32):
            x = torch.randn((B, n, C), device=dev, dtype=torch.float32).to(dtype)
            t_fused, t_torch = pack_legs(torch, _native, x, args.runs)
            (mf, lf, hf), (mt, lt, ht) = quartiles(t_fused), quartiles(t_torch)
            traffic = B * n * C * (x.element_size() + 4)
            lines.append("| %d x %d x %d | %s | %s | %.3f (%.3f .. %.3f) | %.3f (%.3f .. %.3f) | %.2f | %.0f |" % (
                B, n, C, str(dtype).replace("torch.", ""), "rows, unit stride" if C == 1 else "LDS transpose", mf, lf, hf, mt, lt, ht,
                mf / mt, traffic / mf / 1e6))
            del x
    lines += ["", "The two medians differ beyond their spread where the quartile ranges do not overlap.  With C = 1 and float32 "
              "torch's leg is empty: `permute(0, 2, 1).contiguous()` of a `[B, n, 1]` tensor returns the tensor itself and no kernel "
              "runs, so that row compares the copy into caller-provided buffers with no copy at all.", ""]

    if not args.skip_e2e:
        import pandas as pd
        B, n = int(100000 * args.scale), 1024
        params = ComprehensiveFCParameters()
        x = torch.randn((B, n), device=dev, dtype=torch.float32)
        host = x.cpu().numpy()
        frame = pd.DataFrame({"id": np.repeat(np.arange(B, dtype=np.int64), n), "time": np.tile(np.arange(n, dtype=np.int64), B),
                              "0": host.reshape(-1)})

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

        res = {}
        t_tensor = wall(lambda: res.__setitem__("t", extract_features_tensor(x, default_fc_parameters=params)), args.e2e_runs)
        t_frame = wall(lambda: res.__setitem__("f", extract_features(frame, column_id="id", column_sort="time",
                                                                      default_fc_parameters=params, device=0)), args.e2e_runs)
        feats, cols = res["t"]
        same = bool(cols == list(res["f"].columns) and np.array_equal(feats.cpu().numpy(), res["f"].to_numpy(), equal_nan=True))
        # kernel-only time: a run of its own with the plan's event timing on
        plan = extraction._acquire_plan(compile_fc_parameters(params, has_datetime_index=False), 0)
        parts = [pl for pl, _ in plan.parts] if hasattr(plan, "parts") else [plan]
        for pl in parts:
            pl.set_profiling(True)
        extract_features_tensor(x, default_fc_parameters=params)
        kernel_ms = sum(ms for pl in parts for _, ms in pl.last_timings())
        for pl in parts:
            pl.set_profiling(False)
        mt, mf = statistics.median(t_tensor), statistics.median(t_frame)
        lines += ["## 2. End to end: %d series x %d float32 samples, ComprehensiveFCParameters (%d columns)" % (B, n, len(cols)), "",
                  "Host clock around synchronised calls, one warm-up call, median of %d (min .. max)." % args.e2e_runs, "",
                  "| route | seconds | series / s |", "|---|---|---|",
                  "| `extract_features_tensor(x)` (x on the device, features stay on the device) | %.4f (%.4f .. %.4f) | %.0f |" % (
                      mt, min(t_tensor), max(t_tensor), B / mt),
                  "| `extract_features(frame)` (DataFrame in, DataFrame out) | %.4f (%.4f .. %.4f) | %.0f |" % (
                      mf, min(t_frame), max(t_frame), B / mf),
                  "| kernels of the tensor route alone (`Plan.last_timings`, profiling run) | %.4f | %.0f |" % (
                      kernel_ms / 1e3, B / (kernel_ms / 1e3) if kernel_ms else float("nan")), "",
                  "The two routes returned %s columns and cells." % ("the same" if same else "DIFFERENT"), ""]
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
