#!/usr/bin/env python
"""Timing of the valid-step packer (tsfa_pack_dense_valid, `nan_policy="drop"`), on one device, in one process: writes
profiles/dropna_pack_timing.md.

Two batches -- 100 000 x 1024 float32 with one kind ([B, n]) and 12 500 x 1024 x 8 channels-last bfloat16 ([B, n, C]) --
each with 0 %, 1 % and 30 % of the steps dropped (a NaN in one kind of the step), and a (B, n) int64 nanosecond clock.

1. The packers alone, no clock: `tsfa_pack_dense_valid` on the batch with gaps next to `tsfa_pack_dense` on the same batch
   without NaN.  GB/s counts the samples read once and the samples written.
2. With the clock, what a caller pays for packed samples + hours:
     drop   tsfa_pack_dense_valid + tsfa_pack_times on the kept stamps
     (a)    tsfa_pack_dense + tsfa_pack_times on the batch without NaN: the price of the policy when nothing is dropped
     (b)    the torch composition a user writes today, then the existing packers with `lengths`: the isnan / any mask, a
            stable per-row sort of the mask, gathers of every kind and of the stamps, the kept counts

Every leg is enqueued on torch's current stream between two HIP events, after a warm-up; the legs of one table row alternate for
--runs rounds; median and quartiles in milliseconds.

    python profiles/dropna_pack_timing.py [--runs 21] [--out profiles/dropna_pack_timing.md]
"""
import argparse
import hashlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAT = -2 ** 63


def quartiles(ms):
    q = statistics.quantiles(ms, n=4)
    return statistics.median(ms), q[0], q[2]


def fmt(ms):
    return "%.3f (%.3f .. %.3f)" % quartiles(ms)


class Bench:
    def __init__(self, torch, _native, B, n, C, dtype, channels_last, rate):
        self.torch, self.native = torch, _native
        dev = torch.device("cuda:0")
        gen = torch.Generator(device=dev).manual_seed(7)
        shape = (B, n, C) if channels_last else (B, C, n)
        clean = torch.randn(shape, generator=gen, device=dev, dtype=torch.float32).to(dtype)
        gaps = clean.clone()
        if rate > 0:
            drop = torch.rand((B, n), generator=gen, device=dev) < rate
            drop[:, 0] = False                                     # no series is emptied
            kind = torch.randint(0, C, (B, n), generator=gen, device=dev)
            hit = drop[:, :, None] & (kind[:, :, None] == torch.arange(C, device=dev)) if channels_last else \
                drop[:, None, :] & (kind[:, None, :] == torch.arange(C, device=dev)[None, :, None])
            gaps[hit] = float("nan")
        self.clean3 = clean.permute(0, 2, 1) if channels_last else clean
        self.gaps3 = gaps.permute(0, 2, 1) if channels_last else gaps
        self.t = 1_600_000_000 * 10 ** 9 + torch.randint(1, 2 * 10 ** 9, (B, n), generator=gen, device=dev, dtype=torch.int64).cumsum(dim=1)
        self.B, self.n, self.C = B, n, C
        self.x_type = {torch.float32: _native.TSFA_F32, torch.bfloat16: _native.TSFA_BF16}[dtype]
        self.in_size = clean.element_size()
        self.values = torch.empty((C, B * n), dtype=torch.float32, device=dev)
        self.offsets = torch.empty(B + 1, dtype=torch.int64, device=dev)
        self.steps = torch.empty(B * n, dtype=torch.int32, device=dev)
        self.stamps = torch.empty((B, n), dtype=torch.int64, device=dev)
        self.hours = torch.empty(B * n, dtype=torch.float64, device=dev)
        self.scratch_bytes = _native.pack_dense_valid_scratch_bytes(B, n)
        self.scratch = torch.empty(self.scratch_bytes // 8, dtype=torch.int64, device=dev)
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self.side = torch.cuda.current_stream()
        self.stream = self.side.cuda_stream

    def valid(self, timed):
        nv = self.native
        kw = dict(t_ptr=self.t.data_ptr(), t_type=nv.TSFA_I64, t_strides=self.t.stride(), stamps_ptr=self.stamps.data_ptr()) if timed else {}
        nv.pack_dense_valid(self.gaps3.data_ptr(), self.x_type, tuple(self.gaps3.shape), self.gaps3.stride(), self.values.data_ptr(),
                            self.B * self.n, self.offsets.data_ptr(), self.steps.data_ptr(), self.scratch.data_ptr(), self.scratch_bytes,
                            self.flag.data_ptr(), device=0, stream=self.stream, **kw)
        if timed:
            nv.pack_times(self.stamps.data_ptr(), nv.TSFA_I64, 10 ** 9, (self.B, self.n), (self.n, 1), self.offsets.data_ptr(),
                          self.hours.data_ptr(), self.flag.data_ptr(), device=0, stream=self.stream)

    def dense(self, timed, x3=None, t=None, lengths=None):
        nv = self.native
        x3 = self.clean3 if x3 is None else x3
        t = self.t if t is None else t
        kw = {} if lengths is None else dict(lengths_ptr=lengths.data_ptr(), lengths_type=nv.TSFA_I64)
        nv.pack_dense(x3.data_ptr(), self.x_type, tuple(x3.shape), x3.stride(), self.values.data_ptr(), self.B * self.n,
                      self.offsets.data_ptr(), self.flag.data_ptr(), device=0, stream=self.stream, **kw)
        if timed:
            nv.pack_times(t.data_ptr(), nv.TSFA_I64, 10 ** 9, (self.B, self.n), t.stride(), self.offsets.data_ptr(), self.hours.data_ptr(),
                          self.flag.data_ptr(), device=0, stream=self.stream)

    def composed(self):
        """What a user writes today: compact by hand into a right-padded batch plus lengths, then the existing packers."""
        torch = self.torch
        x3 = self.gaps3
        bad = torch.isnan(x3).any(dim=1) | (self.t == NAT)
        order = torch.argsort(bad.to(torch.uint8), dim=1, stable=True)   # kept steps first, in their order
        lengths = (~bad).sum(dim=1)
        xc = torch.gather(x3, 2, order[:, None, :].expand(-1, self.C, -1))
        tc = torch.gather(self.t, 1, order)
        self.dense(True, xc, tc, lengths)

    def time(self, fn):
        a, b = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def rounds(self, legs, runs):
        out = [[] for _ in legs]
        with self.torch.cuda.stream(self.side):   # the stream the batch was made on, and whose handle the library calls get
            for _ in range(3):
                for fn in legs:
                    self.time(fn)
            for _ in range(runs):
                for k, fn in enumerate(legs):
                    out[k].append(self.time(fn))
        self.side.synchronize()
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dropna_pack_timing.md"))
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the batch sizes (rehearsals)")
    args = ap.parse_args()
    if args.runs < 20:
        ap.error("--runs must be at least 20")
    import torch

    from tsfresh_amd import _native
    if _native.device_count() < 1:
        raise SystemExit("dropna_pack_timing.py needs a HIP device: nothing is measured without one")
    with open(_native.LIB_PATH, "rb") as f:
        build = hashlib.sha256(f.read()).hexdigest()[:16]
    lines = ["# The valid-step packer (`nan_policy=\"drop\"`): timing", "",
             "Written by `profiles/dropna_pack_timing.py` on %s, one process, one device; library build id "
             "(sha256(libtsfresh_amd.so)[:16]) `%s`.  HIP events on torch's current stream, 3 warm-up rounds, %d timed rounds with "
             "the legs of a row alternating; median (lower quartile .. upper quartile) in milliseconds." % (
                 torch.cuda.get_device_name(0), build, args.runs), ""]
    alone = ["## 1. The packers alone (no clock)", "",
             "GB/s counts the samples read once plus the samples written (float32 out); the valid-step packer reads the samples "
             "twice and also writes 4 bytes of step index per kept step, which the figure does not credit.", "",
             "| batch | dropped | `tsfa_pack_dense_valid` ms | GB/s | `tsfa_pack_dense` (no NaN) ms | GB/s | ratio |", "|---|---|---|---|---|---|---|"]
    whole = ["## 2. Packed samples + hours, with a (B, n) int64 clock", "",
             "drop: `tsfa_pack_dense_valid` + `tsfa_pack_times`; (a): `tsfa_pack_dense` + `tsfa_pack_times` on the batch without "
             "NaN; (b): isnan / any, a stable per-row argsort of the mask, gathers of every kind and the stamps, the kept counts, "
             "then (a)'s two calls with `lengths`.", "",
             "| batch | dropped | drop ms | (a) ms | (b) ms | drop / (a) | (b) / drop |", "|---|---|---|---|---|---|---|"]
    shapes = (("%d x 1024 float32, one kind", int(100000 * args.scale), 1, torch.float32, False),
              ("%d x 1024 x 8 bfloat16, channels-last", int(12500 * args.scale), 8, torch.bfloat16, True))
    side = torch.cuda.Stream()   # not the null stream: the library calls only enqueue, the events bracket the kernels
    for label, B, C, dtype, channels_last in shapes:
        for rate in (0.0, 0.01, 0.30):
            with torch.cuda.stream(side):
                bench = Bench(torch, _native, B, 1024, C, dtype, channels_last, rate)
            side.synchronize()
            name = label % B
            v, d = bench.rounds([lambda: bench.valid(False), lambda: bench.dense(False)], args.runs)
            bench.valid(False)
            torch.cuda.synchronize()
            kept = int(bench.offsets[-1].item())
            assert int(bench.flag.item()) == 0
            total = B * 1024
            gb_valid = C * (total * bench.in_size + kept * 4) / 1e6
            gb_dense = C * total * (bench.in_size + 4) / 1e6
            mv, md = statistics.median(v), statistics.median(d)
            alone.append("| %s | %.1f %% (%.2f %% measured) | %s | %.0f | %s | %.0f | %.2f |" % (
                name, rate * 100, 100.0 * (total - kept) / total, fmt(v), gb_valid / mv, fmt(d), gb_dense / md, mv / md))
            v, a, b = bench.rounds([lambda: bench.valid(True), lambda: bench.dense(True), bench.composed], args.runs)
            mv, ma, mb = statistics.median(v), statistics.median(a), statistics.median(b)
            whole.append("| %s | %.1f %% | %s | %s | %s | %.2f | %.2f |" % (name, rate * 100, fmt(v), fmt(a), fmt(b), mv / ma, mb / mv))
            del bench
            torch.cuda.empty_cache()
    lines += alone + [""] + whole + [""]
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
