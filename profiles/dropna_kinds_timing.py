#!/usr/bin/env python
"""Timing of the per-kind valid-step packer (tsfa_pack_dense_valid_kinds, `nan_policy="drop_per_kind"`), on one device, in
one process: writes profiles/dropna_kinds_timing.md.  The method is that of profiles/dropna_pack_timing.py.

Three batches -- 100 000 x 1024 float32 with one kind and with four ([B, C, n]) and 12 500 x 1024 x 8 channels-last bfloat16
([B, n, C]) --, each with 0 %, 1 % and 30 % of the samples NaN, placed per (kind, step); step 0 of every row stays.

1. The packers alone: `tsfa_pack_dense_valid_kinds` next to `tsfa_pack_dense_valid` on the same batch (the two keep
   different steps: the wide rule drops a step for every kind).
2. The entry, `extract_features_tensor(nan_policy="drop_per_kind")`, next to what a user writes today: per kind the isnan
   mask, a stable per-row argsort, a gather, the kept counts as `lengths`, and one `extract_features_tensor` call --
   under `MinimalFCParameters`, so that the packing is not lost in the extraction.

Every leg runs between two HIP events on torch's current stream, after 3 warm-up rounds; the legs of one table row alternate
for --runs rounds; median and quartiles in milliseconds.

    python profiles/dropna_kinds_timing.py [--runs 21] [--resources FILE] [--out profiles/dropna_kinds_timing.md]

--resources: the output of `python profiles/kernel_resources.py valid_kinds tsfa_pack_valid_kinds.hip`, appended as section 3.
"""
import argparse
import hashlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fmt(ms):
    q = statistics.quantiles(ms, n=4)
    return "%.3f (%.3f .. %.3f)" % (statistics.median(ms), q[0], q[2])


class Bench:
    def __init__(self, torch, _native, B, n, C, dtype, channels_last, rate):
        self.torch, self.native = torch, _native
        dev = torch.device("cuda:0")
        gen = torch.Generator(device=dev).manual_seed(7)

        def batch(steps):
            x = torch.randn((B, steps, C) if channels_last else (B, C, steps), generator=gen, device=dev, dtype=torch.float32).to(dtype)
            if rate > 0:
                x[torch.rand(x.shape, generator=gen, device=dev) < rate] = float("nan")
            x3 = x.permute(0, 2, 1) if channels_last else x
            x3[:, :, 0] = 1.0                                     # no (series, kind) is emptied
            return x3
        self.x3 = batch(n)
        self.B, self.n, self.C = B, n, C
        self.x_type = {torch.float32: _native.TSFA_F32, torch.bfloat16: _native.TSFA_BF16}[dtype]
        self.in_size = self.x3.element_size()
        self.values = torch.empty((C, B * n), dtype=torch.float32, device=dev)
        self.offsets = torch.empty((C, B + 1), dtype=torch.int64, device=dev)
        self.steps = torch.empty((C, B * n), dtype=torch.int32, device=dev)
        self.scratch_bytes = _native.pack_dense_valid_scratch_bytes(B * C, n)
        self.scratch = torch.empty(self.scratch_bytes // 8, dtype=torch.int64, device=dev)
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self.side = torch.cuda.current_stream()

    def pack(self, fn, x3):
        fn(x3.data_ptr(), self.x_type, tuple(x3.shape), x3.stride(), self.values.data_ptr(), self.B * self.n, self.offsets.data_ptr(),
           self.steps.data_ptr(), self.scratch.data_ptr(), self.scratch_bytes, self.flag.data_ptr(), device=0, stream=self.side.cuda_stream)

    def kinds(self):
        self.pack(self.native.pack_dense_valid_kinds, self.x3)

    def wide(self):
        self.pack(self.native.pack_dense_valid, self.x3)

    def entry(self):
        from tsfresh_amd import MinimalFCParameters, extract_features_tensor
        return extract_features_tensor(self.x3, default_fc_parameters=MinimalFCParameters(), nan_policy="drop_per_kind")[0]

    def composed(self):
        """What a user writes today: compact every kind by hand into a right-padded batch plus lengths, one call per kind."""
        from tsfresh_amd import MinimalFCParameters, extract_features_tensor
        torch, out = self.torch, []
        for c in range(self.C):
            xc = self.x3[:, c]
            bad = torch.isnan(xc)
            order = torch.argsort(bad.to(torch.uint8), dim=1, stable=True)   # kept steps first, in their order
            out.append(extract_features_tensor(torch.gather(xc, 1, order), lengths=(~bad).sum(dim=1),
                                               default_fc_parameters=MinimalFCParameters())[0])
        return torch.cat(out, dim=1)

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dropna_kinds_timing.md"))
    ap.add_argument("--resources", default=None)
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the batch sizes (rehearsals)")
    args = ap.parse_args()
    if args.runs < 20:
        ap.error("--runs must be at least 20")
    import torch

    from tsfresh_amd import _native
    if _native.device_count() < 1:
        raise SystemExit("dropna_kinds_timing.py needs a HIP device: nothing is measured without one")
    with open(_native.LIB_PATH, "rb") as f:
        build = hashlib.sha256(f.read()).hexdigest()[:16]
    lines = ["# The per-kind valid-step packer (`nan_policy=\"drop_per_kind\"`): timing", "",
             "Written by `profiles/dropna_kinds_timing.py` on %s, one process, one device; library build id "
             "(sha256(libtsfresh_amd.so)[:16]) `%s`.  HIP events on torch's current stream, 3 warm-up rounds, %d timed rounds with "
             "the legs of a row alternating; median (lower quartile .. upper quartile) in milliseconds.  NaN are placed per (kind, "
             "step)." % (torch.cuda.get_device_name(0), build, args.runs), ""]
    alone = ["## 1. The packers alone", "",
             "GB/s of the new packer counts the samples read once plus the kept samples and step indices written (4 + 4 bytes); it "
             "reads the samples twice, which the figure does not credit.  The wide packer keeps fewer steps (a step goes for every "
             "kind), so with several kinds and NaN it writes less.", "",
             "| batch | NaN | `tsfa_pack_dense_valid_kinds` ms | GB/s | kept | `tsfa_pack_dense_valid` ms | kept | ratio |",
             "|---|---|---|---|---|---|---|---|"]
    whole = ["## 2. The entry next to the composition a user writes today (`MinimalFCParameters`)", "",
             "entry: `extract_features_tensor(nan_policy=\"drop_per_kind\")`; composed: per kind isnan, a stable per-row argsort, a "
             "gather, the kept counts as `lengths`, one `extract_features_tensor` call.  The two matrices are compared before they are timed.", "",
             "| batch | NaN | entry ms | composed ms | composed / entry | equal |", "|---|---|---|---|---|---|"]
    shapes = (("%d x 1024 float32, one kind", int(100000 * args.scale), 1, torch.float32, False),
              ("%d x 4 x 1024 float32", int(100000 * args.scale), 4, torch.float32, False),
              ("%d x 1024 x 8 bfloat16, channels-last", int(12500 * args.scale), 8, torch.bfloat16, True))
    side = torch.cuda.Stream()   # not the null stream: the library calls only enqueue, the events bracket the kernels
    for label, B, C, dtype, channels_last in shapes:
        for rate in (0.0, 0.01, 0.30):
            with torch.cuda.stream(side):
                bench = Bench(torch, _native, B, 1024, C, dtype, channels_last, rate)
            side.synchronize()
            name, total = label % B, B * 1024 * C
            k, w = bench.rounds([bench.kinds, bench.wide], args.runs)
            bench.wide()
            torch.cuda.synchronize()
            kept_wide = C * int(bench.offsets[0, -1].item())
            bench.kinds()
            torch.cuda.synchronize()
            kept = int(bench.offsets[:, -1].sum().item())
            assert int(bench.flag.item()) == 0
            mk, mw = statistics.median(k), statistics.median(w)
            alone.append("| %s | %.0f %% | %s | %.0f | %.2f %% | %s | %.2f %% | %.2f |" % (
                name, rate * 100, fmt(k), (total * bench.in_size + kept * 8) / 1e6 / mk, 100.0 * kept / total, fmt(w),
                100.0 * kept_wide / total, mk / mw))
            with torch.cuda.stream(side):
                same = torch.equal(bench.entry(), bench.composed())
            e, c = bench.rounds([bench.entry, bench.composed], args.runs)
            whole.append("| %s | %.0f %% | %s | %s | %.2f | %s |" % (name, rate * 100, fmt(e), fmt(c), statistics.median(c) / statistics.median(e),
                                                                  "yes" if same else "NO"))
            print(alone[-1], whole[-1], sep="\n", flush=True)
            del bench
            torch.cuda.empty_cache()
    lines += alone + [""] + whole + [""]
    if args.resources:
        with open(args.resources) as f:
            lines += ["## 3. Resources, as the compiler reports them", "",
                      "`python profiles/kernel_resources.py valid_kinds tsfa_pack_valid_kinds.hip` (template arguments: `Li0` float32, "
                      "`Li1` float64, `Li11` float16, `Li12` bfloat16; `Lb1` unit time stride).  No kernel spills.", "", "```",
                      f.read().rstrip(), "```", ""]
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
