#!/usr/bin/env python
"""The kernel launches of the device packer's two entries, to compare two builds of the library launch by launch.

Without arguments it packs four frames and nothing else: a shuffled frame of 2 * TILE + 1 rows and an in-order frame of 1000
rows, each once through `_native.DevicePack` (tsfa_pack_device) and once through a `_native.DevicePackSet` with three
interleaved kinds and one value column (tsfa_pack_set_create, tsfa_pack_set_values).  Run it under the kernel trace, once
per library (TSFA_LIB names the other build), as a run of its own:
    rocprofv3 --kernel-trace --output-format csv -d out/a -o p -- python profiles/pack_sorter_launches.py
    TSFA_LIB=/path/to/other/libtsfresh_amd.so rocprofv3 --kernel-trace --output-format csv -d out/b -o p -- python ...
    python profiles/pack_sorter_launches.py --compare out/a out/b
--compare reads the two *_kernel_trace.csv files, cuts each dispatch list at k_pack_minmax (the first launch of either
entry: four calls) and prints, per call, the ordered (kernel, grid, workgroup) list and whether the two builds agree; it
exits 1 when they do not.  The runtime's copy kernels (device-side hipMemcpy) are in the lists too; those that stage a
call's columns run before its k_pack_minmax and so close the list of the call before.
"""
import csv
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TILE = 4096
CALLS = ("DevicePack, shuffled", "DevicePackSet, shuffled", "DevicePack, in order", "DevicePackSet, in order")


def pack_four_frames():
    import numpy as np

    from tsfresh_amd import _native
    rng = np.random.default_rng(1)
    n = 2 * TILE + 1
    shuffled = (rng.integers(0, 300, n).astype(np.int64), rng.permutation(n).astype(np.int64))
    # 10 ids of 100 stamps in (id, sort) order; with the kinds interleaved the set has only its kind passes left
    in_order = (np.repeat(np.arange(10, dtype=np.int64), 100), np.tile(np.arange(100, dtype=np.int64), 10))
    for ids, sort in (shuffled, in_order):
        kinds = np.arange(len(ids), dtype=np.int64) % 3
        values = rng.standard_normal(len(ids)).astype(np.float32)
        cols = [_native.pack_column(a) for a in (ids, sort, kinds, values)]
        pack = _native.DevicePack(cols[0], cols[1], cols[3], keep_sort=True)
        print("DevicePack: rows %d series %d passes %d in_order %d" % (pack.n_rows, pack.n_series, pack.n_passes, pack.was_in_order))
        pack.close()
        pset = _native.DevicePackSet(cols[0], cols[1], cols[2], keep_sort=True)
        packs = pset.values(cols[3])
        print("DevicePackSet: rows %d kinds %d passes %d in_order %d" % (pset.n_rows, pset.n_kinds, pset.n_passes, pset.was_in_order))
        for p in packs:
            p.close()
        pset.close()


def launches(directory):
    """The dispatches of one trace in start order -> [[(kernel, grid, workgroup)] per call]."""
    paths = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if len(paths) != 1:
        raise SystemExit("%s: expected one *kernel_trace.csv, found %d" % (directory, len(paths)))
    with open(paths[0], newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    calls = [[]]
    for r in rows:
        m = re.search(r"\bk_\w+", r["Kernel_Name"])
        name = m.group(0) if m else r["Kernel_Name"]   # (the runtime's own copy and fill kernels are listed as they ran)
        if name == "k_pack_minmax" and any(k.startswith("k_") for k, _, _ in calls[-1]):
            calls.append([])
        calls[-1].append((name, tuple(int(r["Grid_Size_" + a]) for a in "XYZ"), tuple(int(r["Workgroup_Size_" + a]) for a in "XYZ")))
    return calls


def compare(dir_a, dir_b):
    a, b = launches(dir_a), launches(dir_b)
    same = len(a) == len(b) == len(CALLS)
    for k, call in enumerate(a):
        agree = k < len(b) and call == b[k]
        same = same and agree
        print("\n%s: %d launches, %s" % (CALLS[k] if k < len(CALLS) else "call %d" % k, len(call), "identical" if agree else "DIFFERENT"))
        for i, (name, grid, wg) in enumerate(call):
            other = "" if agree else "    | " + (str(b[k][i]) if k < len(b) and i < len(b[k]) else "-")
            print("  %-22s grid %-16s workgroup %s%s" % (name, grid, wg, other))
    print("\n" + ("identical: %d calls" % len(a) if same else "the two builds DIFFER"))
    return 0 if same else 1


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    pack_four_frames()
