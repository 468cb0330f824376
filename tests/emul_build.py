"""Test helper: the one build recipe of the tests/emul*_lib.py helpers -- the g++ build of a tests/emul/*.cpp driver over the
kernel sources, rebuilt when it is older than anything it may include.

TEST INFRASTRUCTURE ONLY.  The product never imports this.
"""
import glob
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# every helper module; each has SRC, LIB and a load() that builds (here) and binds its library
LIBS = ("emul_lib", "emul_pack_lib", "emul_pack_set_lib", "emul_pack_rows_lib", "emul_pack_dense_lib", "emul_pack_times_lib",
        "emul_pack_valid_lib", "emul_roll_lib", "emul_roll_dense_lib", "emul_mprofile_lib", "emul_sort_lib", "emul_rel_tails_lib",
        "emul_rel_ks_lib")


def build(src, lib):
    """Compile `src` into the shared library `lib` unless `lib` is newer than `src`, the C header, every kernel header and
    every header the drivers share (tests/emul/*.h)."""
    deps = [src, os.path.join(ROOT, "include", "tsfresh_amd.h")] + glob.glob(os.path.join(ROOT, "tsfresh_amd", "csrc", "*.h")) \
        + glob.glob(os.path.join(HERE, "emul", "*.h"))
    if os.path.exists(lib) and all(os.path.getmtime(d) <= os.path.getmtime(lib) for d in deps):
        return
    tmp = "%s.%d.tmp" % (lib, os.getpid())  # atomic: several processes (the gloo test's ranks) may build at once
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-DTSFA_EMUL", src, "-o", tmp])
    os.replace(tmp, lib)
