"""Device memory goes with its owner (csrc/tsfa_devmem.h): plans, the selection statistics, a window set refused after its
first allocation, and a plain pack, each cycled in a fresh child process (torch imported first so that
torch.cuda.mem_get_info and the library see one HIP runtime, as in tests/test_pack_device.py).  Free device memory after the
last cycle equals the value after the second, and -- the positive control, so that "equal" cannot hide behind the allocator's
granularity -- it is lower while one more object of the same kind is held open."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

_PROLOGUE = r"""
import sys
import numpy as np
import torch   # first: torch ships its own HIP runtime and must be the one that opens the device in this process
torch.cuda.init()
sys.path.insert(0, %(root)r)
from tsfresh_amd import _native

def free():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]
"""

_PLAN_SCRIPT = _PROLOGUE + r"""
from tsfresh_amd.feature_extraction.plan import compile_fc_parameters
# One column of the BASIC, SORT, ENTROPY, AR, SPECTRAL, SEQ and CWT families each, in two plans that between them hold most of
# a plan's buffers.  No single plan can: force_long switches the symbol-rows route of lempel_ziv_complexity off, and a calculator
# goes either to its tuned kernel or to k_general.
#   "long": every family through its HBM-scratch build (long_scratch); number_cwt_peaks within the tables (k_cwtpeaks).
#           seq_rows = 1 is set as well, but force_long wins: plan->seq_rows stays empty here.
#   "rows": the LDS builds with lempel_ziv_complexity's symbol rows in HBM (plan->seq_rows, the buffer that once leaked), and
#           number_cwt_peaks beyond the tables' 16 widths, so k_general runs (gen_scratch, d_gen_specs).
base = {"mean": None, "quantile": [{"q": 0.3}], "sample_entropy": None, "ar_coefficient": [{"coeff": 1, "k": 10}],
        "fft_coefficient": [{"coeff": 1, "attr": "abs"}], "lempel_ziv_complexity": [{"bins": 10}]}
specs = {"long": compile_fc_parameters(dict(base, number_cwt_peaks=[{"n": 5}])).native_specs(_native.calc_id),
         "rows": compile_fc_parameters(dict(base, number_cwt_peaks=[{"n": 17}])).native_specs(_native.calc_id)}
n_series, length = 4096, 256
values = np.random.default_rng(3).standard_normal(n_series * length)
offsets = np.arange(n_series + 1, dtype=np.int64) * length
out = np.empty((n_series, len(specs["long"])))

def run(kind):
    plan = _native.Plan(specs[kind])
    plan.set_option("seq_rows", 1)
    if kind == "long":
        plan.set_option("force_long", 1)
    plan.set_profiling(True)            # the timing events exist
    plan.extract_host(values, offsets, out=out)
    assert np.isfinite(out[:, 0]).all()
    launches, timed = plan.last_launches(), [name for name, _ in plan.last_timings()]
    seq = [l for l in launches if l["family"] == "SEQ"]
    assert len(seq) == 1 and ("CWT" in {l["family"] for l in launches}) == (kind == "long"), launches
    if kind == "long":
        assert all(l["long_build"] == 1 for l in launches) and "k_general" not in timed, (launches, timed)
    else:   # bit 8 of the SEQ variant: the symbol rows are in HBM
        assert (seq[0]["variant"] >> 8) & 1 and not seq[0]["long_build"] and "k_general" in timed, (launches, timed)
    return plan

seen = []
for cycle in range(8):                  # long, rows, long, rows, ...: four cycles of each kind
    run("rows" if cycle & 1 else "long").close()
    seen.append(free())
held = []
for kind in ("long", "rows"):           # the positive control, one plan open at a time as in the cycles
    plan = run(kind)
    held.append(free())
    plan.close()
    seen.append(free())
print("FREE", seen, held)
# the first cycle of EACH kind loads the code objects of the kernels only that kind launches (k_general, the rows build of
# k_seq): seen[3] is the value after the second cycle of the later kind, and from there on every cycle of either kind is flat
assert len(set(seen[3:])) == 1, seen
assert max(held) < seen[7], (held, seen)
print("MEMORY_OK")
"""

_SELECT_SCRIPT = _PROLOGUE + r"""
from tsfresh_amd.feature_selection.significance_tests import target_tie_statistics
n, m, T = 2048, 256, 3
rng = np.random.default_rng(5)
X = np.round(rng.standard_normal((n, m)), 2)
X[:, ::7] = (X[:, ::7] > 0)                       # binary columns: the Fisher cells
codes = rng.integers(0, T, n).astype(np.int32)
y = rng.standard_normal(n)
holes = X.copy()
holes[::5, ::3] = np.nan
holes[1::9, 1::4] = np.inf
# the tails and FDR entry points take device pointers only: their matrix and outputs are made once, before anything is
# measured.  The staged copy of a host matrix (d.dX) is what relevance_classes, relevance_real and impute_matrix allocate.
dev = torch.device("cuda:0")
Xd = torch.as_tensor(X, device=dev)
p, p1 = (torch.empty((m, k), dtype=torch.float64, device=dev) for k in (T, 1))
routes, routes1 = (torch.empty((m, k), dtype=torch.uint8, device=dev) for k in (T, 1))
types, types1, relevant = (torch.zeros(m, dtype=torch.uint8, device=dev) for _ in range(3))
rel_table = torch.zeros((m, T), dtype=torch.uint8, device=dev)
n_sig = torch.zeros(m, dtype=torch.int32, device=dev)
p_min = torch.empty(m, dtype=torch.float64, device=dev)

def run():
    assert len(_native.relevance_classes(X, codes, T, with_ks=True)) == 7
    assert len(_native.relevance_real(X, y)[0]) == m
    torch.cuda.synchronize()
    _native.relevance_tails_classes(Xd.data_ptr(), n, m, m, codes, T, p.data_ptr(), routes.data_ptr(), types.data_ptr(), with_ks=True)
    _native.relevance_tails_real(Xd.data_ptr(), n, m, m, y, target_tie_statistics, p1.data_ptr(), routes1.data_ptr(), types1.data_ptr())
    _native.relevance_fdr(p.data_ptr(), types.data_ptr(), m, T, 0.05, 1.0, 1, False, rel_table.data_ptr(), relevant.data_ptr(),
                          n_sig.data_ptr(), p_min.data_ptr())
    filled = holes.copy()
    _native.impute_matrix(filled)
    assert np.isfinite(filled).all()

seen = []
for _ in range(6):
    run()
    seen.append(free())
buf = _native._DeviceBuffer(_native.load(), X, 0)   # 4 MB held open
run()
held = free()
buf.free()
print("FREE", seen, held, free())
assert seen[5] == seen[1], seen
assert held < seen[5], (held, seen)
assert free() == seen[1]
print("MEMORY_OK")
"""

_REFUSAL_SCRIPT = _PROLOGUE + r"""
n_series = 1 << 20                                  # two rows each: the window builder's count array is 4 MB
ids = _native.pack_column(np.repeat(np.arange(n_series, dtype=np.int64), 2))
sort = _native.pack_column(np.tile(np.arange(2, dtype=np.int64), n_series))
values = _native.pack_column(np.ones(2 * n_series, dtype=np.float32))
pack = _native.DevicePack(ids, sort, values)
assert pack.n_series == n_series
seen = []
for _ in range(6):
    try:
        _native.DeviceWindows(pack, steps=1)        # refused after the counts were allocated and computed
        raise AssertionError("steps = 1 below series of two samples was accepted")
    except _native.NativeError as e:
        assert "is below the pack's longest series (2 samples)" in str(e), e
    seen.append(free())
windows = _native.DeviceWindows(pack)
assert windows.n_windows == 2 * n_series
held = free()
windows.close()
print("FREE", seen, held, free())
assert seen[5] == seen[1], seen
assert held < seen[5], (held, seen)
assert free() == seen[1]
print("MEMORY_OK")
"""

_PACK_SCRIPT = _PROLOGUE + r"""
n = 1 << 20
rng = np.random.default_rng(9)
ids_a, sort_a = rng.integers(0, 4096, n), rng.permutation(n)
vals_a = rng.standard_normal(n).astype(np.float32)
ids, sort, values = (_native.pack_column(a) for a in (ids_a, sort_a, vals_a))
order = np.lexsort((sort_a, ids_a))

def run():
    pack = _native.DevicePack(ids, sort, values, keep_sort=True)
    # read after construction: the buffers the pack now shares with nobody are the ones the sort filled
    assert np.array_equal(pack.values_host(), vals_a[order]) and np.array_equal(pack.sort, sort_a[order])
    assert np.array_equal(pack.ids, np.unique(ids_a)) and np.array_equal(pack.offsets, np.searchsorted(ids_a[order], np.arange(4097)))
    return pack

run().close()   # (first use: the runtime's own one-time allocations)
start = free()
pack = run()
held = free()
pack.close()
print("FREE", start, held, free())
assert held < start, (held, start)
assert free() == start
print("MEMORY_OK")
"""


@pytest.mark.parametrize("script", [_PLAN_SCRIPT, _SELECT_SCRIPT, _REFUSAL_SCRIPT, _PACK_SCRIPT],
                         ids=["plan", "selection_statistics", "windows_refused_after_allocation", "plain_pack"])
def test_free_device_memory_is_flat_over_cycles_and_lower_while_held(gpu, script):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", script % {"root": root}], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "MEMORY_OK" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]
