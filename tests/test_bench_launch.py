"""bench.py starts its own ranks when `--gpus N` is given without a launcher: `python bench.py --gpus 8`
has the shape of the recorded N = 1 command, so the scaling run needs no wrapper.  The reference's counterpart is the
process pool of MultiprocessingDistributor (tsfresh/utilities/distribution.py:438-494)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_self_launch_command_for_eight_ranks():
    import bench
    port = bench.free_port()
    assert 1024 < port < 65536
    argv = ["--gpus", "8", "--steps", "5", "--warmup", "2"]
    cmd, env = bench.self_launch_command(8, argv, port)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nnodes=1" in cmd
    assert cmd[cmd.index("--nproc-per-node") + 1] == "8"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"      # the container hostname may not resolve
    assert cmd[cmd.index("--master-port") + 1] == str(port)
    script = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[script + 1:] == argv                                  # the ranks see the caller's flags unchanged
    assert env["HSA_ENABLE_IPC_MODE_LEGACY"] == "0" and env["TSFA_BENCH_LAUNCHED"] == "1"


def test_a_launched_rank_does_not_launch_again(monkeypatch):
    """Under a launcher (WORLD_SIZE set) main() goes on to the device check instead of spawning: no GPU here, so it
    stops with the 'needs a HIP device' message -- not with a subprocess."""
    import bench
    calls = []
    monkeypatch.setattr(subprocess, "call", lambda *a, **k: calls.append(a) or 0)
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    import torch
    if torch.cuda.is_available():
        pytest.skip("needs a box without a GPU")
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert "HIP device" in str(e.value) and not calls


def test_without_a_launcher_gpus_n_spawns_n_ranks(monkeypatch):
    import bench
    calls = []
    monkeypatch.setattr(subprocess, "call", lambda cmd, env=None: calls.append((cmd, env)) or 7)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 7 and len(calls) == 1                    # the job's exit code is handed back
    cmd, env = calls[0]
    assert cmd[cmd.index("--nproc-per-node") + 1] == "4" and cmd[-4:] == ["--gpus", "4", "--steps", "3"]


def test_strong_scaling_flag_reaches_the_ranks_unchanged():
    """`--strong --n-series TOTAL` (configs[3]: 1 M x 256 split over N): the self-launch hands the flag to every rank; a rank
    derives its share from WORLD_SIZE (bench.py main)."""
    import bench
    argv = ["--gpus", "8", "--strong", "--n-series", "1000000", "--length", "256"]
    cmd, _ = bench.self_launch_command(8, argv, 29999)
    assert cmd[-len(argv):] == argv


def test_configs4_as_a_strong_scaling_job_is_a_valid_command(capsys, monkeypatch):
    """BASELINE configs[4]: `bench.py --strong --ragged 4096:8192 --n-series 50000 --gpus 4 --params efficient`.  ONE length
    list for the job, shards of ~equal sum(len^2) and therefore UNEQUAL height -> the point-to-point exchange form
    (round-5 VERDICT "Next" #8b).  --plan-only prints the layout without a GPU."""
    import numpy as np

    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--strong", "--ragged", "4096:8192", "--n-series", "50000", "--gpus", "4",
                                      "--params", "efficient", "--plan-only"])
    bench.main()
    doc = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert doc["gpus"] == 4 and doc["scaling"] == "strong" and doc["exchange"] == "p2p"
    assert sum(doc["shard_rows"]) == 50000 and len(set(doc["shard_rows"])) > 1
    cost = np.array(doc["sum_len2"])
    assert cost.max() / cost.min() < 1.001                      # balanced on what the O(n^2) calculators cost
    # every rank derives the SAME layout (seeded), its own slice of it, and the launcher hands the flags through unchanged
    a = bench.strong_ragged_layout(50000, 4096, 8192, 4)
    b = bench.strong_ragged_layout(50000, 4096, 8192, 4)
    assert a["counts"] == b["counts"] == doc["shard_rows"] and np.array_equal(a["lens"], b["lens"])
    argv = ["--gpus", "4", "--strong", "--ragged", "4096:8192", "--n-series", "50000", "--params", "efficient"]
    cmd, _ = bench.self_launch_command(4, argv, 29998)
    assert cmd[-len(argv):] == argv
    # configs[3] stays the all-gather form: equal shards
    monkeypatch.setattr(sys, "argv", ["bench.py", "--strong", "--n-series", "1000000", "--length", "256", "--gpus", "8", "--plan-only"])
    bench.main()
    doc = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert doc["exchange"] == "all_gather" and doc["shard_rows"] == [125000] * 8


def test_dump_outputs_writes_the_matrix_or_a_fixed_sample_within_the_budget(tmp_path, monkeypatch):
    """--dump-outputs: the whole matrix when it fits, else the same seeded row sample for the same shape, under the byte
    budget; float64 throughout; the columns that are NaN by definition left out by name."""
    import numpy as np
    import torch

    import bench
    names = ["c%d" % j for j in range(7)]
    names[3] = "query_similarity_count__query_None__threshold_0.0"
    full = torch.arange(50 * 7, dtype=torch.float64).reshape(50, 7)
    full[:, 3] = float("nan")
    keep = [0, 1, 2, 4, 5, 6]
    doc = bench.dump_outputs(str(tmp_path / "all"), full, names)
    assert doc == {"dir": str(tmp_path / "all"), "rows": 50, "of_rows": 50, "cols": 6, "of_cols": 7,
                   "left_out": [names[3]], "nonfinite_cells": 0}
    got = np.load(tmp_path / "all" / "features.npy")
    assert got.dtype == np.float64 and np.array_equal(got, full.numpy()[:, keep]) and np.isfinite(got).all()
    assert np.array_equal(np.load(tmp_path / "all" / "rows.npy"), np.arange(50.0))
    assert np.array_equal(np.load(tmp_path / "all" / "cols.npy"), np.array(keep, dtype=np.float64))
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 3 * 4096 + 8 * 6 + 8 * 7 * 20)   # 20 rows of 6 columns + their row number
    for d in ("a", "b"):
        assert bench.dump_outputs(str(tmp_path / d), full, names)["rows"] == 20
    rows = np.load(tmp_path / "a" / "rows.npy")
    assert rows.dtype == np.float64 and np.array_equal(rows, np.load(tmp_path / "b" / "rows.npy"))
    assert np.all(np.diff(rows) > 0) and rows.max() < 50
    got = np.load(tmp_path / "a" / "features.npy")
    assert np.array_equal(got, full.numpy()[rows.astype(np.int64)][:, keep])
    files = ("features.npy", "rows.npy", "cols.npy")
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= bench.DUMP_MAX_BYTES


def test_steps_below_one_are_refused(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2


@pytest.mark.gpu
def test_bench_dumps_what_its_timed_step_computed(gpu, tmp_path):
    """The dump of a run holds the matrix of its timed steps: every row of the seeded input, and a few of them against the
    oracle."""
    import numpy as np

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from oracle.extract import oracle_matrix
    from parity import compare
    from tsfresh_amd import ComprehensiveFCParameters
    from tsfresh_amd.feature_extraction.plan import compile_fc_parameters
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    n, L = 3000, 256
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                          "--n-series", str(n), "--length", str(L), "--no-cpu-baseline", "--no-e2e",
                          "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    doc = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert doc["steps"] == 2 and doc["ms_per_step"] > 0
    left_out = ["query_similarity_count__query_None__threshold_0.0"]
    assert doc["dumped_outputs"] == {"dir": str(tmp_path), "rows": n, "of_rows": n, "cols": 782, "of_cols": 783,
                                     "left_out": left_out, "nonfinite_cells": 0}
    got = np.load(tmp_path / "features.npy")
    assert got.shape == (n, 782) and got.dtype == np.float64 and np.isfinite(got).all()
    assert np.array_equal(np.load(tmp_path / "rows.npy"), np.arange(float(n)))
    x = np.random.default_rng(42).standard_normal((n, L), dtype=np.float32)   # bench.py's input at rank 0
    pick = [0, 1, n // 2, n - 1]
    values = x[pick].astype(np.float64).reshape(-1)
    offsets = np.arange(len(pick) + 1, dtype=np.int64) * L
    params = ComprehensiveFCParameters()
    names, want = oracle_matrix(values, offsets, params)
    plan_cols = compile_fc_parameters(params).names
    cols = ["value__" + plan_cols[int(j)] for j in np.load(tmp_path / "cols.npy")]
    assert [c for c in plan_cols if "value__" + c not in cols] == left_out
    names, want = [c for c in names if c in cols], want[:, [names.index(c) for c in names if c in cols]]
    bad = compare(names, got[pick][:, [cols.index(c) for c in names]], want, [x[i].astype(np.float64) for i in pick])
    assert not bad, bad[:5]


@pytest.mark.gpu
def test_plain_bench_run_carries_only_the_headline(gpu):
    """Without --full a run prints the headline line and nothing that needs passes, pools or checks of its own: no
    per-kernel timings, roofline, parity sample, boundary timings or CPU baseline."""
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                          "--n-series", "2000", "--length", "256"], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    doc = json.loads(lines[0])
    assert doc["metric"] == "series/sec (comprehensive, len=256)" and doc["unit"] == "series/sec"
    assert doc["higher_is_better"] is True and doc["dtype"] == "f64"
    assert doc["steps"] == 2 and doc["warmup"] == 1 and doc["ms_per_step"] > 0
    assert abs(doc["value"] - 2000 * 1000.0 / doc["ms_per_step"]) <= 1e-6 * doc["value"]
    extras = {"kernel_ms", "outputs_finite", "roofline", "nonfinite_columns", "multi_gpu", "parity_sample", "e2e",
              "e2e_headline", "cpu_baseline"}
    assert not extras & set(doc), sorted(extras & set(doc))


@pytest.mark.gpu
def test_strong_ragged_bench_runs_on_one_gpu(gpu):
    """The same command at --gpus 1 on the device (a shard = the whole job): the layout code path, ragged lengths, one rank."""
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--strong", "--ragged", "300:700",
                          "--n-series", "3000", "--params", "efficient", "--steps", "2", "--warmup", "1", "--full",
                          "--no-cpu-baseline", "--no-e2e"], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    doc = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert doc["scaling"] == "strong" and doc["value"] > 0 and doc["outputs_finite"]


@pytest.mark.gpu
def test_bench_self_launch_path_on_one_gpu(gpu):
    """`python bench.py --gpus 1` THROUGH the self-launch path (torch.distributed.run, one rank, RCCL communicator of
    one): the JSON line comes back on stdout with the multi_gpu block saying what RCCL saw."""
    env = dict(os.environ, TSFA_BENCH_SELF_LAUNCH="1", TSFA_BENCH_FORCE_DIST="1")
    env.pop("WORLD_SIZE", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                          "--n-series", "2000", "--full", "--no-cpu-baseline", "--no-e2e"], env=env, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    doc = json.loads(lines[0])
    assert doc["n_gpus"] == 1 and doc["value"] > 0 and doc["outputs_finite"]
    assert doc["multi_gpu"]["world"] == 1 and doc["multi_gpu"]["ranks_seen_by_rccl"] == 1
    assert doc["multi_gpu"]["self_launched"] is True
    assert doc["parity_sample"] == "ok"
