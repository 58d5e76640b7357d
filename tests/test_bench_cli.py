"""bench.py's command line: a plain run prints the timed loop's line only, `--full` adds the legs
that take runs of their own, and `--dump-outputs DIR` writes the last timed step's outputs, the same
from run to run (seeded inputs, deterministic kernels), within its size cap."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

NAMES = ("z", "kkt", "iters", "status", "x0", "u_prev", "traj_all")


def test_dump_outputs_is_float64_and_keeps_a_seeded_sample_under_the_cap(tmp_path):
    import torch

    g = torch.Generator().manual_seed(3)
    t = {"z": torch.randn(1000, 300, dtype=torch.float64, generator=g), "iters": torch.arange(1000, dtype=torch.int32),
         "traj_all": torch.randn(2000, 31, 2, dtype=torch.float64, generator=g)}
    bench.dump_outputs(str(tmp_path / "all"), "", t)           # under the cap: everything, no row files
    assert sorted(os.listdir(tmp_path / "all")) == ["iters.npy", "traj_all.npy", "z.npy"]
    z = np.load(tmp_path / "all" / "z.npy")
    assert z.dtype == np.float64 and np.array_equal(z, t["z"].numpy())
    assert np.array_equal(np.load(tmp_path / "all" / "iters.npy"), np.arange(1000.0))
    cap = 10**6
    for rep in ("a", "b"):
        bench.dump_outputs(str(tmp_path / rep), "", t, cap=cap)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted([f"{k}.npy" for k in t] + [f"{k}_rows.npy" for k in t])
    assert sum(np.load(tmp_path / "a" / f).nbytes for f in files) <= cap
    for f in files:   # the same sample in every run
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
    for k, v in t.items():
        rows = np.load(tmp_path / "a" / f"{k}_rows.npy").astype(int)
        assert len(rows) > 100 and np.array_equal(np.load(tmp_path / "a" / f"{k}.npy"), v.numpy()[rows])


def _run(monkeypatch, capsys, argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "CMPC_DEVICE", "CMPC_DIST_BACKEND"):
        monkeypatch.delenv(k, raising=False)
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_lean_full_adds_its_legs_and_dumps_agree(monkeypatch, capsys, tmp_path):
    common = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--agents", "96"]
    a = _run(monkeypatch, capsys, common + ["--dump-outputs", str(tmp_path / "a")])
    assert a["steps"] == 3 and a["full"] is False and a["ms_per_step"] > 0 and a["unsolved"] == 0
    assert a["value"] == pytest.approx(96 * 1e3 / a["ms_per_step"])
    for k in ("metric", "unit", "higher_is_better", "dtype", "roofline"):
        assert a[k] is not None
    for k in ("cpu_baseline", "max_abs_err_vs_cpu", "cfg5", "reference_config", "osqp_dropin", "fp32_vs_fp64"):
        assert a[k] is None, k
    b = _run(monkeypatch, capsys, common + ["--full", "--no-ref", "--no-cfg5", "--cpu-seconds", "0.05",
                                            "--dump-outputs", str(tmp_path / "b")])
    assert b["full"] is True and b["cpu_baseline"]["value"] > 0 and b["max_abs_err_vs_cpu"] < 1e-6
    assert b["reference_config"] is None and b["cfg5"] is None
    assert sorted(os.listdir(tmp_path / "a")) == sorted(f"{k}.npy" for k in NAMES)
    for k in NAMES:   # the dump is the timed path's, taken before --full's legs advance the rounds further
        x, y = np.load(tmp_path / "a" / f"{k}.npy"), np.load(tmp_path / "b" / f"{k}.npy")
        assert x.dtype == np.float64 and x.shape[0] == 96 and np.array_equal(x, y), k
    assert np.isfinite(np.load(tmp_path / "a" / "z.npy")).all()
    assert np.isin(np.load(tmp_path / "a" / "status.npy"), (1.0, 2.0)).all()   # solved / solved-inaccurate
