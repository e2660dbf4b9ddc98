"""GPU: a plain `bench.py` run prints the headline figure only, and `--dump-outputs` writes what the timed path computed in
its last iteration -- the same arrays from run to run with the same arguments (seeded inputs), so that two builds can be
compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["costs.npy", "softmin.npy", "state.npy", "u_prev.npy", "waypoint_idx.npy"]


def _bench(out_dir, steps=30, warmup=5):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                          "--warmup", str(warmup), "--dump-outputs", str(out_dir)],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout  # ONE result line
    return json.loads(lines[0])


def test_plain_run_is_lean_and_dumps_the_same_outputs_every_time(tmp_path):
    a, b = _bench(tmp_path / "a"), _bench(tmp_path / "b")
    for d in (a, b):
        assert d["steps"] == 30 and d["warmup"] == 5 and d["ms_per_step"] > 0 and d["value"] > 0
        assert d["unit"] == "trajectory-steps/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
        for extra in ("roofline", "phase_latency_us", "host_in_loop_latency_us", "batched_agents", "cpu_baseline"):
            assert extra not in d  # --full only
    assert sorted(os.listdir(tmp_path / "a")) == NAMES
    shapes = {"costs.npy": (4096,), "softmin.npy": (3,), "state.npy": (3,), "u_prev.npy": (50, 2), "waypoint_idx.npy": (1,)}
    for n in NAMES:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype == np.float64 and x.shape == shapes[n], (n, x.dtype, x.shape)
        assert np.all(np.isfinite(x)), n
        np.testing.assert_array_equal(x, y, err_msg=n)
    assert float(np.load(tmp_path / "a" / "waypoint_idx.npy")[0]) == a["config"]["waypoint_idx_at_end_of_timing"]
