"""bench.py without --full: one JSON line for exactly the K timed steps, nothing else measured, and --dump-outputs writes what the
last timed step returned -- the same arrays, bit for bit, from two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 64


def _run(out_dir):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", str(B),
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(kartohip_lib, tmp_path):
    runs = [(_run(tmp_path / name), tmp_path / name) for name in ("a", "b")]
    for d, _ in runs:
        assert d["metric"] == "scan-matches/sec" and d["unit"] == "scan-matches/s" and d["higher_is_better"] is True
        assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["dtype"]
        assert abs(d["value"] - B / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-5
        for k in ("value_windows", "roofline", "cpu_baseline", "solve_ms", "loop_batch_ms", "replay_scans_per_s", "details_file"):
            assert k not in d, k
    shapes = {"response": (B,), "mean": (B, 3), "covariance": (B, 3, 3), "status": (B,)}
    (_, a), (_, b) = runs
    for name, shape in shapes.items():
        x, y = np.load(a / f"{name}.npy"), np.load(b / f"{name}.npy")
        assert x.dtype == np.float64 and x.shape == shape, (name, x.dtype, x.shape)
        assert np.array_equal(x, y), name
    assert (np.load(a / "status.npy") == 0).all() and (np.load(a / "response.npy") > 0.1).all()
