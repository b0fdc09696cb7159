"""CPU: `bench.py --gpus N` without a launcher never reports a one-GPU line under an N-GPU flag -- it drives N devices from
one process through the library's multi-device path, or exits non-zero when the host has fewer than N.  GPU: what a plain
run prints and what --dump-outputs writes."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpus_2_without_a_launcher_runs_two_slots_or_exits_nonzero():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
                        "--workload", "cfg3-mini", "--no-cpu-baseline"], env=env, capture_output=True, text=True, timeout=600)
    import torch
    if torch.cuda.device_count() >= 2:
        assert p.returncode == 0, p.stderr[-2000:]
        assert '"n_gpus": 2' in p.stdout
    else:
        assert p.returncode != 0
        assert '"n_gpus"' not in p.stdout
        assert "refusing" in p.stderr


def test_world_size_that_contradicts_gpus_is_refused():
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert "assert world == args.gpus or world == 1" not in src      # round 5's silent pass
    assert "--gpus %d but WORLD_SIZE is %d" in src


def _bench(*argv):
    import json
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_plain_line_steps_and_dumped_outputs(hip, tmp_path):
    """A plain run prints the headline only, --steps sets the timed steps, and --dump-outputs writes the last step's outputs
    as float64 .npy files (64 MB at most) that do not depend on how many steps ran before them."""
    import numpy as np
    a = _bench("--gpus", "1", "--workload", "cfg3-mini", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / "a"))
    b = _bench("--gpus", "1", "--workload", "cfg3-mini", "--steps", "3", "--warmup", "0", "--dump-outputs", str(tmp_path / "b"))
    for d, steps in ((a, 2), (b, 3)):
        assert d["steps"] == steps and d["ms_per_step"] > 0 and d["value"] > 0 and d["higher_is_better"] is True
        assert d["dtype"] == "f64" and d["unit"] == "Mcells/s" and "roofline" not in d and "cpu_baseline" not in d
        assert abs(d["value"] - 1500 * 1500 / d["ms_per_step"] / 1e3) < 1e-6 * d["value"]
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and "final.npy" in names and "lambda.npy" in names
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 << 20
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype == np.float64 and np.array_equal(x, y, equal_nan=True), n
    assert np.load(tmp_path / "a" / "final.npy").size == 1500 * 1500      # a plane smaller than the sample is written whole
    assert float(np.load(tmp_path / "a" / "lambda.npy")) == a["lambda"]
