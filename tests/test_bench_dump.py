"""bench.py --dump-outputs: the output of the last timed step, written as .npy so that two builds can be compared output for
output, and --steps as the number of timed steps in the result line."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_selection_keeps_everything_that_fits():
    import bench
    patch = 96 * 96 * 4
    assert bench.dump_selection(1024, patch, bench.DUMP_BUDGET_BYTES) is None       # the headline's 1024 patches: 37.7 MB
    assert bench.dump_selection(0, 0, bench.DUMP_BUDGET_BYTES) is None


@pytest.mark.parametrize("n", [4096, 100000])
def test_dump_selection_samples_a_fixed_subset_within_the_budget(n):
    import bench
    patch = 96 * 96 * 4
    sel = bench.dump_selection(n, patch, bench.DUMP_BUDGET_BYTES)
    assert sel is not None and len(sel) > 0
    assert np.array_equal(sel, np.unique(sel)) and sel[0] >= 0 and sel[-1] < n
    assert len(sel) * (patch + 8) + 512 <= bench.DUMP_BUDGET_BYTES
    assert np.array_equal(sel, bench.dump_selection(n, patch, bench.DUMP_BUDGET_BYTES))
    half = bench.dump_selection(n, patch, bench.DUMP_BUDGET_BYTES // 2)        # two ranks share the budget
    assert len(half) * (patch + 8) + 512 <= bench.DUMP_BUDGET_BYTES // 2


def test_zero_steps_is_refused():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], cwd=ROOT, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True, timeout=120)
    assert out.returncode == 2 and "--steps" in out.stderr


def _bench(dump, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--patches", "6", "--steps", str(steps), "--warmup", "1",
           "--no-cpu-baseline", "--no-host-path", "--no-layer-by-layer", "--check-output", "--dump-outputs", str(dump)]
    out = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_dump_is_the_timed_output_and_repeats(tmp_path):
    a = _bench(tmp_path / "a", 1)
    b = _bench(tmp_path / "b", 3)
    for r, steps in ((a, 1), (b, 3)):
        assert r["steps"] == steps and r["ms_per_step"] > 0
        assert r["dump_outputs"]["files"] == ["y.npy"] and not r["dump_outputs"]["sampled"]
    ya = np.load(tmp_path / "a" / "y.npy")
    yb = np.load(tmp_path / "b" / "y.npy")
    assert ya.dtype == np.float32 and ya.shape == (6, 96, 96, 1) and np.isfinite(ya).all()
    assert os.listdir(tmp_path / "a") == ["y.npy"]
    # the dumped array is the y that --check-output hashed after the timed steps
    digest = hashlib.sha256("".join(hashlib.sha256(ya[i].tobytes()).hexdigest() for i in range(len(ya))).encode()).hexdigest()
    assert digest == a["output_sha256"]
    # same arguments up to --steps: same inputs, same outputs
    assert np.array_equal(ya, yb) and a["output_sha256"] == b["output_sha256"]
