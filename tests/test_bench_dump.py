"""bench.py --dump-outputs: the output of the last timed step, written as .npy so that two builds can be compared output for
output, and --steps as the number of timed steps in the result line.  A plain run prints the headline alone; --full adds every
other leg."""
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


# what only --full adds to the line (strong_scaling: N > 1 only)
FULL_LEGS = ("north_star", "cpu_baseline", "host_path", "graph_replay", "float32_tensors", "f32_path", "layer_by_layer",
             "other_configs", "parity")


def _line(args):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args
    out = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone():
    r = _line(["--patches", "6", "--steps", "2", "--warmup", "1"])
    assert r["steps"] == 2 and r["warmup"] == 1 and r["ms_per_step"] > 0 and r["higher_is_better"] is True
    assert abs(r["value"] - 6 * 48 * 48 / (r["ms_per_step"] * 1e-3) / 1e6) / r["value"] < 1e-3
    assert r["roofline"]["kernel_ms_per_step"] > 0 and r["dtype"]
    assert not [k for k in FULL_LEGS if k in r]


@pytest.mark.gpu
def test_full_run_adds_every_leg():
    """--full on a small batch (--cpu-sample 2, --other-steps 1): every leg is there and none failed."""
    r = _line(["--patches", "6", "--steps", "1", "--warmup", "1", "--full", "--cpu-sample", "2", "--other-steps", "1"])
    assert r["steps"] == 1 and r["ms_per_step"] > 0
    # (north_star: the committed counters are replayed for the 1024-patch workload only)
    for k in FULL_LEGS[1:]:
        assert k in r and "error" not in r[k], (k, r.get(k))
    for key in ("C2", "C5"):
        assert "error" not in r["other_configs"][key] and r["other_configs"][key]["steps"] == 1
    assert r["graph_replay"]["bit_identical_to_plain_launches"] and r["float32_tensors"]["bit_identical_to_headline"]
    assert r["parity"]["set5_psnr_delta_db"] <= r["parity"]["bars"]["set5_psnr_delta_db"]
    assert r["parity"]["max_abs"] <= r["parity"]["bars"]["max_abs"]


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
