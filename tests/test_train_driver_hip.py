"""The training driver on the GPU: SuperResolution.train_batch / save_model / load_model with the optimizer slots, and
train.py end to end with evaluate.py loading what it wrote."""
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import CONFIGS, GOLDEN, ROOT
from test_host import _flags

pytestmark = pytest.mark.gpu

L7 = dict(CONFIGS["L7_F32to8_x2"], self_ensemble=1)


def _batches(count, n=4, size=24):
    from helper import loader
    d = loader.DynamicDataSets(2, size)
    d.set_data_dir(os.path.join(GOLDEN, "set14"))
    random.seed(0)
    d.init_batch_index()
    return [[d.load_batch_image(255.0) for _ in range(n)] for _ in range(count)]


def _model(ck, weights=None):
    from dcscn_amd.model import SuperResolution
    m = SuperResolution(_flags(checkpoint_dir=ck, batch_num=4, **L7))
    m.build_graph()
    m.build_optimizer()
    if weights is not None:
        m.load_weights(weights)
    m.init_train_step()
    return m


def _steps(m, batches, start, count):
    for i in range(start, start + count):
        m.batch_input, m.batch_input_bicubic, m.batch_true = (list(t) for t in zip(*batches[i]))
        m.train_batch()


def test_resume_through_save_model_and_load_model(oracle, tmp_path):
    from dcscn_amd import ckpt
    cfg = oracle.make_config(**CONFIGS["L7_F32to8_x2"])
    weights = oracle.synthetic_weights(cfg, seed=0)
    batches = _batches(20)
    a = _model(str(tmp_path / "a"), weights)
    _steps(a, batches, 0, 20)
    a.save_model(name="straight")
    a.close()
    b = _model(str(tmp_path / "b"), weights)
    _steps(b, batches, 0, 10)
    b.save_model(name="half")
    b.close()
    c = _model(str(tmp_path / "b"))
    c.load_model(name="half")
    c.step = 10                                             # the resumed run is given its step: same dropout masks
    _steps(c, batches, 10, 10)
    c.save_model(name="resumed")
    c.close()
    half = ckpt.load_checkpoint(str(tmp_path / "b" / "half.ckpt"), include_optimizer_slots=True)
    for k, v in weights.items():
        assert half[k + "/Adam"].shape == v.shape and half[k + "/Adam_1"].shape == v.shape
    assert half["beta1_power"].shape == () and float(half["beta1_power"]) == float(np.float32(0.9) ** 11)
    want = ckpt.load_checkpoint(str(tmp_path / "a" / "straight.ckpt"), include_optimizer_slots=True)
    got = ckpt.load_checkpoint(str(tmp_path / "b" / "resumed.ckpt"), include_optimizer_slots=True)
    assert set(want) == set(got) and len(want) == 3 * len(weights) + 2
    for k in want:
        assert np.array_equal(np.asarray(want[k]).view(np.uint32), np.asarray(got[k]).view(np.uint32)), k


def test_train_py_trains_saves_and_evaluate_py_loads_it(tmp_path):
    flags = ["--scale=2", "--layers=7", "--filters=32", "--min_filters=8", "--filters_decay_gamma=1.2", "--nin_filters=24",
             "--nin_filters2=8", "--reconstruct_layers=0", "--pixel_shuffler_filters=1", "--self_ensemble=1",
             "--data_dir=" + GOLDEN, "--checkpoint_dir=" + str(tmp_path / "models"), "--output_dir=" + str(tmp_path / "out"),
             "--test_dataset=set5"]
    p = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--dataset=set14", "--batch_num=8", "--batch_image_size=24",
                        "--training_images=80", "--initial_lr=0.002", "--lr_decay_epoch=1", "--end_lr=0.0015"] + flags,
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    log = p.stdout + p.stderr
    assert p.returncode == 0, log[-3000:]
    m = re.search(r"Model Average \[set5\] PSNR:([0-9.]+)", log)
    assert m, log[-3000:]
    trained = float(m.group(1))
    saved = [f for f in os.listdir(str(tmp_path / "models")) if f.endswith(".ckpt.index")]
    assert saved == ["dcscn_L7_F32to8_G1.20_NIN_A24_B8_PS_R1F32.ckpt.index"], saved
    e = subprocess.run([sys.executable, os.path.join(ROOT, "evaluate.py"), "--save_results=false"] + flags,
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    elog = e.stdout + e.stderr
    assert e.returncode == 0, elog[-3000:]
    m2 = re.search(r"Model Average \[set5\] PSNR:([0-9.]+)", elog)
    assert m2, elog[-3000:]
    assert abs(float(m2.group(1)) - trained) < 1e-3, (trained, m2.group(1))
    assert np.isfinite(trained) and trained > 0.0
