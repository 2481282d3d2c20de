"""Host-side checks of the training driver: helper/loader.DynamicDataSets, SuperResolution's training bookkeeping and
train.py's refusal of --build_batch; no GPU needed."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_host import _flags


def _dataset(scale=2, size=24):
    from helper import loader
    d = loader.DynamicDataSets(scale, size)
    d.set_data_dir(os.path.join(GOLDEN, "set14"))
    return d


def test_dynamic_datasets_shapes_ranges_and_reproducibility():
    d = _dataset()
    assert d.count == len(os.listdir(os.path.join(GOLDEN, "set14")))
    batches = []
    for _ in range(2):
        random.seed(123)
        d.init_batch_index()
        batches.append([d.load_batch_image(255.0) for _ in range(20)])         # > count: the index is reshuffled once
    for (x, x2, y), (xb, x2b, yb) in zip(*batches):
        assert x.shape == (24, 24, 1) and x2.shape == (48, 48, 1) and y.shape == (48, 48, 1)
        # the true patch is Y of YCbCr (16 .. 235) of a colour image, the pixels of a grey one; the bicubic resizes may ring
        assert y.min() >= 0 and y.max() <= 255
        for a in (x, x2):
            assert np.all(np.isfinite(a)) and a.min() >= -16.0 and a.max() <= 271.0
        assert np.array_equal(x, xb) and np.array_equal(x2, x2b) and np.array_equal(y, yb)
    random.seed(124)
    d.init_batch_index()
    other = [d.load_batch_image(255.0) for _ in range(20)]
    assert any(not np.array_equal(a[2], b[2]) for a, b in zip(batches[0], other))


def test_dynamic_datasets_max_value_scales_all_three():
    d = _dataset(scale=3, size=16)
    random.seed(5)
    d.init_batch_index()
    x, x2, y = d.load_batch_image(1.0)
    assert x.shape == (16, 16, 1) and x2.shape == (48, 48, 1) and y.shape == (48, 48, 1)
    assert max(x.max(), x2.max(), y.max()) <= 1.0 + 1e-6


def test_model_training_bookkeeping(tmp_path):
    from dcscn_amd.model import SuperResolution
    m = SuperResolution(_flags(checkpoint_dir=str(tmp_path / "models"), initial_lr=0.002, lr_decay=0.5, lr_decay_epoch=3, end_lr=2e-4, training_images=50, batch_num=20))
    assert m.training_images == 60                                     # ceil(50 / 20) * 20, DCSCN.py:72
    assert m.total_epochs == 12                                        # 0.002 -> 0.0001 in 4 decays of 3 epochs
    m.init_train_step()
    assert m.lr == 0.002 and m.step == 0
    assert [m.update_epoch_and_lr() for _ in range(4)] == [False, False, True, False]
    assert m.lr == 0.001
    m.step = 7
    m.dropout_seed = 3
    assert m.dropout_key() == (3 << 32) + 7
    m.build_optimizer()
    assert m._train_flags["optimizer"] == "adam" and m._train_flags["dropout_rate"] == 0.8
    with pytest.raises(SystemExit):
        m.load_datasets("data", "batch", 48)
    m.log_to_tensorboard("x.png", 30.0)                                # documented no-op


def test_train_py_refuses_build_batch(tmp_path):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--build_batch=true", "--data_dir=" + GOLDEN, "--dataset=set14",
                        "--checkpoint_dir=" + str(tmp_path / "models")], cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert p.returncode != 0
    assert "--build_batch true (BatchDataSets) is not supported" in p.stdout
