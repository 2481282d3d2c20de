"""Host-side checks of the training restatement (tests/train_ref.py) and of checkpoint slots; no GPU needed."""
import os
import tempfile

import numpy as np
import torch

from conftest import CONFIGS, synthetic_batch
import train_ref as R


def test_hash_matches_the_reference_values_of_the_header():
    # include/dcscn.h, "Dropout mask": splitmix64(0), layer_key(1, 0) and the top 24 bits of the first two elements
    assert int(R.splitmix64(0)) == 0xE220A8397B1DCDAF
    lk = R.layer_key(1, 0)
    assert int(lk) == 0xBEEB8DA1658EEC67
    assert int(R.splitmix64(lk ^ np.uint64(0)) >> np.uint64(40)) == 0x778B1A
    assert int(R.splitmix64(lk ^ np.uint64(1)) >> np.uint64(40)) == 0x3ED40B
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dcscn.h")) as f:
        header = f.read()
    for value in ("0xE220A8397B1DCDAF", "0xBEEB8DA1658EEC67", "0x778B1A", "0x3ED40B"):
        assert value in header


def test_dropout_mask_keeps_the_requested_fraction():
    m = R.dropout_mask(1234, 3, (4, 32, 32, 16), 0.8)
    assert abs(m.mean() - 0.8) < 0.01
    assert not np.array_equal(m, R.dropout_mask(1234, 4, (4, 32, 32, 16), 0.8))
    assert np.array_equal(m, R.dropout_mask(1234, 3, (4, 32, 32, 16), 0.8))


def _cases():
    return [("L7_F32to8_x2", CONFIGS["L7_F32to8_x2"]), ("L7_F32to8_x4", CONFIGS["L7_F32to8_x4"]),
            ("L2_F4to4_x2", CONFIGS["L2_F4to4_x2"]),
            ("k5_relu_r2", dict(layers=4, filters=16, min_filters=8, nin_filters=12, nin_filters2=6, cnn_size=5, activator="relu",
                                reconstruct_layers=2, reconstruct_filters=6, use_nin=False, scale=3))]


def test_restatement_forward_matches_the_float64_torch_model(oracle):
    from cpu_path_torch import TorchCpuModel
    for _, over in _cases():
        cfg = oracle.make_config(**over)
        w = oracle.synthetic_weights(cfg, seed=3)
        x, x2 = synthetic_batch(2, 12, 14, cfg["scale"], seed=4)
        leaves = {k: torch.tensor(np.asarray(v, np.float64)) for k, v in w.items()}
        y = R.forward(cfg, leaves, x, x2).permute(0, 2, 3, 1).numpy()
        ref = TorchCpuModel(cfg, w, dtype=torch.float64).forward(x, x2)
        assert np.max(np.abs(y - ref)) <= 1e-9 * max(1.0, np.max(np.abs(ref))), over


def test_restatement_gradient_matches_finite_differences(oracle):
    cfg = oracle.make_config(layers=3, filters=6, min_filters=4, nin_filters=4, nin_filters2=3, reconstruct_layers=2,
                             reconstruct_filters=3, scale=2)
    w = oracle.synthetic_weights(cfg, seed=1)
    x, x2 = synthetic_batch(1, 6, 6, 2, seed=2)
    y_true = x2 + np.random.default_rng(0).normal(0, 5, x2.shape).astype(np.float32)
    _, g = R.loss_and_grads(cfg, w, x, x2, y_true, l2_decay=1e-3)
    for name in ("CNN2/conv_W", "B2/conv_B", "A1/prelu/A1_prelu", "Up-PS/Up-PS_CNN/conv_W", "R-CNN1/conv_W"):
        w2 = {k: np.asarray(v, np.float64).copy() for k, v in w.items()}
        idx = (0,) * w2[name].ndim
        h = 1e-6
        w2[name][idx] += h
        lp = R.loss_and_grads(cfg, w2, x, x2, y_true, l2_decay=1e-3)[0]["loss"]
        w2[name][idx] -= 2 * h
        lm = R.loss_and_grads(cfg, w2, x, x2, y_true, l2_decay=1e-3)[0]["loss"]
        fd = (lp - lm) / (2 * h)
        assert abs(fd - g[name][idx]) <= 1e-5 * max(1.0, abs(fd)), (name, fd, g[name][idx])


def test_checkpoint_with_adam_slots_round_trips(oracle):
    from dcscn_amd import ckpt
    cfg = oracle.make_config(**CONFIGS["L7_F32to8_x2"])
    w = oracle.synthetic_weights(cfg, seed=0)
    tensors = dict(w)
    rng = np.random.default_rng(1)
    for k, v in w.items():
        tensors[k + "/Adam"] = rng.standard_normal(v.shape).astype(np.float32)
        tensors[k + "/Adam_1"] = rng.uniform(0, 1, v.shape).astype(np.float32)
    tensors["beta1_power"] = np.array(0.9 ** 3, np.float32)
    tensors["beta2_power"] = np.array(0.999 ** 3, np.float32)
    with tempfile.TemporaryDirectory() as d:
        prefix = os.path.join(d, "model")
        ckpt.save_checkpoint(prefix, tensors)
        back = ckpt.load_checkpoint(prefix, include_optimizer_slots=True)
        plain = ckpt.load_checkpoint(prefix)
    assert set(back) == set(tensors)
    for k, v in tensors.items():
        assert back[k].shape == v.shape and np.array_equal(back[k], v), k
    assert set(plain) == set(w)
