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


def _assert_matches_finite_differences(cfg, w, x, x2, y_true, names):
    """Element 0 of every tensor in ``names``: autograd against the central difference of the float64 loss."""
    _, g = R.loss_and_grads(cfg, w, x, x2, y_true, l2_decay=1e-3)
    for name in names:
        w2 = {k: np.asarray(v, np.float64).copy() for k, v in w.items()}
        idx = (0,) * w2[name].ndim
        h = 1e-6
        w2[name][idx] += h
        lp = R.loss_and_grads(cfg, w2, x, x2, y_true, l2_decay=1e-3)[0]["loss"]
        w2[name][idx] -= 2 * h
        lm = R.loss_and_grads(cfg, w2, x, x2, y_true, l2_decay=1e-3)[0]["loss"]
        fd = (lp - lm) / (2 * h)
        assert abs(fd - g[name][idx]) <= 1e-5 * max(1.0, abs(fd)), (name, fd, g[name][idx])


def test_restatement_gradient_matches_finite_differences(oracle):
    base = dict(layers=3, filters=6, min_filters=4, nin_filters=4, nin_filters2=3, reconstruct_layers=2, reconstruct_filters=3, scale=2)
    for act in ("prelu", "relu", "leaky_relu", "sigmoid", "tanh", "selu"):
        cfg = oracle.make_config(**dict(base, activator=act))
        w = oracle.synthetic_weights(cfg, seed=1)
        x, x2 = synthetic_batch(1, 6, 6, 2, seed=2)
        if act in ("sigmoid", "tanh", "selu"):
            x = x / np.float32(255.0)                               # off saturation, as the device tests feed these activators
        y_true = x2 + np.random.default_rng(0).normal(0, 5, x2.shape).astype(np.float32)
        names = ["CNN2/conv_W", "B2/conv_B", "Up-PS/Up-PS_CNN/conv_W", "R-CNN1/conv_W"] + (["A1/prelu/A1_prelu"] if act == "prelu" else [])
        _assert_matches_finite_differences(cfg, w, x, x2, y_true, names)


def test_restatement_gradient_on_formerly_refused_and_one_channel_nets(oracle):
    """loss_and_grads raised 'grad_weight must be contiguous' on the first two of these (a permuted weight view handed to conv2d);
    the third has one-channel layers (min_filters = 1) with NIN."""
    cases = [(dict(layers=3, filters=24, min_filters=1, filters_decay_gamma=2.0, use_nin=False, pixel_shuffler_filters=16), (1, 2, 20),
              ("CNN3/conv_W", "C/conv_B", "Up-PS/Up-PS_CNN/conv_W")),
             (dict(layers=2, filters=52, min_filters=4, filters_decay_gamma=1.5, use_nin=False, reconstruct_layers=3, reconstruct_filters=32,
                   pixel_shuffler_filters=1), (4, 17, 10), ("CNN2/conv_W", "C/prelu/C_prelu", "R-CNN2/conv_W")),
             (dict(layers=4, filters=9, min_filters=1, filters_decay_gamma=2.0, nin_filters=9, nin_filters2=3, scale=3), (2, 5, 4),
              ("CNN4/conv_W", "CNN4/prelu/CNN4_prelu", "B2/conv_W"))]
    for over, (n, h, wd), names in cases:
        cfg = oracle.make_config(**over)
        w = oracle.synthetic_weights(cfg, seed=1)
        x, x2 = synthetic_batch(n, h, wd, cfg["scale"], seed=2)
        y_true = x2 + np.random.default_rng(0).normal(0, 5, x2.shape).astype(np.float32)
        _, g = R.loss_and_grads(cfg, w, x, x2, y_true, l2_decay=1e-3)
        assert set(g) == set(w) and all(np.isfinite(v).all() and v.shape == w[k].shape for k, v in g.items())
        _assert_matches_finite_differences(cfg, w, x, x2, y_true, names)


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
