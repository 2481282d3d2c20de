"""Option "fast16" (include/dcscn.h), host side (no GPU): the CPU restatement tests/fast16_model.py that the device tests of
tests/test_fast16_hip.py are measured against, and the --fast16 switch.

The restatement is pinned from both sides: with no layer selected it IS the float64 oracle, and with the eligibility rule of
tools/f16x3_numerics.py on L12 x2 (weights seed 0, one 20 x 20 image from U(0, 255)) its rms error against the float64 oracle lies in
[3e-4, 1e-3] on the 0-255 scale -- the figure modelled for the option was 5.6e-4.  The conditions the device tests put on the
device output (a nonzero error, max-abs <= 8 x rms) are checked on the restatement alone first."""
import os

import numpy as np
import pytest

import fast16_model as M
from conftest import CONFIGS, GOLDEN, synthetic_batch
from test_host import _flags


@pytest.fixture(scope="module")
def l12(oracle):
    cfg = oracle.make_config(**CONFIGS["L12_F196to48_x2"])
    return cfg, oracle.synthetic_weights(cfg, seed=0)


def test_restatement_with_no_layer_selected_is_the_oracle(oracle, l12):
    cfg, weights = l12
    x, x2 = synthetic_batch(1, 9, 11, cfg["scale"], seed=3)
    real = oracle.conv2d_same
    y = M.restate(oracle, cfg, weights, x, x2, frozenset())
    assert oracle.conv2d_same is real
    ref = oracle.forward(cfg, weights, x, x2, dtype=np.float64)
    assert y.dtype == np.float64 and np.array_equal(y, ref)
    assert np.array_equal(M.restate(oracle, cfg, weights, x, x2, lambda name, w: False), ref)


def test_restatement_restores_the_oracle_when_a_layer_raises(oracle, l12):
    cfg, weights = l12
    x, x2 = synthetic_batch(1, 5, 5, cfg["scale"], seed=3)
    real = oracle.conv2d_same

    def rule(name, w):
        raise KeyError(name)
    with pytest.raises(KeyError):
        M.restate(oracle, cfg, weights, x, x2, rule)
    assert oracle.conv2d_same is real


def test_rounding_helpers():
    w = np.array([[0.75, -3.0e-5, 1.0 / 3.0]], np.float32)
    s = M.weight_scale(w)
    assert s == 2.0 ** 14 and 2.0 ** 13 <= 0.75 * s < 2.0 ** 14
    q = M.f16_weights(w)
    assert q[0, 0] == 0.75 and abs(q[0, 2] - 1.0 / 3.0) <= 2.0 ** -12 / 3.0 and q[0, 2] != np.float64(np.float32(1.0 / 3.0))
    assert M.f16_round(np.array([2049.0]))[0] == 2048.0 and M.f16_round(np.array([255.0]))[0] == 255.0
    assert M.weight_scale(np.zeros((1, 1))) == 1.0


def test_restatement_error_on_l12_x2_brackets_the_modelled_figure(oracle, l12):
    cfg, weights = l12
    x, x2 = synthetic_batch(1, 20, 20, cfg["scale"], seed=0)
    ref, mod, e = M.model_error(oracle, "host L12 x2 20x20", cfg, weights, x, x2, M.numerics_rule)
    mx = M.max_abs(mod, ref)
    print("L12 x2 1x20x20, numerics rule: rms %.3g  max-abs %.3g  max/rms %.2f" % (e, mx, mx / e))
    assert 3e-4 <= e <= 1e-3
    assert mx <= 8 * e
    names = [n for n, o in zip(M.C.conv_names(oracle, cfg), M.C.convs(oracle, cfg))
             if M.numerics_rule(n, weights[o["var"] + "/conv_W"])]
    assert "CNN1" not in names and names[-1] != M.C.conv_names(oracle, cfg)[-1] and {"CNN2", "CNN12", "A1", "B1"} <= set(names), names


@pytest.mark.parametrize("n,h,w", [(1, 19, 35), (3, 7, 9)])
def test_device_conditions_hold_for_the_restatement_alone_l12(oracle, l12, n, h, w):
    """The shapes of the device test: the restatement differs from the oracle and its max-abs error stays below 8 x its rms."""
    cfg, weights = l12
    x, x2 = synthetic_batch(n, h, w, cfg["scale"], seed=5)
    ref, mod, e = M.model_error(oracle, "host L12 x2 %dx%dx%d" % (n, h, w), cfg, weights, x, x2, M.numerics_rule)
    print("L12 x2 %dx%dx%d: rms %.3g max-abs %.3g" % (n, h, w, e, M.max_abs(mod, ref)))
    assert e > 1e-5 and M.max_abs(mod, ref) <= 8 * e


def golden_crop(oracle):
    """(cfg, trained weights, lr [1, 48, 48, 1], bicubic, HR ground truth [96, 96, 1]) of tests/golden/crop_L7_x2.npz: the crop was cut
    from the third Set5 image at LR rows 40 .. 87, columns 30 .. 77 (tests/golden/make_golden.py)."""
    import json
    from PIL import Image
    with open(os.path.join(GOLDEN, "goldens.json")) as f:
        g = json.load(f)
    cfg = oracle.make_config(**CONFIGS["L7_F32to8_x2"])
    weights = dict(np.load(os.path.join(GOLDEN, "weights_L7_x2.npz")))
    crop = np.load(os.path.join(GOLDEN, "crop_L7_x2.npz"))
    img = np.atleast_3d(np.array(Image.open(os.path.join(GOLDEN, "set5", g["files"][2]))))
    true_y = oracle.rgb_to_y(oracle.align(img, 2))
    lr = oracle.pil_bicubic(true_y, 0.5)[40:88, 30:78]
    assert np.array_equal(lr.astype(np.float32), crop["lr"])
    truth = np.ascontiguousarray(true_y[80:176, 60:156]).reshape(96, 96, 1)
    return cfg, weights, crop["lr"][None], crop["bicubic"][None], truth


def psnr_delta_bound(e_model, mse):
    """|PSNR(a) - PSNR(b)| of two outputs whose rms distance is at most 2 e_model, one of which has mean square error ``mse`` against the
    truth: rmse_a <= rmse_b + 2 e_model (triangle inequality), so the ratio of the two is at most 1 + 2 e_model / sqrt(mse)."""
    return 20.0 * np.log10(1.0 + 2.0 * e_model / np.sqrt(mse))


def test_device_conditions_hold_for_the_restatement_alone_trained_weights(oracle):
    cfg, weights, lr, bic, truth = golden_crop(oracle)
    ref, mod, e = M.model_error(oracle, "host L7 x2 crop", cfg, weights, lr, bic, M.numerics_rule)
    mse_ref = float(np.mean((ref[0] - truth) ** 2))
    mse_mod = float(np.mean((mod[0] - truth) ** 2))
    d = abs(10 * np.log10(mse_ref / mse_mod))
    print("L7 x2 crop: rms %.3g max-abs %.3g  rmse vs truth %.4g  |dPSNR| %.3g  bound %.3g" % (
        e, M.max_abs(mod, ref), np.sqrt(mse_ref), d, psnr_delta_bound(e, mse_ref)))
    assert e > 1e-6 and M.max_abs(mod, ref) <= 8 * e
    assert 0 < d <= psnr_delta_bound(e, mse_ref)


def test_fast16_flag_parses_and_defaults_to_false(tmp_path):
    from helper import args
    from dcscn_amd.model import SuperResolution
    assert "fast16" in args.FLAGS
    flag = args.FLAGS._flags["fast16"]
    assert flag.default is False and flag.kind == "boolean" and args.FLAGS.fast16 is False
    saved = (flag.value, flag.present, args.FLAGS.is_parsed())
    try:
        assert args.FLAGS(["prog", "--fast16"]) == ["prog"] and args.FLAGS.fast16 is True
        assert args.FLAGS(["prog", "--fast16=false"]) == ["prog"] and args.FLAGS.fast16 is False
        assert args.FLAGS(["prog", "--fast16", "true"]) == ["prog", "true"] and args.FLAGS.fast16 is True
        assert args.FLAGS(["prog", "--nofast16"]) == ["prog"] and args.FLAGS.fast16 is False
    finally:
        flag.value, flag.present = saved[0], saved[1]
        object.__setattr__(args.FLAGS, "_parsed", saved[2])
    m = SuperResolution(_flags(checkpoint_dir=str(tmp_path / "models")))
    assert m.fast16 is False
    m = SuperResolution(_flags(checkpoint_dir=str(tmp_path / "models"), fast16=True))
    assert m.fast16 is True
