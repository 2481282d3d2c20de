"""PSNR / SSIM on the device (csrc/metrics.hip; dcscn_psnr_ssim, dcscn_evaluate_rgb_metrics, SuperResolution.device_metrics)
against imaging.compute_psnr_and_ssim, the host restatement of helper/utilty.py:509-536.

The PSNR is formed from two exact integers and must have the host's bits.  The SSIM bar is 1e-10 absolute: the device sums the
11 taps in order where scipy pairs the symmetric ones, which moved the SSIM by 1.5e-14 on the CPU (test_metrics_host.py).  The
roundings, at worst a few ulps of 255^2 in uxx - ux^2, enter factors bounded below by C1 = 6.5 and C2 = 58.5, about 1e-12 per
pixel at the very worst.  1e-10 is four orders above the CPU figure and four below the sixth decimal evaluate.py prints.
Measured on an MI355X over the 143 image pairs of the first test: PSNR and the integer sums equal everywhere, worst
|SSIM device - host| 6.62e-14 (the 114 goldens: 1.43e-14)."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_golden_hip import _goldens, _model
from test_metrics_host import golden_cases, kernel_restatement

pytestmark = pytest.mark.gpu

SSIM_TOL = 1e-10


def _host(a, b, border):
    from dcscn_amd import imaging as util
    return util.compute_psnr_and_ssim(a, b, border_size=border)


def _sq_err(a, b, border):
    """The int64 squared error of the trimmed, shaved images in numpy."""
    a = np.clip(np.rint(np.asarray(a, np.float64)), 0, 255).astype(np.int64).reshape(a.shape[0], a.shape[1])
    b = np.clip(np.rint(np.asarray(b, np.float64)), 0, 255).astype(np.int64).reshape(b.shape[0], b.shape[1])
    if border > 0:
        a, b = a[border:-border, border:-border], b[border:-border, border:-border]
    return int(((a - b) ** 2).sum(dtype=np.int64)), a.size


def _check(eng, label, a, b, border):
    """One image pair: PSNR ==, squared error and pixel count == numpy's integers, SSIM within the bar; returns |SSIM difference|."""
    want_psnr, want_ssim = _host(a, b, border)
    got = eng.psnr_ssim(a, b, border, full=True)
    sq, n = _sq_err(a, b, border)
    print("%-40s psnr %r / %r  ssim %r / %r  diff %.3g" % (label, got.psnr, want_psnr, got.ssim, want_ssim, abs(got.ssim - want_ssim)))
    assert (got.sq_err_sum, got.n_pixels) == (sq, n), label
    assert got.psnr == want_psnr, label
    assert abs(got.ssim - want_ssim) <= SSIM_TOL, (label, got.ssim, want_ssim)
    assert eng.psnr_ssim(a, b, border) == (got.psnr, got.ssim)
    return abs(got.ssim - want_ssim)


def _random_cases():
    rng = np.random.default_rng(11)
    out = []
    for h, w in ((37, 53), (300, 70)):
        a = rng.uniform(-20, 280, (h, w))
        b = a + rng.normal(0, 6, (h, w))
        for border in (0, 2, 3):
            out.append(("random %dx%d border %d" % (h, w, border), a, b, border))
        out.append(("random %dx%d [H, W, 1]" % (h, w), a[:, :, None], b[:, :, None], 2))
        out.append(("random %dx%d mixed ranks" % (h, w), a, b[:, :, None], 0))
        out.append(("random %dx%d float32" % (h, w), a.astype(np.float32), b.astype(np.float32), 2))
        out.append(("random %dx%d float32 vs float64" % (h, w), a.astype(np.float32), b, 0))
        out.append(("random %dx%d identical" % (h, w), a, a.copy(), 2))
    for (h, w), border in (((15, 5), 2), ((11, 1), 0), ((12, 7), 0), ((16, 11), 2)):       # shaved to 11 x 1 and 12 x 7
        a = rng.uniform(-20, 280, (h, w))
        out.append(("small %dx%d border %d" % (h, w, border), a, rng.uniform(-20, 280, (h, w)), border))
    ties = np.array([0.5, 1.5, 254.5, 255.5, -0.5, 2.5, 253.5, 127.5, 128.5])
    a = np.tile(ties, (14, 3))
    out.append(("ties vs their even neighbours", a, np.tile(np.array([0.0, 2, 254, 255, 0, 2, 254, 128, 128]), (14, 3)), 0))
    out.append(("ties vs noise", a, rng.uniform(0, 255, a.shape), 1))
    out.append(("ties float32", a.astype(np.float32), rng.uniform(0, 255, a.shape).astype(np.float32), 0))
    for va, vb in ((0.0, 0.0), (255.0, 0.0), (17.0, 17.4), (100.0, 131.0), (300.0, -7.0)):
        out.append(("constant %g vs %g" % (va, vb), np.full((23, 9), va), np.full((23, 9), vb), 1))
    out.append(("uint8 grey", rng.integers(0, 256, (40, 33, 1), dtype=np.uint8), rng.uniform(0, 255, (40, 33, 1)), 2))
    return out


def test_ties_round_half_to_even(tmp_path):
    g, m = _model(tmp_path, "L7_x2")
    eng = m._ready_engine()
    a = np.tile(np.array([0.5, 1.5, 254.5, 255.5, -0.5]), (11, 1))
    b = np.tile(np.array([0.0, 2.0, 254.0, 255.0, 0.0]), (11, 1))
    got = eng.psnr_ssim(a, b, 0, full=True)
    assert got.sq_err_sum == 0 and got.n_pixels == 55 and got.psnr == float("inf") and got.ssim == 1.0
    m.close()


def test_psnr_ssim_matches_the_host_on_goldens_and_random_images(tmp_path):
    g, m = _model(tmp_path, "L7_x2")
    eng = m._ready_engine()
    cases = golden_cases()
    assert len(cases) == 114
    cases += _random_cases()
    worst = max(_check(eng, *case) for case in cases)
    print("worst |SSIM device - host| over %d cases: %.3g" % (len(cases), worst))
    # the device against the numpy restatement of its own order of sums: the same arithmetic up to the final mean's grouping
    worst_r = 0.0
    for label, a, b, border in cases[::6]:
        got = eng.psnr_ssim(a, b, border, full=True)
        r = kernel_restatement(a, b, border)
        assert (got.psnr, got.sq_err_sum, got.n_pixels) == (r[0], r[2], r[3])
        worst_r = max(worst_r, abs(got.ssim - r[1]))
    print("worst |SSIM device - numpy restatement|: %.3g" % worst_r)
    assert worst_r <= SSIM_TOL
    m.close()


def test_psnr_ssim_shape_mismatch_returns_none_and_runs_before_finalize():
    from dcscn_amd import engine
    g = _goldens()
    rng = np.random.default_rng(2)
    a, b = rng.uniform(0, 255, (20, 31)), rng.uniform(0, 255, (20, 31))
    with engine.Engine(dict(g["models"]["L7_x2"]["flags"], scale=2)) as eng:       # created, never finalized
        assert eng.psnr_ssim(a, b[:, :-1]) is None
        _check(eng, "before finalize", a, b, 2)
        with pytest.raises(engine.EngineError) as e:
            eng.evaluate_rgb_metrics(np.zeros((32, 32, 3), np.uint8))
        assert e.value.status == 6


@pytest.mark.parametrize("key,ens", [("L7_x2", 1), ("L7_x3", 1), ("L7_x4", 1), ("L7_x2", 8), ("L7_x4", 3)])
def test_evaluate_rgb_metrics_equals_evaluate_rgb_plus_host_metrics(tmp_path, key, ens):
    from dcscn_amd import imaging as util
    g, m = _model(tmp_path, key, self_ensemble=ens)
    eng = m._ready_engine()
    border = m.scale
    assert m.psnr_calc_border_size == border
    done = 0
    for f in g["files"]:
        path = os.path.join(GOLDEN, "set5", f)
        true_image = util.set_image_alignment(util.load_image(path, print_console=False), m.scale)
        if not m._device_colour_path(true_image):
            continue
        true_y, y = eng.evaluate_rgb(true_image, ens)
        want = _host(true_y, y, border)
        model, bicubic, out = eng.evaluate_rgb_metrics(true_image, ens, border, want_bicubic=True, want_output=True, full=True)
        print(key, ens, f, model.psnr, want[0], model.ssim, want[1], abs(model.ssim - want[1]))
        assert model.psnr == want[0] and abs(model.ssim - want[1]) <= SSIM_TOL
        assert (model.sq_err_sum, model.n_pixels) == _sq_err(true_y, y, border)
        want_b = m.evaluate_bicubic(path)                          # host: Pillow resizes + numpy / scipy metrics
        assert bicubic.psnr == want_b[0] and abs(bicubic.ssim - want_b[1]) <= SSIM_TOL
        assert out.dtype == y.dtype and np.array_equal(out, y)
        pair, none_b, none_y = eng.evaluate_rgb_metrics(true_image, ens, border)
        assert pair == (model.psnr, model.ssim) and none_b is None and none_y is None
        done += 1
    assert done >= 3
    m.close()


def _dataset_files():
    out = []
    for name in ("set5", "set14"):
        d = os.path.join(GOLDEN, name)
        out += [os.path.join(d, f) for f in sorted(os.listdir(d))]
    return out


def _same(got, want, what):
    assert got[0] == want[0], (what, got, want)
    assert abs(got[1] - want[1]) <= SSIM_TOL, (what, got, want)


@pytest.mark.parametrize("key,ens", [("L7_x2", 1), ("L7_x4", 3)])
def test_model_with_device_metrics_reports_the_host_values(tmp_path, key, ens):
    from dcscn_amd import imaging as util
    files = _dataset_files()
    assert any(util.load_image(f, print_console=False).shape[2] == 1 for f in files)        # grey img_003 of Set14 is in
    g, host = _model(tmp_path, key, self_ensemble=ens)
    g, dev = _model(tmp_path, key, self_ensemble=ens, device_metrics=True)
    assert host.device_metrics is False and dev.device_metrics is True
    for f in files:
        _same(dev.do_for_evaluate(f), host.do_for_evaluate(f), ("do_for_evaluate", f))
        _same(dev.evaluate_bicubic(f), host.evaluate_bicubic(f), ("evaluate_bicubic", f))
    for got, want, f in zip(dev.do_for_evaluate_many(files), host.do_for_evaluate_many(files), files):
        _same(got, want, ("do_for_evaluate_many", f))
    _same(dev.evaluate(files), host.evaluate(files), "evaluate")
    for f in files:
        _same(dev.do_for_evaluate_with_output(f, str(tmp_path / "dev")), host.do_for_evaluate_with_output(f, str(tmp_path / "host")),
              ("do_for_evaluate_with_output", f))
    host.close()
    dev.close()


def test_model_with_device_metrics_raises_the_host_error_for_a_small_image(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(3)
    g, dev = _model(tmp_path, "L7_x2", device_metrics=True)
    g, host = _model(tmp_path, "L7_x2")
    for name, shape in (("rgb.png", (14, 20, 3)), ("grey.png", (14, 20))):                  # 10 rows after shaving 2
        path = str(tmp_path / name)
        Image.fromarray(rng.integers(0, 256, shape, dtype=np.uint8)).save(path)
        for m in (host, dev):
            with pytest.raises(ValueError, match="win_size exceeds image extent"):
                m.do_for_evaluate(path)
    host.close()
    dev.close()


def test_two_runs_give_the_same_bits(tmp_path):
    from dcscn_amd import imaging as util
    g, m = _model(tmp_path, "L7_x2", self_ensemble=8)
    eng = m._ready_engine()
    label, a, b, border = golden_cases()[40]
    first = eng.psnr_ssim(a, b, border, full=True)
    true_image = util.set_image_alignment(util.load_image(os.path.join(GOLDEN, "set5", g["files"][0]), print_console=False), 2)
    first_rgb = eng.evaluate_rgb_metrics(true_image, 8, 2, want_bicubic=True)
    for _ in range(3):
        again = eng.psnr_ssim(a, b, border, full=True)
        assert bytes(again) == bytes(first)
        assert eng.evaluate_rgb_metrics(true_image, 8, 2, want_bicubic=True) == first_rgb
    m.close()


def test_tiled_forward_gives_the_same_metrics(tmp_path):
    """A workspace budget smaller than the image makes the forward pass cut it into windows; the metrics are taken from the
    stitched output like from a whole one, and agree with evaluate_rgb + host metrics in the same state."""
    from dcscn_amd import imaging as util
    g, m = _model(tmp_path, "L7_x2")
    eng = m._ready_engine()
    true_image = util.set_image_alignment(util.load_image(os.path.join(GOLDEN, "set5", g["files"][1]), print_console=False), 2)
    whole = eng.evaluate_rgb_metrics(true_image, 1, 2, want_output=True, full=True)
    before = eng.workspace_bytes()
    lr_pixels = (true_image.shape[0] // 2) * (true_image.shape[1] // 2)
    assert lr_pixels > 4 * 64 * 64
    eng.set_option("workspace_budget_bytes", (before // lr_pixels + 1) * 64 * 64)           # windows of about 64 x 64 LR pixels
    true_y, y = eng.evaluate_rgb(true_image, 1)
    tiled = eng.evaluate_rgb_metrics(true_image, 1, 2, want_output=True, full=True)
    want = _host(true_y, y, 2)
    assert np.array_equal(tiled[2], y)
    assert tiled[0].psnr == want[0] and abs(tiled[0].ssim - want[1]) <= SSIM_TOL
    # against the untiled pass: the outputs agree to float32 rounding, so at most a handful of pixels round differently
    assert abs(tiled[0].psnr - whole[0].psnr) <= 1e-3 and abs(tiled[0].ssim - whole[0].ssim) <= 1e-5
    m.close()


def test_metrics_after_a_training_step(tmp_path):
    """dcscn_evaluate_rgb_metrics synchronises the inference plan with the trained variables like dcscn_evaluate_rgb does."""
    from conftest import synthetic_batch
    from dcscn_amd import imaging as util
    g, m = _model(tmp_path, "L7_x2")
    eng = m._ready_engine()
    true_image = util.set_image_alignment(util.load_image(os.path.join(GOLDEN, "set5", g["files"][0]), print_console=False), 2)
    before = eng.evaluate_rgb_metrics(true_image, 1, 2, full=True)[0]
    eng.train_begin(dict(optimizer="adam", beta1=0.9, beta2=0.999, epsilon=1e-8, momentum=0.9, l2_decay=1e-4, clipping_norm=5.0,
                         dropout_rate=1.0, use_l1_loss=False))
    x, x2 = synthetic_batch(4, 24, 24, 2, seed=5)
    y = (x2 + np.random.default_rng(6).normal(0, 8, x2.shape)).astype(np.float32)
    eng.train_step(x, x2, y, 2e-3)
    after = eng.evaluate_rgb_metrics(true_image, 1, 2, full=True)[0]
    true_y, out = eng.evaluate_rgb(true_image, 1)
    want = _host(true_y, out, 2)
    assert after.psnr == want[0] and abs(after.ssim - want[1]) <= SSIM_TOL
    assert after.sq_err_sum != before.sq_err_sum                 # the step changed the network, and the metrics saw it
    m.close()


def test_refusals(tmp_path):
    from dcscn_amd import engine
    g, m = _model(tmp_path, "L7_x2")
    eng = m._ready_engine()
    a = np.zeros((14, 20))
    with pytest.raises(engine.EngineError) as e:
        eng.psnr_ssim(a, a, 2)                                    # 10 rows after shaving
    assert e.value.status == 1 and "win_size" in e.value.message
    assert eng.psnr_ssim(np.zeros((15, 20)), np.zeros((15, 20)), 2) == (float("inf"), 1.0)
    with pytest.raises(engine.EngineError) as e:
        eng.psnr_ssim(np.zeros((30, 4)), np.zeros((30, 4)), 2)    # no column left
    assert e.value.status == 1 and "win_size" in e.value.message
    with pytest.raises(engine.EngineError) as e:
        eng.psnr_ssim(np.zeros((30, 30)), np.zeros((30, 30)), -1)
    assert e.value.status == 1 and "win_size" in e.value.message
    rgb = np.zeros((14, 20, 3), np.uint8)
    with pytest.raises(engine.EngineError) as e:
        eng.evaluate_rgb_metrics(rgb, 1, 2)
    assert e.value.status == 1 and "win_size" in e.value.message
    with pytest.raises(engine.EngineError) as e:
        eng.evaluate_rgb_metrics(np.zeros((32, 32, 3), np.uint8), 1, -2)
    assert e.value.status == 1
    lib, h = eng._lib, eng._h
    out = engine.Metrics()
    buf = np.zeros((16, 16))
    dp = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert lib.dcscn_psnr_ssim(h, None, dp, 16, 16, 0, ctypes.byref(out)) == 1
    assert lib.dcscn_psnr_ssim(h, dp, None, 16, 16, 0, ctypes.byref(out)) == 1
    assert lib.dcscn_psnr_ssim(h, dp, dp, 16, 16, 0, None) == 1
    assert lib.dcscn_psnr_ssim(None, dp, dp, 16, 16, 0, ctypes.byref(out)) == 1
    img = np.zeros((32, 32, 3), np.uint8)
    u8 = img.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    assert lib.dcscn_evaluate_rgb_metrics(h, None, 32, 32, 1, 2, ctypes.byref(out), None, None) == 1
    assert lib.dcscn_evaluate_rgb_metrics(h, u8, 32, 32, 1, 2, None, None, None) == 1
    assert lib.dcscn_evaluate_rgb_metrics(h, u8, 32, 32, 1, 2, ctypes.byref(out), None, None) == 0
    m.close()
