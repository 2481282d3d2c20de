"""PSNR / SSIM on the device, host side (no GPU): the binding's struct, the --device_metrics switch, and what csrc/metrics.hip must
compute -- a plain numpy restatement of the kernel's arithmetic and order of sums against imaging.compute_psnr_and_ssim (numpy +
scipy.ndimage, the restatement of helper/utilty.py:509-536)."""
import ctypes
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_host import _flags

WIN, PAD = 11, 5


def gaussian_window():
    """scipy.ndimage's window for sigma 1.5 truncated at 3.5 sigma: exp(-0.5 / sigma^2 * x^2) / sum, 11 taps, float64."""
    x = np.arange(-PAD, PAD + 1)
    phi = np.exp(-0.5 / (1.5 * 1.5) * x ** 2)
    return phi / phi.sum()


def kernel_restatement(image1, image2, border_size=0):
    """(psnr, ssim, sq_err_sum, n_pixels) the way the kernels compute them: integer trim, int64 squared error, the five 11-tap sums
    taken tap by tap in order over the rows whose window lies inside the image, S summed row by row, the mean over rows and then
    over columns one after the other.  No scipy."""
    a = np.clip(np.rint(np.asarray(image1, np.float64)), 0, 255).astype(np.int64)
    b = np.clip(np.rint(np.asarray(image2, np.float64)), 0, 255).astype(np.int64)
    a, b = a.reshape(a.shape[0], a.shape[1]), b.reshape(b.shape[0], b.shape[1])
    if border_size > 0:
        a = a[border_size:-border_size, border_size:-border_size]
        b = b[border_size:-border_size, border_size:-border_size]
    h, w = a.shape
    if h < WIN:
        raise ValueError("win_size exceeds image extent")
    sq = int(((a - b) ** 2).sum(dtype=np.int64))
    psnr = float("inf") if sq == 0 else 10.0 * math.log10((255.0 * 255.0) / (float(sq) / float(h * w)))
    wt = gaussian_window()
    fa, fb = a.astype(np.float64), b.astype(np.float64)
    rows = h - 2 * PAD

    def filt(x):
        acc = np.zeros((rows, w))
        for k in range(WIN):
            acc = acc + wt[k] * x[k:k + rows]
        return acc

    ux, uy, uxx, uyy, uxy = filt(fa), filt(fb), filt(fa * fa), filt(fb * fb), filt(fa * fb)
    cov_norm = WIN / (WIN - 1.0)
    vx = cov_norm * (uxx - ux * ux)
    vy = cov_norm * (uyy - uy * uy)
    vxy = cov_norm * (uxy - ux * uy)
    c1, c2 = (0.01 * 255.0) * (0.01 * 255.0), (0.03 * 255.0) * (0.03 * 255.0)
    s = ((2.0 * ux * uy + c1) * (2.0 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    column = np.zeros(w)
    for r in range(rows):
        column = column + s[r]
    column = column / float(rows)
    total = 0.0
    for c in range(w):
        total += column[c]
    return psnr, total / float(w), sq, h * w


def golden_cases():
    """(label, true Y or grey image, host bicubic of its LR image, border) for every Set5 and Set14 golden at x2, x3, x4, with
    border = scale and border = 0: 19 files x 3 x 2 = 114 image pairs."""
    from dcscn_amd import imaging as util
    from dcscn_amd.model import build_input_image
    out = []
    for name in ("set5", "set14"):
        d = os.path.join(GOLDEN, name)
        for f in sorted(os.listdir(d)):
            image = util.load_image(os.path.join(d, f), print_console=False)
            for scale in (2, 3, 4):
                true_image = util.set_image_alignment(image, scale)
                true_y = util.convert_rgb_to_y(true_image) if true_image.shape[2] == 3 else true_image
                lr = build_input_image(true_image, channels=1, scale=scale, alignment=scale, convert_ycbcr=True)
                bicubic = util.resize_image_by_pil(lr, scale, resampling_method="bicubic")
                for border in (scale, 0):
                    out.append(("%s/%s x%d border %d" % (name, f, scale, border), true_y, bicubic, border))
    return out


def test_metrics_struct_is_32_bytes():
    from dcscn_amd import engine
    assert ctypes.sizeof(engine.Metrics) == 32
    assert [n for n, _ in engine.Metrics._fields_] == ["psnr", "ssim", "sq_err_sum", "n_pixels"]
    assert engine.ABI_VERSION == 4
    assert "dcscn_psnr_ssim" in engine.EXPORTED_SYMBOLS and "dcscn_evaluate_rgb_metrics" in engine.EXPORTED_SYMBOLS


def test_device_metrics_flag_defaults_to_off(tmp_path):
    from helper import args
    from dcscn_amd.model import SuperResolution
    assert "device_metrics" in args.FLAGS and args.FLAGS._flags["device_metrics"].default is False
    assert args.FLAGS._flags["device_metrics"].kind == "boolean"
    m = SuperResolution(_flags(checkpoint_dir=str(tmp_path / "models")))
    assert m.device_metrics is False
    m = SuperResolution(_flags(checkpoint_dir=str(tmp_path / "models"), device_metrics=True))
    assert m.device_metrics is True


def test_kernel_arithmetic_matches_the_host_metrics_on_every_golden():
    """Pins what the kernel must compute: PSNR bit for bit, SSIM within 1e-12 of the scipy-based host function."""
    from dcscn_amd import imaging as util
    cases = golden_cases()
    assert len(cases) == 114
    worst = 0.0
    for label, a, b, border in cases:
        want_psnr, want_ssim = util.compute_psnr_and_ssim(a, b, border_size=border)
        psnr, ssim, _, _ = kernel_restatement(a, b, border)
        assert psnr == want_psnr, label
        worst = max(worst, abs(ssim - want_ssim))
        assert abs(ssim - want_ssim) <= 1e-12, (label, ssim, want_ssim)
    print("worst |SSIM restatement - host| over %d cases: %.3g" % (len(cases), worst))


def test_identical_images_give_inf_and_one():
    from dcscn_amd import imaging as util
    label, a, _, border = golden_cases()[0]
    assert util.compute_psnr_and_ssim(a, a.copy(), border_size=border) == (float("inf"), 1.0)
    assert kernel_restatement(a, a.copy(), border)[:2] == (float("inf"), 1.0)


def test_restatement_refuses_what_the_host_refuses():
    from dcscn_amd import imaging as util
    a = np.full((12, 9), 7.0)
    with pytest.raises(ValueError, match="win_size"):
        util.compute_psnr_and_ssim(a, a, border_size=1)
    with pytest.raises(ValueError, match="win_size"):
        kernel_restatement(a, a, 1)
