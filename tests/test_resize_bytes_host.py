"""The 8-bit bicubic tables of the library (dcscn_resample_table_bytes, host code) against Pillow itself: the numpy
restatement of Pillow's 8-bpc passes (resize_bytes_model.py), fed by the library's tables, must reproduce
Image.resize(BICUBIC) bit for bit for modes 'L' and 'RGB'; its accumulators must fit the int32 the kernels hold them in;
and the uint8 cast the device applies must be the cast save_image applies on this host."""
import numpy as np
import pytest
from PIL import Image

import resize_bytes_model as M


def _pil(img, oh, ow):
    im = Image.fromarray(img[:, :, 0]) if img.shape[2] == 1 else Image.fromarray(img, "RGB")
    return np.asarray(im.resize([ow, oh], resample=Image.BICUBIC)).reshape(oh, ow, img.shape[2])


def _table(in_size, out_size):
    from dcscn_amd import engine
    return engine.resample_table_bytes(in_size, out_size)


def test_table_is_the_float_table_at_22_bits():
    from dcscn_amd import engine
    for sizes in ((48, 96), (99, 33), (7, 7), (1, 4)):
        bounds, weights = engine.resample_table(*sizes)
        bounds8, coeffs = engine.resample_table_bytes(*sizes)
        assert coeffs.dtype == np.int32 and coeffs.shape == weights.shape and np.array_equal(bounds, bounds8)
        want = np.where(weights < 0, np.trunc(-0.5 + weights * (1 << 22)), np.trunc(0.5 + weights * (1 << 22)))
        assert np.array_equal(coeffs, want.astype(np.int32))


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("shape,out", M.SHAPES)
def test_restatement_with_the_library_tables_equals_pillow(shape, out, channels):
    rng = np.random.default_rng(shape[0] * 1000 + out[1] * 7 + channels)
    for img in (rng.integers(0, 256, shape + (channels,), dtype=np.uint8),
                rng.choice(np.array([0, 255], np.uint8), shape + (channels,)),
                M.checkerboard(shape[0], shape[1], channels)):
        got = M.resize(img, out[0], out[1], _table)
        assert np.array_equal(got, _pil(img, out[0], out[1]))


@pytest.mark.parametrize("shape,out", M.SHAPES)
def test_accumulators_stay_inside_int32(shape, out):
    lo, hi = np.iinfo(np.int32).min, np.iinfo(np.int32).max
    for img in (np.zeros(shape + (1,), np.uint8), np.full(shape + (1,), 255, np.uint8), M.checkerboard(shape[0], shape[1], 1),
                255 - M.checkerboard(shape[0], shape[1], 1)):
        accs = []
        M.resize(img, out[0], out[1], _table, accumulators=accs)
        for acc in accs:
            assert lo <= acc.min() and acc.max() <= hi


def test_save_image_cast_is_the_cast_rule_on_this_host():
    """save_image's plain astype(uint8) on float arrays = truncate to a 32-bit integer, keep the low 8 bits, for values inside
    (-2^31, 2^31).  A failure here is this host's numpy, not a kernel."""
    rng = np.random.default_rng(3)
    edge = np.array([-3.7, 257.9, 0.0, -0.0, 255.999, 256.0, -0.999, -1.0, -256.0, -256.5, 511.5, 65535.9, 65536.0, -65537.2,
                     2.0 ** 31 - 1.5, -(2.0 ** 31) + 1.5, 1e9 + 0.25, -1e9 - 0.25])
    values = np.concatenate([edge, rng.uniform(-600, 900, 4000), rng.uniform(-2.0 ** 31 + 2, 2.0 ** 31 - 2, 4000)])
    assert list(M.cast_rule(np.array([-3.7, 257.9]))) == [253, 1]
    for dtype in (np.float64, np.float32):                  # (do() returns float32 without the self-ensemble, float64 with it)
        a = values.astype(dtype)
        a = a[np.abs(a.astype(np.float64)) < 2.0 ** 31]     # rounding to float32 can reach 2^31
        with np.errstate(invalid="ignore"):
            assert np.array_equal(a.astype(np.uint8), M.cast_rule(a.astype(np.float64)))
