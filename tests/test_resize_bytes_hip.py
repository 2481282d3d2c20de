"""dcscn_resize_bicubic_bytes against Pillow itself: Image.resize(BICUBIC) on mode-'L' and mode-'RGB' uint8 images (what the
reference's util.resize_image_by_pil does with 8-bit images, helper/utilty.py:211-239).  The bar is BIT equality: Pillow's
int32 fixed-point tables, its horizontal pass through a uint8 intermediate, its clip."""
import numpy as np
import pytest
from PIL import Image

import resize_bytes_model as M

pytestmark = pytest.mark.gpu


def _pil(img, oh, ow):
    im = Image.fromarray(img[:, :, 0]) if img.shape[2] == 1 else Image.fromarray(img, "RGB")
    return np.asarray(im.resize([ow, oh], resample=Image.BICUBIC)).reshape(oh, ow, img.shape[2])


def _images(shape, channels, seed):
    """n = 2 images per call: (random, checkerboard) and (0 / 255 noise, inverted checkerboard)."""
    rng = np.random.default_rng(seed)
    board = M.checkerboard(shape[0], shape[1], channels)
    return [np.stack([rng.integers(0, 256, shape + (channels,), dtype=np.uint8), board]),
            np.stack([rng.choice(np.array([0, 255], np.uint8), shape + (channels,)), 255 - board])]


@pytest.fixture(scope="module")
def eng(oracle):
    from dcscn_amd import engine
    cfg = oracle.make_config(layers=2, filters=8, min_filters=8)
    e = engine.Engine(cfg, device=0)                      # no weights: the resize is usable before finalize
    yield e
    e.close()


def _check(eng, shape, out, channels):
    for batch in _images(shape, channels, shape[0] * 1000 + out[1] * 7 + channels):
        got = eng.resize_bicubic_bytes(batch, out[0], out[1])
        assert got.dtype == np.uint8 and got.shape == (2,) + out + (channels,)
        for i in range(2):
            ref = _pil(batch[i], out[0], out[1])
            assert np.array_equal(got[i], ref), "image %d: %d bytes differ" % (i, int(np.count_nonzero(got[i] != ref)))


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("shape,out", M.SHAPES)
def test_resize_bytes_is_bit_identical_to_pillow(eng, shape, out, channels):
    _check(eng, shape, out, channels)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("out_w", [5, 6, 7, 8])
def test_rows_that_end_at_every_byte_of_a_dword(eng, out_w, channels):
    """Output rows of out_w * channels bytes, every residue mod 4: dwords that straddle two rows, and the bytewise tail."""
    _check(eng, (6, 3), (9, out_w), channels)             # both passes
    _check(eng, (9, 3), (9, out_w), channels)             # the horizontal pass writes the result
    _check(eng, (6, out_w), (9, out_w), channels)         # the vertical pass alone


def test_single_images_keep_their_layout(eng):
    rng = np.random.default_rng(1)
    grey = rng.integers(0, 256, (11, 13), dtype=np.uint8)
    rgb = rng.integers(0, 256, (11, 13, 3), dtype=np.uint8)
    assert np.array_equal(eng.resize_bicubic_bytes(grey, 22, 26), _pil(grey[:, :, None], 22, 26)[:, :, 0])
    assert np.array_equal(eng.resize_bicubic_bytes(rgb, 22, 26), _pil(rgb, 22, 26))


def test_device_form_on_a_second_stream_at_an_odd_address(eng):
    """dcscn_resize_bicubic_bytes_device on a stream of the caller's, then dcscn_synchronize; the output starts one byte past
    a dword (a bytewise head), and the bytes around it stay as they were."""
    from test_hip_parity import _Hip
    rng = np.random.default_rng(2)
    batch = rng.integers(0, 256, (2, 17, 33, 3), dtype=np.uint8)
    oh, ow = 51, 99
    n_out = 2 * oh * ow * 3
    guard = np.full((n_out + 8 + 3) // 4 * 4, 77, np.uint8)
    hip = _Hip()
    try:
        src, dst = hip.upload(batch), hip.upload(guard)
        assert dst % 4 == 0
        eng.resize_bicubic_bytes_device(src, dst + 1, 2, 17, 33, 3, oh, ow, stream=hip.stream())
        eng.synchronize()
        got = hip.download(dst, (guard.size // 4,)).view(np.uint8)
    finally:
        hip.close()
    assert got[0] == 77 and np.all(got[1 + n_out:] == 77)
    got = got[1:1 + n_out].reshape(2, oh, ow, 3)
    for i in range(2):
        assert np.array_equal(got[i], _pil(batch[i], oh, ow))


def test_refusals(eng):
    import ctypes
    from dcscn_amd import engine
    img = np.zeros((2, 8, 8, 2), np.uint8)
    with pytest.raises(engine.EngineError) as e:
        eng.resize_bicubic_bytes(img, 16, 16)                         # channels = 2
    assert e.value.status == 1 and "channels" in e.value.message
    for oh, ow in ((0, 16), (16, 0)):
        with pytest.raises(engine.EngineError) as e:
            eng.resize_bicubic_bytes(np.zeros((8, 8, 3), np.uint8), oh, ow)
        assert e.value.status == 1
    with pytest.raises(engine.EngineError) as e:
        eng.resize_bicubic_bytes(np.zeros((0, 8, 3), np.uint8), 4, 4)
    assert e.value.status == 1
    lib, u8 = engine.load_library(), ctypes.POINTER(ctypes.c_uint8)
    buf = np.zeros((8, 8), np.uint8)
    assert lib.dcscn_resize_bicubic_bytes(eng._h, None, buf.ctypes.data_as(u8), 1, 8, 8, 1, 8, 8) == 1
    assert lib.dcscn_resize_bicubic_bytes(eng._h, buf.ctypes.data_as(u8), None, 1, 8, 8, 1, 8, 8) == 1
    assert lib.dcscn_resize_bicubic_bytes_device(eng._h, None, None, 1, 8, 8, 1, 8, 8, None) == 1
    assert lib.dcscn_resize_bicubic_bytes(None, buf.ctypes.data_as(u8), buf.ctypes.data_as(u8), 1, 8, 8, 1, 8, 8) == 1
    with pytest.raises(engine.EngineError):
        eng.resize_bicubic_bytes(np.zeros((8, 8), np.float32), 16, 16)
