"""dcscn_sr_rgb_bytes: sr.py's colour branch from one upload of the uint8 RGB image, every result as the bytes save_image writes.
What it must return is fixed by code that exists without it, plus save_image's cast (resize_bytes_model.cast_rule: truncate
toward zero, keep the low 8 bits -- the reference wraps values outside 0..255, it does not clip):
  rgb_bicubic == Pillow's RGB BICUBIC;  y_bicubic == rule(dcscn_resize_bicubic(float32(Y)));
  y_out, rgb_out == rule(the y and rgb of dcscn_sr_rgb fed with Pillow's upscaled image).
The bar is equality of every byte."""
import os

import numpy as np
import pytest
from PIL import Image

import resize_bytes_model as M
from conftest import CONFIGS, GOLDEN
from test_golden_hip import _model

pytestmark = pytest.mark.gpu

ALL = ("rgb_bicubic", "y_bicubic", "y_out", "rgb_out")


def _pil_rgb(img, scale):
    h, w = img.shape[:2]
    return np.asarray(Image.fromarray(img, "RGB").resize([w * scale, h * scale], resample=Image.BICUBIC))


def _expected(eng, img, n_ensemble):
    """(the four expected uint8 arrays, the float y and rgb that reach the casts)"""
    from dcscn_amd import imaging
    s = eng.scale
    h, w = img.shape[:2]
    up = _pil_rgb(img, s)
    y32 = imaging.convert_rgb_to_y(img).astype(np.float32).reshape(h, w)
    y, rgb = eng.sr_rgb(img, up, n_ensemble)
    want = {"rgb_bicubic": up, "y_bicubic": M.cast_rule(eng.resize_bicubic(y32, s * h, s * w))[:, :, None],
            "y_out": M.cast_rule(y), "rgb_out": M.cast_rule(rgb)}
    return want, y, rgb


def _outside(values):
    return int(np.count_nonzero(values < 0)), int(np.count_nonzero(values >= 256))


def _assert_same(got, want, names, what):
    assert sorted(got) == sorted(names)
    for k in names:
        assert got[k].dtype == np.uint8 and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(got[k], want[k]), "%s %s: %d bytes differ" % (what, k, int(np.count_nonzero(got[k] != want[k])))


@pytest.mark.parametrize("key,crop,n_ensemble", [("L7_x2", (96, 80), 1), ("L7_x2", (96, 80), 8), ("L7_x3", (40, 33), 1),
                                                 ("L7_x4", (40, 33), 1)])
def test_sr_rgb_bytes_on_the_golden_models(tmp_path, key, crop, n_ensemble):
    """The first three Set5 images, cropped.  With the golden weights the RGB recombination leaves 0..255 on both sides on these
    crops (float64 oracle: 718 values < 0 and 5 >= 256 at x2, 205 and 1 at x3, 391 and 9 at x4), so rgb_out's cast wraps."""
    g, m = _model(tmp_path, key, self_ensemble=n_ensemble)
    eng = m._ready_engine()
    below = above = 0
    for i, f in enumerate(g["files"][:3]):
        img = np.ascontiguousarray(np.asarray(Image.open(os.path.join(GOLDEN, "set5", f)).convert("RGB"))[:crop[0], :crop[1]])
        want, y, rgb = _expected(eng, img, n_ensemble)
        lo, hi = _outside(rgb)
        print("%s %s ensemble %d: %d values < 0, %d values >= 256 reach the rgb_out cast" % (key, f, n_ensemble, lo, hi))
        below, above = below + lo, above + hi
        _assert_same(eng.sr_rgb_bytes(img, n_ensemble), want, ALL, f)
        if i == 0:                                        # one at a time: the same bytes as all together
            for k in ALL:
                _assert_same(eng.sr_rgb_bytes(img, n_ensemble, want=(k,)), want, (k,), f + " alone")
            _assert_same(eng.sr_rgb_bytes(img, n_ensemble, want=("y_bicubic", "rgb_bicubic")), want, ("rgb_bicubic", "y_bicubic"), f)
    m.close()
    assert below >= 1 and above >= 1, (below, above)


def test_y_out_wraps_where_the_network_leaves_the_range(oracle):
    """A 0 / 255 checkerboard through seeded synthetic weights: the bicubic of its Y overshoots to about -26 and 277 in the
    corners and the network's Y follows it (float64 oracle, seed 0: 2 values < 0 and 2 >= 256 in Y, 6 and 6 in the RGB), so
    the casts of y_bicubic, y_out and rgb_out all wrap."""
    from dcscn_amd import engine
    cfg = oracle.make_config(**CONFIGS["L7_F32to8_x2"])
    img = M.checkerboard(24, 20, 3)
    with engine.Engine(cfg, device=0) as eng:
        eng.load_weights(oracle.synthetic_weights(cfg, seed=0))
        for n_ensemble in (1, 2):
            want, y, rgb = _expected(eng, img, n_ensemble)
            print("ensemble %d: Y %s, RGB %s values (< 0, >= 256)" % (n_ensemble, _outside(y), _outside(rgb)))
            assert min(_outside(y)) >= 1 and min(_outside(rgb)) >= 1
            _assert_same(eng.sr_rgb_bytes(img, n_ensemble), want, ALL, "checkerboard")


def test_refusals(oracle):
    import ctypes
    from dcscn_amd import engine
    cfg = oracle.make_config(**CONFIGS["L7_F32to8_x2"])
    img = M.checkerboard(8, 8, 3)
    with engine.Engine(cfg, device=0) as eng:
        with pytest.raises(engine.EngineError) as e:
            eng.sr_rgb_bytes(img)                                     # before finalize
        assert e.value.status == 6
        eng.load_weights(oracle.synthetic_weights(cfg, seed=0))
        u8 = ctypes.POINTER(ctypes.c_uint8)
        out = np.empty((16, 16, 3), np.uint8)
        lib = engine.load_library()
        assert lib.dcscn_sr_rgb_bytes(eng._h, img.ctypes.data_as(u8), 8, 8, 1, None, None, None, None) == 1
        assert lib.dcscn_sr_rgb_bytes(eng._h, None, 8, 8, 1, out.ctypes.data_as(u8), None, None, None) == 1
        assert lib.dcscn_sr_rgb_bytes(eng._h, img.ctypes.data_as(u8), 8, 8, 9, out.ctypes.data_as(u8), None, None, None) == 1
        assert lib.dcscn_sr_rgb_bytes(eng._h, img.ctypes.data_as(u8), 0, 8, 1, out.ctypes.data_as(u8), None, None, None) == 1
        with pytest.raises(engine.EngineError):
            eng.sr_rgb_bytes(img, want=("rgb",))
        with pytest.raises(engine.EngineError):
            eng.sr_rgb_bytes(img[:, :, 0])


def _files(folder):
    return {n: np.asarray(Image.open(os.path.join(folder, n))) for n in sorted(os.listdir(folder))}


@pytest.mark.parametrize("mode,size", [("L", (48, 40)), ("RGB", (64, 48))])
def test_do_for_file_writes_the_same_files_with_and_without_the_device_byte_paths(tmp_path, mode, size):
    """sr.py's work on a grey PNG (the uint8 resizes through dcscn_resize_bicubic_bytes) and on an RGB one (dcscn_sr_rgb_bytes)
    against the host path -- Pillow and numpy -- forced as test_color_hip forces it: the same files, the same pixels."""
    g, m = _model(tmp_path, "L7_x2")
    src = os.path.join(GOLDEN, "set5", g["files"][2])
    crop = tmp_path / "in.png"
    Image.open(src).convert(mode).crop((0, 0, size[1], size[0])).save(crop)
    loaded = np.asarray(Image.open(crop))
    assert m._device_byte_resize(loaded) and m._device_colour_path(loaded) == (mode == "RGB")
    m.do_for_file(str(crop), str(tmp_path / "dev"))
    m._device_byte_resize = lambda image: False
    m._device_colour_path = lambda image: False
    m.do_for_file(str(crop), str(tmp_path / "host"))
    dev, host = _files(tmp_path / "dev" / m.name), _files(tmp_path / "host" / m.name)
    assert sorted(dev) == sorted(host) == ["in.png", "in_bicubic.png", "in_bicubic_y.png", "in_result.png"] + (
        ["in_result_y.png"] if mode == "RGB" else [])
    for name in dev:
        assert dev[name].shape == host[name].shape and np.array_equal(dev[name], host[name]), name
    m.close()
