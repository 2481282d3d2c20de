"""helper/loader.py DynamicDataSets.next_patch: the patch descriptors the device batches are built from draw exactly what
load_batch_image draws, and cutting a descriptor out of the cached image gives load_batch_image's y.  No GPU needed."""
import os
import random

import numpy as np
import pytest
from PIL import Image

from conftest import GOLDEN


def _dataset(data_dir, scale, size):
    from helper import loader
    d = loader.DynamicDataSets(scale, size)
    d.set_data_dir(data_dir)
    return d


def _synthetic_dir(tmp_path, hr):
    """RGBA, LA, RGB, L images of odd sizes, one exactly hr x hr, and one smaller than a patch (skipped by the loader)."""
    rng = np.random.default_rng(1)
    d = tmp_path / "images"
    d.mkdir()
    shapes = [("rgba.png", "RGBA", (hr + 2, hr + 8, 4)), ("la.png", "LA", (hr + 1, 2 * hr + 1, 2)), ("exact.png", "RGB", (hr, hr, 3)),
              ("grey.png", "L", (hr, 3 * hr - 1)), ("odd.png", "RGB", (2 * hr + 11, hr + 14, 3)), ("small.png", "RGB", (hr - 1, 4 * hr, 3))]
    for name, mode, shape in shapes:
        Image.fromarray(rng.integers(0, 256, shape, dtype=np.uint8), mode).save(str(d / name))
    return str(d)


def _check_draws(data_dir, scale, size, count, seed, capsys=None):
    d = _dataset(data_dir, scale, size)
    random.seed(seed)
    d.init_batch_index()
    patches = [d.next_patch() for _ in range(count)]
    after_patches = random.getstate()
    h = _dataset(data_dir, scale, size)
    random.seed(seed)
    h.init_batch_index()
    host = [h.load_batch_image(255.0) for _ in range(count)]
    assert random.getstate() == after_patches
    from dcscn_amd import imaging as util
    hr = size * scale
    for (filename, top, left, fliplr), (_, _, y) in zip(patches, host):
        assert fliplr in (0, 1)
        crop = d.image(filename)[top:top + hr, left:left + hr, :]
        assert crop.shape[:2] == (hr, hr)
        want = util.convert_rgb_to_y(crop)
        if fliplr:
            want = np.fliplr(want)
        assert want.dtype == y.dtype and want.shape == y.shape
        assert np.array_equal(want, y), filename
    return patches


@pytest.mark.parametrize("scale,size", [(2, 48), (3, 48), (4, 32)])
def test_next_patch_consumes_random_as_load_batch_image_on_set14(scale, size):
    patches = _check_draws(os.path.join(GOLDEN, "set14"), scale, size, 40, seed=scale)    # 40 draws: two reshuffles of the 14 images
    assert {p[3] for p in patches} == {0, 1}
    assert any(p[0].endswith("img_003.png") for p in patches)                                # the grey image of Set14


def test_next_patch_skips_small_images_and_crops_exact_ones(tmp_path):
    scale, size = 3, 5
    data_dir = _synthetic_dir(tmp_path, scale * size)
    patches = _check_draws(data_dir, scale, size, 30, seed=11)
    names = {os.path.basename(p[0]) for p in patches}
    assert "small.png" not in names and {"rgba.png", "la.png", "exact.png", "grey.png", "odd.png"} <= names
    assert all((p[1], p[2]) == (0, 0) for p in patches if p[0].endswith("exact.png"))
