"""The 8-fold augmented training set without its files (helper/loader.py DynamicDataSets(augment_level=N)): the eight variants against
numpy, augmentation.py and convert_y.py as command-line tools, and the virtual dataset against the on-disk one augmentation.py's files
make -- the same draws, the same arrays, the same ``random`` state.  No GPU needed."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

from conftest import GOLDEN, ROOT
from test_train_batches_host import _synthetic_dir

SUFFIXES = ("", "_v", "_h", "_hv", "_r1", "_r2", "_r1_v", "_r2_v")
# the numpy expression of every code (include/dcscn.h, DCSCN_AUG_*)
NUMPY = (lambda m: m, np.flipud, np.fliplr, lambda m: np.flipud(np.fliplr(m)), np.rot90, lambda m: np.rot90(m, -1),
         lambda m: np.flipud(np.rot90(m)), lambda m: np.flipud(np.rot90(m, -1)))


# out[i, j] of the table in include/dcscn.h as the source's (row, column), for a source [H, W]
INDEX_MAP = (lambda H, W, i, j: (i, j), lambda H, W, i, j: (H - 1 - i, j), lambda H, W, i, j: (i, W - 1 - j),
             lambda H, W, i, j: (H - 1 - i, W - 1 - j), lambda H, W, i, j: (j, W - 1 - i), lambda H, W, i, j: (H - 1 - j, i),
             lambda H, W, i, j: (j, i), lambda H, W, i, j: (H - 1 - j, W - 1 - i))


@pytest.mark.parametrize("channels", [3, 1])
def test_augment_is_the_numpy_expression_and_the_index_map_of_every_code(channels):
    from dcscn_amd import imaging as util
    assert tuple(util.AUGMENT_SUFFIXES) == SUFFIXES
    m = np.random.default_rng(channels).integers(0, 256, (5, 7, channels), dtype=np.uint8)
    for code in range(8):
        got = util.augment(m, code)
        assert got.shape == ((5, 7, channels) if code < 4 else (7, 5, channels)), code
        assert np.array_equal(got, NUMPY[code](m)), code
        assert np.shares_memory(got, m), code                                   # a view: nothing is copied per variant
        for i in range(got.shape[0]):
            for j in range(got.shape[1]):
                assert np.array_equal(got[i, j], m[INDEX_MAP[code](5, 7, i, j)]), (code, i, j)
    for code in (-1, 8):
        with pytest.raises(ValueError):
            util.augment(m, code)


def _png_dir(tmp_path):
    """data/few/: two RGB images and a grey one, none square."""
    rng = np.random.default_rng(3)
    d = tmp_path / "data" / "few"
    d.mkdir(parents=True)
    for name, shape in (("a.png", (9, 13, 3)), ("b.png", (12, 5, 3)), ("g.png", (6, 11))):
        Image.fromarray(rng.integers(0, 256, shape, dtype=np.uint8)).save(str(d / name))
    return d


def _run(tmp_path, script, *argv):
    return subprocess.run([sys.executable, os.path.join(ROOT, script), "--data_dir=" + str(tmp_path / "data")] + list(argv),
                          cwd=str(tmp_path), capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("level", [3, 8, None])
def test_augmentation_py_writes_the_variants_under_their_suffixes(tmp_path, level):
    from dcscn_amd import imaging as util
    src = _png_dir(tmp_path)
    p = _run(tmp_path, "augmentation.py", "--dataset=few", *([] if level is None else ["--augment_level=%d" % level]))
    assert p.returncode == 0, p.stdout + p.stderr
    level = 4 if level is None else level                                        # the reference's default
    out = tmp_path / "data" / ("few_%d" % level)
    assert sorted(os.listdir(str(out))) == sorted(stem + SUFFIXES[c] + ".png" for stem in "abg" for c in range(level))
    for stem in "abg":
        original = util.load_image(str(src / (stem + ".png")), print_console=False)
        for code in range(level):
            got = util.load_image(str(out / (stem + SUFFIXES[code] + ".png")), print_console=False)
            assert got.dtype == np.uint8 and np.array_equal(got, util.augment(original, code)), (stem, code)


def test_convert_y_py_writes_the_luma_as_bmp_and_passes_grey_files_through(tmp_path):
    from dcscn_amd import imaging as util
    src = _png_dir(tmp_path)
    p = _run(tmp_path, "convert_y.py", "--dataset=few")
    assert p.returncode == 0, p.stdout + p.stderr
    out = tmp_path / "data" / "few_y"
    assert sorted(os.listdir(str(out))) == ["a.bmp", "b.bmp", "g.bmp"]
    for stem in "abg":
        original = util.load_image(str(src / (stem + ".png")), print_console=False)
        got = util.load_image(str(out / (stem + ".bmp")), print_console=False)
        assert got.shape == original.shape[:2] + (1,) and got.dtype == np.uint8
        want = original if stem == "g" else util.convert_rgb_to_y(original).astype(np.uint8)
        assert np.array_equal(got, want), stem


@pytest.mark.parametrize("script,extra", [("augmentation.py", ["--augment_level=2"]), ("convert_y.py", [])])
def test_the_tools_refuse_unknown_arguments(tmp_path, script, extra):
    _png_dir(tmp_path)
    p = _run(tmp_path, script, "--dataset=few", "--no_such_flag=1", *extra)
    assert p.returncode != 0 and "no_such_flag" in p.stderr
    p = _run(tmp_path, script, "--dataset=few", "stray", "words", *extra)
    assert "Unknown args" in p.stdout
    assert sorted(os.listdir(str(tmp_path / "data"))) == ["few"]                # nothing was written


def _write_level8(data_dir, out_dir):
    """The files augmentation.py --augment_level 8 writes of data_dir; returns them ordered base file (os.listdir order), then code."""
    from dcscn_amd import imaging as util
    os.makedirs(out_dir)
    base = util.get_files_in_directory(data_dir)
    copies = []
    for path in base:
        stem, ext = os.path.splitext(os.path.basename(path))
        for code in range(8):
            copies.append(os.path.join(out_dir, stem + SUFFIXES[code] + ext))
            util.save_image(copies[-1], util.augment(util.load_image(path, print_console=False), code), print_console=False)
    return base, copies


@pytest.mark.parametrize("scale,size", [(2, 7), (4, 3)])
def test_virtual_level_8_dataset_equals_the_dataset_on_disk(tmp_path, scale, size):
    from helper import loader
    hr = scale * size
    base, copies = _write_level8(_synthetic_dir(tmp_path, hr), str(tmp_path / "images_8"))
    disk = loader.DynamicDataSets(scale, size)
    disk.filenames, disk.count = copies, len(copies)
    virtual = loader.DynamicDataSets(scale, size, augment_level=8)
    virtual.filenames, virtual.count = list(base), len(base)
    count = 100                                                                 # 48 entries: two reshuffles
    for max_value in (255.0, 1.0):
        random.seed(17)
        disk.init_batch_index()
        want_patches = [disk.next_patch() for _ in range(count)]
        random.seed(17)
        disk.init_batch_index()
        want = [disk.load_batch_image(max_value) for _ in range(count)]
        want_state = random.getstate()

        random.seed(17)
        virtual.init_batch_index()
        assert virtual.count == len(copies) and virtual.entries == [(f, c) for f in base for c in range(8)]
        got_patches = [virtual.next_patch() for _ in range(count)]
        assert random.getstate() == want_state
        random.seed(17)
        virtual.init_batch_index()
        got = [virtual.load_batch_image(max_value) for _ in range(count)]
        assert random.getstate() == want_state

        assert [p[1:4] for p in got_patches] == [p[1:] for p in want_patches]
        for g, w in zip(got_patches, want_patches):                             # ... and the same file of the on-disk set
            assert len(g) == 5 and len(w) == 4
            stem, ext = os.path.splitext(os.path.basename(g[0]))
            assert os.path.basename(w[0]) == stem + SUFFIXES[g[4]] + ext, (g, w)
        assert {p[4] for p in got_patches} == set(range(8)) and {p[3] for p in got_patches} == {0, 1}
        assert "small.png" not in {os.path.basename(p[0]) for p in got_patches}
        for i, (g, w) in enumerate(zip(got, want)):
            for name, a, b in zip(("x", "x2", "y"), g, w):
                assert a.dtype == b.dtype and a.shape == b.shape, (i, name)
                assert np.array_equal(a, b), (i, name, got_patches[i])
    assert len(virtual._cache) == len(base)                                     # one decode per base file


@pytest.mark.parametrize("level", [0, 1])
def test_levels_0_and_1_are_the_plain_dataset(tmp_path, level):
    from helper import loader
    data_dir = _synthetic_dir(tmp_path, 14)
    plain = loader.DynamicDataSets(2, 7)
    plain.set_data_dir(data_dir)
    d = loader.DynamicDataSets(2, 7, augment_level=level)
    d.set_data_dir(data_dir)
    assert d.count == plain.count == 6
    random.seed(9)
    plain.init_batch_index()
    want = [plain.next_patch() for _ in range(20)]
    want_state = random.getstate()
    random.seed(9)
    d.init_batch_index()
    assert d.count == 6 and len(d.batch_index) == 6
    got = [d.next_patch() for _ in range(20)]
    assert got == want and all(len(p) == 4 for p in got)
    assert random.getstate() == want_state


def test_model_passes_the_flag_to_its_dataset(tmp_path):
    from dcscn_amd.model import SuperResolution
    from helper import args
    from test_host import _flags
    flag = args.FLAGS._flags["train_augment_level"]
    assert flag.kind == "integer" and flag.default == 0
    for level, entries in ((0, 14), (8, 112)):
        m = SuperResolution(_flags(checkpoint_dir=str(tmp_path / "models"), train_augment_level=level))
        m.load_dynamic_datasets(os.path.join(GOLDEN, "set14"), 16)
        m.train.init_batch_index()
        assert m.train.augment_level == level and m.train.count == entries


@pytest.mark.parametrize("level", [9, -1])
def test_train_py_refuses_a_level_outside_0_to_8(tmp_path, level):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--train_augment_level=%d" % level, "--data_dir=" + GOLDEN,
                        "--dataset=set14", "--checkpoint_dir=" + str(tmp_path / "models")], cwd=str(tmp_path), capture_output=True,
                       text=True, timeout=120)
    assert p.returncode != 0
    assert "--train_augment_level %d is not one of 0 .. 8" % level in p.stdout
