"""Training batches built on the device (dcscn_train_build_batch / dcscn_train_step_patches) against the host loader
(helper/loader.py DynamicDataSets.load_batch_image) at run time, bit for bit, and the training driver through them."""
import os
import random

import numpy as np
import pytest

from conftest import CONFIGS, GOLDEN
from test_host import _flags
from test_train_batches_host import _dataset, _synthetic_dir

pytestmark = pytest.mark.gpu

FLAGS = dict(optimizer="adam", beta1=0.9, beta2=0.999, epsilon=1e-8, momentum=0.9, l2_decay=1e-4, clipping_norm=5.0, dropout_rate=0.8)
SET14 = os.path.join(GOLDEN, "set14")


def _engine(oracle, scale, begin=True):
    from dcscn_amd import engine
    cfg = oracle.make_config(**CONFIGS["L7_F32to8_x%d" % scale])
    eng = engine.Engine(cfg, device=0)
    eng.load_weights(oracle.synthetic_weights(cfg, seed=0))
    if begin:
        eng.train_begin(FLAGS)
    return eng


def _draw(data_dir, scale, size, count, seed, max_value):
    """count descriptors from next_patch and, from the same random state, load_batch_image's arrays."""
    d = _dataset(data_dir, scale, size)
    random.seed(seed)
    d.init_batch_index()
    patches = [d.next_patch() for _ in range(count)]
    random.seed(seed)
    d.init_batch_index()
    host = [d.load_batch_image(max_value) for _ in range(count)]
    want = [np.stack([np.asarray(h[k], np.float32) for h in host]) for k in range(3)]
    return d, patches, want


def _check_batch(eng, d, patches, size, max_value, want):
    ids = {}
    for f, _, _, _ in patches:
        if f not in ids:
            ids[f] = eng.train_add_image(d.image(f))
    got = eng.train_build_batch([(ids[f], t, l, fl) for f, t, l, fl in patches], size, max_value)
    for name, g, w in zip(("x", "x2", "y_true"), got, want):
        assert g.shape == w.shape, (name, g.shape, w.shape)
        bad = np.flatnonzero(g.view(np.uint32) != w.view(np.uint32))
        assert bad.size == 0, "%s: %d values differ, first at %d: %r vs %r" % (name, bad.size, bad[0], g.flat[bad[0]], w.flat[bad[0]])


@pytest.mark.parametrize("scale,size", [(2, 48), (3, 48), (4, 32)])
@pytest.mark.parametrize("max_value", [255.0, 1.0])
def test_set14_batches_equal_the_host_loader(oracle, scale, size, max_value):
    d, patches, want = _draw(SET14, scale, size, 20, seed=scale, max_value=max_value)
    assert {p[3] for p in patches} == {0, 1}
    channels = {d.image(p[0]).shape[2] for p in patches}
    assert channels == {1, 3}, channels                  # img_003 is grey: one batch mixes L and RGB patches
    with _engine(oracle, scale) as eng:
        _check_batch(eng, d, patches, size, max_value, want)


@pytest.mark.parametrize("scale,size", [(2, 7), (3, 5), (4, 3)])
@pytest.mark.parametrize("max_value", [255.0, 1.0])
def test_synthetic_images_equal_the_host_loader(oracle, tmp_path, scale, size, max_value):
    """RGBA and LA files, odd sizes, an image of exactly one patch (top = left = 0), grey and RGB patches in one batch."""
    data_dir = _synthetic_dir(tmp_path, scale * size)
    d, patches, want = _draw(data_dir, scale, size, 24, seed=5, max_value=max_value)
    names = {os.path.basename(p[0]) for p in patches}
    assert {"rgba.png", "la.png", "exact.png", "grey.png", "odd.png"} <= names
    with _engine(oracle, scale) as eng:
        _check_batch(eng, d, patches, size, max_value, want)


def _train(tmp_path, weights, device_batches, steps=12):
    from dcscn_amd.model import SuperResolution
    m = SuperResolution(_flags(checkpoint_dir=str(tmp_path), batch_num=20, batch_image_size=48, self_ensemble=1, **CONFIGS["L7_F32to8_x2"]))
    m.build_graph()
    m.build_optimizer()
    m.load_weights(weights)
    m.load_dynamic_datasets(SET14, 48)
    m.init_train_step()
    random.seed(1234)
    m.init_epoch_index()
    losses = []
    for _ in range(steps):
        if device_batches:
            m.build_input_batch()
        else:
            for i in range(m.batch_num):
                m.batch_input[i], m.batch_input_bicubic[i], m.batch_true[i] = m.train.load_batch_image(m.max_value)
        m.train_batch()
        losses.append(m.training_loss_sum)
    tensors = m._training_tensors()
    m.close()
    return losses, tensors


def test_train_batch_on_device_batches_equals_host_batches(oracle, tmp_path):
    cfg = oracle.make_config(**CONFIGS["L7_F32to8_x2"])
    weights = oracle.synthetic_weights(cfg, seed=0)
    dev_losses, dev = _train(tmp_path / "dev", weights, True)
    host_losses, host = _train(tmp_path / "host", weights, False)
    assert dev_losses == host_losses
    assert set(dev) == set(host) and len(dev) == 3 * len(weights) + 2
    for k in dev:
        assert np.array_equal(np.asarray(dev[k]).view(np.uint32), np.asarray(host[k]).view(np.uint32)), k


def test_bad_patches_and_calls_before_train_begin_are_refused(oracle):
    from dcscn_amd.engine import EngineError
    image = np.zeros((40, 30, 3), np.uint8)
    with _engine(oracle, 2, begin=False) as eng:
        for call in (lambda: eng.train_add_image(image), lambda: eng.train_build_batch([(0, 0, 0, 0)], 8),
                     lambda: eng.train_step_patches([(0, 0, 0, 0)], 8, 1e-3)):
            with pytest.raises(EngineError) as e:
                call()
            assert e.value.status == 6, e.value                        # DCSCN_ERR_STATE
    with _engine(oracle, 2) as eng:
        for channels in (2, 4):
            with pytest.raises(EngineError) as e:
                eng.train_add_image(np.zeros((40, 30, channels), np.uint8))
            assert e.value.status == 1 and "channels" in e.value.message
        assert eng.train_add_image(image) == 0                         # 40 x 30, 16 x 16 patches at lr_size 8
        ok = (0, 24, 14, 1)
        bad = [([ok, (1, 0, 0, 0)], 8, 255.0, "patch 1: unknown image"),
               ([ok, (-1, 0, 0, 0)], 8, 255.0, "patch 1: unknown image"),
               ([(0, 25, 0, 0)], 8, 255.0, "patch 0: the 16 x 16 crop"),
               ([ok, (0, 0, 15, 0)], 8, 255.0, "patch 1: the 16 x 16 crop"),
               ([(0, -1, 0, 0)], 8, 255.0, "patch 0: the 16 x 16 crop"),
               ([ok, ok, (0, 0, 0, 2)], 8, 255.0, "patch 2: fliplr"),
               ([ok], 0, 255.0, "lr_size"),
               ([ok], 8, 0.0, "max_value"),
               ([ok], 8, -1.0, "max_value"),
               ([], 8, 255.0, "patches")]
        for patches, lr_size, max_value, msg in bad:
            for call in (lambda: eng.train_build_batch(patches, lr_size, max_value),
                         lambda: eng.train_step_patches(patches, lr_size, 1e-3, max_value)):
                with pytest.raises(EngineError) as e:
                    call()
                assert e.value.status == 1 and msg in e.value.message, (patches, e.value)
        x, x2, y = eng.train_build_batch([ok], 8)                      # the handle still works
        assert x.shape == (1, 8, 8, 1) and x2.shape == y.shape == (1, 16, 16, 1) and np.all(y == 16.0)      # Y of black
        assert len(eng.train_step_patches([ok, ok], 8, 1e-3)) == 4


# ---------------------------------------------------------------------------------------------
# batches of more than 32 patches: batch_gather and batch_finish are launched once per 32 patches (kChunk of csrc/train_data.hip),
# their outputs offset by whole chunks, and the slot numbers of the grey and of the RGB patches run on across the launches
# ---------------------------------------------------------------------------------------------
CHUNK = 32


def _kinds(d, patches):
    """Channels of every patch's image: 1 = grey (uint8 planes on the device), 3 = RGB (float planes)."""
    return [d.image(p[0]).shape[2] for p in patches]


def _seed_where(data_dir, scale, size, count, accept):
    """The first draw seed whose ``count`` patches' kinds satisfy ``accept`` (the order of the files of a directory, and with it
    what a seed draws, is the file system's: the seed is searched, on the CPU, and the property asserted)."""
    d = _dataset(data_dir, scale, size)
    for seed in range(1, 200):
        random.seed(seed)
        d.init_batch_index()
        if accept(_kinds(d, [d.next_patch() for _ in range(count)])):
            return seed
    raise AssertionError("no seed below 200 draws the batch this test needs")


def _both_sides(kinds):
    """Grey and RGB patches below index 32 and at or above it."""
    return set(kinds[:CHUNK]) == {1, 3} and set(kinds[CHUNK:]) == {1, 3}


def _assert_crosses(kinds, count, last=None):
    assert len(kinds) == count > CHUNK
    assert set(kinds[:CHUNK]) == {1, 3}, kinds
    if last is None:
        assert set(kinds[CHUNK:]) == {1, 3}, kinds
    else:
        assert kinds[CHUNK:] == [last], kinds                # 33 patches: the one patch of the second launch, of the kind asked for
    for kind in set(kinds[CHUNK:]):
        # a patch of the second launch takes a slot behind the patches of its kind in the first: the carry-over of the slot numbers
        assert kinds[:CHUNK].count(kind) >= 1, (kind, kinds)


def _crossing_cases(data_dir, scale, size):
    """(count, seed, kind of patch 32 or None): 64 and 65 patches with both kinds on both sides of index 32, and 33 patches twice,
    patch 32 once grey and once RGB (one draw of 33 has a single patch at or above 32, so two draws cover both kinds there)."""
    cases = [(count, _seed_where(data_dir, scale, size, count, _both_sides), None) for count in (64, 65)]
    for last in (1, 3):
        cases.append((33, _seed_where(data_dir, scale, size, 33, lambda k: set(k[:CHUNK]) == {1, 3} and k[CHUNK] == last), last))
    return cases


def _check_crossing(oracle, data_dir, scale, size, cases):
    with _engine(oracle, scale) as eng:
        for i, (count, seed, last) in enumerate(cases):
            max_value = (255.0, 1.0)[i % 2]
            d, patches, want = _draw(data_dir, scale, size, count, seed=seed, max_value=max_value)
            kinds = _kinds(d, patches)
            _assert_crosses(kinds, count, last)
            print("%d patches at scale %d size %d, seed %d, max_value %g: %d grey and %d RGB below index 32, %d and %d from it on"
                  % (count, scale, size, seed, max_value, kinds[:CHUNK].count(1), kinds[:CHUNK].count(3), kinds[CHUNK:].count(1),
                     kinds[CHUNK:].count(3)))
            _check_batch(eng, d, patches, size, max_value, want)


@pytest.mark.parametrize("scale,size", [(2, 7), (4, 3)])
def test_synthetic_batches_across_the_32_patch_launch_equal_the_host_loader(oracle, tmp_path, scale, size):
    data_dir = _synthetic_dir(tmp_path, scale * size)
    _check_crossing(oracle, data_dir, scale, size, _crossing_cases(data_dir, scale, size))


def test_set14_batch_across_the_32_patch_launch_equals_the_host_loader(oracle):
    scale, size = 2, 16
    _check_crossing(oracle, SET14, scale, size, [(65, _seed_where(SET14, scale, size, 65, _both_sides), None)])


def test_step_on_33_patches_equals_the_step_on_the_loaders_arrays(oracle):
    """train_step_patches on 33 patches (the 33rd a grey one, behind grey ones of the first launch) against train_step on what
    load_batch_image cuts of the same patches: stats and state bit for bit, c-DCSCN x2, clipped adam with dropout."""
    scale, size, count = 2, 8, 33
    seed = _seed_where(SET14, scale, size, count, lambda k: set(k[:CHUNK]) == {1, 3} and k[CHUNK] == 1)
    d, patches, want = _draw(SET14, scale, size, count, seed=seed, max_value=255.0)
    _assert_crosses(_kinds(d, patches), count, 1)
    cfg = oracle.make_config(**CONFIGS["L7_F32to8_x2"])
    names = list(oracle.synthetic_weights(cfg, seed=0))
    with _engine(oracle, scale) as dev, _engine(oracle, scale) as host:
        ids = {}
        for f, _, _, _ in patches:
            if f not in ids:
                ids[f] = dev.train_add_image(d.image(f))
        for step in range(2):
            got = dev.train_step_patches([(ids[f], t, l, fl) for f, t, l, fl in patches], size, 1e-3, dropout_key=77 + step)
            ref = host.train_step(*want, 1e-3, dropout_key=77 + step)
            print("step %d: stats %r" % (step, got))
            assert np.array_equal(np.array(got).view(np.uint64), np.array(ref).view(np.uint64)), (got, ref)
            for k in names:
                for s in ("", "/Adam", "/Adam_1", "/grad"):
                    assert np.array_equal(dev.get_tensor(k + s).view(np.uint32), host.get_tensor(k + s).view(np.uint32)), (step, k + s)
            for s in ("beta1_power", "beta2_power"):
                assert np.array_equal(dev.get_tensor(s).view(np.uint32), host.get_tensor(s).view(np.uint32)), (step, s)
