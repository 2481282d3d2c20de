"""Training on the 8-fold augmented set without its files: the dcscn_patch_aug entry points (dcscn_train_build_batch_aug,
dcscn_train_step_patches_aug, dcscn_train_local_gradients_patches_aug) against the host loader's cut of util.augment(image, code) --
which tests/test_train_augment_host.py shows to be the cut of the file augmentation.py writes -- bit for bit, and the training
driver through them."""
import random

import numpy as np
import pytest
import torch            # before the library is loaded: torch initialises HIP first (the records of test 4 are torch tensors)

from conftest import CONFIGS
from test_host import _flags
from test_train_batches_hip import CHUNK, SET14, _engine
from test_train_batches_host import _synthetic_dir

pytestmark = pytest.mark.gpu


def _assert_bits(got, want, what=""):
    for name, g, w in zip(("x", "x2", "y_true"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype == np.float32, (what, name, g.shape, w.shape)
        bad = np.flatnonzero(g.view(np.uint32) != w.view(np.uint32))
        assert bad.size == 0, "%s %s: %d values differ, first at %d: %r vs %r" % (what, name, bad.size, bad[0], g.flat[bad[0]], w.flat[bad[0]])


def _virtual(data_dir, scale, size):
    from helper import loader
    d = loader.DynamicDataSets(scale, size, augment_level=8)
    d.set_data_dir(data_dir)
    return d


def _draw(d, count, seed, max_value):
    """count 5-field descriptors from next_patch and, from the same random state, load_batch_image's arrays as float32."""
    random.seed(seed)
    d.init_batch_index()
    patches = [d.next_patch() for _ in range(count)]
    random.seed(seed)
    d.init_batch_index()
    host = [d.load_batch_image(max_value) for _ in range(count)]
    return patches, [np.stack([np.asarray(h[k], np.float32) for h in host]) for k in range(3)]


def _descriptors(eng, d, patches, ids):
    out = []
    for f, *fields in patches:
        if f not in ids:
            ids[f] = eng.train_add_image(d.image(f))            # the base image: one upload for its eight variants
        out.append((ids[f], *fields))
    return out


def _covers(d, patches):
    """Every code, both fliplr values, grey and RGB patches, and a rotated variant (code >= 4) on both sides of index 32."""
    codes = [p[4] for p in patches]
    return (set(codes) == set(range(8)) and {p[3] for p in patches} == {0, 1} and {d.image(p[0]).shape[2] for p in patches} == {1, 3}
            and max(codes[:CHUNK]) >= 4 and max(codes[CHUNK:]) >= 4)


# ---- 1: drawn batches ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale,size", [(2, 7), (3, 5), (4, 3)])
@pytest.mark.parametrize("max_value", [255.0, 1.0])
def test_drawn_level_8_batches_equal_the_host_loader(oracle, tmp_path, scale, size, max_value):
    d = _virtual(_synthetic_dir(tmp_path, scale * size), scale, size)
    count = 65
    for seed in range(1, 200):                                   # searched on the CPU: what a seed draws depends on the directory's file order
        random.seed(seed)
        d.init_batch_index()
        if _covers(d, [d.next_patch() for _ in range(count)]):
            break
    patches, want = _draw(d, count, seed, max_value)
    assert len(patches) == count and all(len(p) == 5 for p in patches) and _covers(d, patches), patches
    with _engine(oracle, scale) as eng:
        ids = {}
        got = eng.train_build_batch(_descriptors(eng, d, patches, ids), size, max_value)
        assert len(ids) <= 5                                     # the five files that hold a patch, not their 40 variants
    _assert_bits(got, want, "scale %d size %d max_value %g seed %d" % (scale, size, max_value, seed))


# ---- 2: every code x fliplr at the four corners of the transformed image -----------------------------------------------------
def _host_cut(image, patch, scale, size, max_value):
    """load_batch_image's patch of (top, left, fliplr, code), cut from util.augment(image, code)."""
    from dcscn_amd import imaging as util
    from dcscn_amd.model import build_input_image
    top, left, fliplr, code = patch
    hr = scale * size
    y = util.augment(image, code)[top:top + hr, left:left + hr, :]
    assert y.shape[:2] == (hr, hr)
    y = build_input_image(y, channels=1, convert_ycbcr=True)
    if fliplr:
        y = np.fliplr(y)
    x = util.resize_image_by_pil(y, 1 / scale)
    x2 = util.resize_image_by_pil(x, scale)
    if max_value != 255:
        x, x2, y = (np.multiply(a, max_value / 255.0) for a in (x, x2, y))
    return x, x2, y


def _corner_patches(image, hr):
    out = []
    for code in range(8):
        ht, wt = image.shape[:2] if code < 4 else image.shape[1::-1]
        for fliplr in (0, 1):
            for top in (0, ht - hr):
                for left in (0, wt - hr):
                    out.append((top, left, fliplr, code))
    return out


@pytest.mark.parametrize("max_value", [255.0, 1.0])
def test_every_code_and_flip_at_the_corners_equals_the_host_cut(oracle, max_value):
    scale, size = 2, 3
    rng = np.random.default_rng(23)
    images = [rng.integers(0, 256, (11, 17, 3), dtype=np.uint8), rng.integers(0, 256, (13, 8, 1), dtype=np.uint8)]
    with _engine(oracle, scale) as eng:
        rows, want = [], []
        for image in images:
            image_id = eng.train_add_image(image)
            for patch in _corner_patches(image, scale * size):
                rows.append((image_id,) + patch)
                want.append(_host_cut(image, patch, scale, size, max_value))
        assert len(rows) == 2 * 8 * 2 * 4
        got = eng.train_build_batch(rows, size, max_value)
    want = [np.stack([np.asarray(w[k], np.float32) for w in want]) for k in range(3)]
    for i, row in enumerate(rows):                               # per patch, to name the code an index map is wrong for
        _assert_bits([g[i] for g in got], [w[i] for w in want], "patch %d (image, top, left, fliplr, code) = %r" % (i, row))


# ---- 3: refusals -------------------------------------------------------------------------------------------------------------
def test_bad_transforms_and_crops_outside_the_transformed_image_are_refused(oracle):
    from dcscn_amd.engine import EngineError
    with _engine(oracle, 2) as eng:
        assert eng.train_add_image(np.zeros((40, 30, 3), np.uint8)) == 0      # 40 x 30; 16 x 16 patches at lr_size 8
        ok = (0, 24, 14, 1, 3)
        bad = [([ok, (0, 0, 0, 0, -1)], "patch 1: transform -1"),
               ([(0, 0, 0, 0, 8)], "patch 0: transform 8"),
               ([ok, ok, (0, 24, 0, 0, 4)], "patch 2: the 16 x 16 crop"),      # the rotated image is 30 x 40: top <= 14
               ([(0, 0, 24, 0, 0)], "patch 0: the 16 x 16 crop"),
               ([(0, 0, 24, 0, 3)], "patch 0: the 16 x 16 crop"),
               ([(0, 0, 0, 2, 5)], "patch 0: fliplr"),
               ([(1, 0, 0, 0, 5)], "patch 0: unknown image")]
        for patches, msg in bad:
            for call in (lambda: eng.train_build_batch(patches, 8), lambda: eng.train_step_patches(patches, 8, 1e-3)):
                with pytest.raises(EngineError) as e:
                    call()
                assert e.value.status == 1 and msg in e.value.message, (patches, e.value)
        with pytest.raises(EngineError) as e:
            eng.train_build_batch([(0, 24, 0, 0, 4)], 8)
        assert "30 x 40" in e.value.message and "transform 4" in e.value.message, e.value
        with pytest.raises(EngineError) as e:
            eng.train_build_batch([(0, 0, 24, 0, 0)], 8)
        assert "40 x 30" in e.value.message, e.value
        accepted = [[(0, 24, 0, 0)], [(0, 0, 24, 0, 4)], [(0, 14, 24, 1, 7)], [(0, 24, 14, 0, 1), (0, 0, 0, 1)]]
        for patches in accepted:
            x, x2, y = eng.train_build_batch(patches, 8)                      # the handle still works
            assert x.shape == (len(patches), 8, 8, 1) and x2.shape == y.shape == (len(patches), 16, 16, 1) and np.all(y == 16.0)   # Y of black
            assert len(eng.train_step_patches(patches, 8, 1e-3)) == 4


# ---- 4: steps ----------------------------------------------------------------------------------------------------------------
def test_steps_on_5_tuples_equal_the_steps_on_the_host_cut_arrays(oracle):
    """c-DCSCN x2, clipped adam with dropout, two steps on Set14 patches of all eight variants: train_step_patches against train_step
    on what the host loader cuts, and train_local_gradients_patches + train_apply_records(world = 1) against both, bit for bit."""
    scale, size, count = 2, 8, 16
    d = _virtual(SET14, scale, size)
    for seed in range(1, 200):
        random.seed(seed)
        d.init_batch_index()
        patches = [d.next_patch() for _ in range(count)]
        if {p[4] for p in patches} == set(range(8)) and {d.image(p[0]).shape[2] for p in patches} == {1, 3}:
            break
    patches, want = _draw(d, count, seed, 255.0)
    assert {p[4] for p in patches} == set(range(8)) and {d.image(p[0]).shape[2] for p in patches} == {1, 3}, patches
    names = list(oracle.synthetic_weights(oracle.make_config(**CONFIGS["L7_F32to8_x2"]), seed=0))
    state = [k + s for k in names for s in ("", "/Adam", "/Adam_1", "/grad")] + ["beta1_power", "beta2_power"]
    with _engine(oracle, scale) as dev, _engine(oracle, scale) as host, _engine(oracle, scale) as rank:
        rows, rank_rows = _descriptors(dev, d, patches, {}), _descriptors(rank, d, patches, {})
        assert all(len(r) == 5 for r in rows)
        stream = torch.cuda.Stream()
        record = torch.zeros(rank.train_record_floats(), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for step in range(2):
            ref = host.train_step(*want, 1e-3, dropout_key=77 + step)
            got = dev.train_step_patches(rows, size, 1e-3, dropout_key=77 + step)
            rank.train_local_gradients_patches(rank_rows, size, record.data_ptr(), dropout_key=77 + step, first_index=0,
                                               stream=stream.cuda_stream)
            via_record = rank.train_apply_records(record.data_ptr(), 1, 1e-3, stream=stream.cuda_stream)
            print("step %d: stats %r" % (step, got))
            for stats in (got, via_record):
                assert np.array_equal(np.array(stats).view(np.uint64), np.array(ref).view(np.uint64)), (step, stats, ref)
            for k in state:
                w = host.get_tensor(k).view(np.uint32)
                assert np.array_equal(dev.get_tensor(k).view(np.uint32), w), (step, k)
                assert np.array_equal(rank.get_tensor(k).view(np.uint32), w), (step, k, "through the record")


# ---- 5: the model ------------------------------------------------------------------------------------------------------------
def _train(tmp_path, weights, device_batches, steps=6):
    from dcscn_amd.model import SuperResolution
    m = SuperResolution(_flags(checkpoint_dir=str(tmp_path), batch_num=20, batch_image_size=16, self_ensemble=1, train_augment_level=8,
                               **CONFIGS["L7_F32to8_x2"]))
    m.build_graph()
    m.build_optimizer()
    m.load_weights(weights)
    m.load_dynamic_datasets(SET14, 16)
    m.init_train_step()
    random.seed(1234)
    m.init_epoch_index()
    assert m.train.count == 8 * 14
    losses, codes = [], set()
    for _ in range(steps):
        if device_batches:
            m.build_input_batch()
            assert all(len(p) == 5 for p in m._patches)
            codes |= {p[4] for p in m._patches}
        else:
            for i in range(m.batch_num):
                m.batch_input[i], m.batch_input_bicubic[i], m.batch_true[i] = m.train.load_batch_image(m.max_value)
        m.train_batch()
        if device_batches:
            assert 1 <= len(m._device_images) <= 14, len(m._device_images)      # one upload per base file
        losses.append(m.training_loss_sum)
    tensors = m._training_tensors()
    m.close()
    return losses, tensors, codes


def test_model_at_level_8_on_device_batches_equals_host_batches(oracle, tmp_path):
    cfg = oracle.make_config(**CONFIGS["L7_F32to8_x2"])
    weights = oracle.synthetic_weights(cfg, seed=0)
    dev_losses, dev, codes = _train(tmp_path / "dev", weights, True)
    host_losses, host, _ = _train(tmp_path / "host", weights, False)
    assert codes == set(range(8))                                # 120 draws of 112 entries
    assert dev_losses == host_losses
    assert set(dev) == set(host) and len(dev) == 3 * len(weights) + 2
    for k in dev:
        assert np.array_equal(np.asarray(dev[k]).view(np.uint32), np.asarray(host[k]).view(np.uint32)), k
