"""Training of the transposed-conv nets on the GPU (option "train_transposed" of include/dcscn.h) against the float64 restatement of
tests/train_ref_transposed.py; the bars are the f32 path's (tests/test_train_hip.py, tests/test_train_separable_hip.py)."""
import os
import random

import numpy as np
import pytest
import torch

from conftest import CONFIGS, GOLDEN
from test_host import _flags
import train_ref as R
import train_ref_transposed as T

pytestmark = pytest.mark.gpu

FLAGS = dict(optimizer="adam", beta1=0.9, beta2=0.999, epsilon=1e-8, momentum=0.9, l2_decay=1e-4, clipping_norm=5.0,
             dropout_rate=1.0, use_l1_loss=False)
TW = "Up-TCNN/Tconv_W"


def _engine(cfg, weights, options=(), **flags):
    from dcscn_amd import engine
    eng = engine.Engine(cfg, device=0)
    eng.load_weights(weights)
    eng.set_option("train_transposed", 1)
    if cfg["depthwise_separable"]:
        eng.set_option("train_separable", 1)
    for key in options:
        eng.set_option(key, 1)
    eng.train_begin(dict(FLAGS, **flags))
    return eng


def _gradients(case, options=()):
    """(stats, {name: gradient}) of the library on a case of train_ref_transposed, at its L2_DECAY and KEY."""
    cfg, weights, x, x2, y = T.case_inputs(case)
    with _engine(cfg, weights, options, use_l1_loss=case[6], dropout_rate=case[5], l2_decay=T.L2_DECAY) as eng:
        stats = eng.train_gradients(x, x2, y, dropout_key=T.KEY)
        return stats, {name: eng.get_tensor(name + "/grad") for name in weights}


def _check(case, options=()):
    stats, got = _gradients(case, options)
    ref, g64 = T.reference(case)
    print("%r: stats %r, reference %r" % (case, stats, ref))
    worst = []
    for name, g in g64.items():
        err, top = float(np.max(np.abs(got[name].astype(np.float64) - g))), float(np.max(np.abs(g)))
        print("  %-40s max err %.3g  bound %.3g" % (name, err, 1e-4 * top))
        if err > 1e-4 * top:
            worst.append((name, err, 1e-4 * top))
    assert abs(stats[0] - ref["image_loss"]) <= 1e-6 * abs(ref["image_loss"]), (stats, ref)
    assert abs(stats[3] - ref["loss"]) <= 1e-6 * abs(ref["loss"]), (stats, ref)
    _, norm = R.clip_factor(g64, 0.0)
    assert abs(stats[2] - norm) <= 1e-4 * norm, (stats[2], norm)
    assert not worst, worst


@pytest.mark.parametrize("case", T.MAIN_CASES, ids=T.case_id)
def test_gradients_match_float64_autograd(case):
    _check(case)


@pytest.mark.parametrize("case", T.EDGE_CASES, ids=T.case_id)
def test_gradients_on_edge_shapes(case):
    _check(case)


def test_gradients_under_split16():
    """t4: its feature layers are eligible for the split16 kernels, Up-TCNN stays on f32; the bars do not move."""
    _check(T.MAIN_CASES[2], options=("train_split16", "train_split16_wgrad"))


@pytest.mark.parametrize("opt", ["adam", "momentum", "gd"])
def test_one_optimizer_step_matches_tf_update_rules(oracle, opt):
    cfg = T.net("t2")
    weights = oracle.synthetic_weights(cfg, seed=2)
    x, x2, y = T.batch(cfg, 2, 12, 16, 5)
    lr, clipping_norm = 1e-3, 0.01
    with _engine(cfg, weights, optimizer=opt, clipping_norm=clipping_norm) as eng:
        eng.train_gradients(x, x2, y)
        g = {k: eng.get_tensor(k + "/grad").astype(np.float64) for k in weights}
        eng.train_step(x, x2, y, lr)
        w1 = {k: eng.get_tensor(k) for k in weights}
        slots = {}
        for k in weights:
            if opt == "adam":
                slots[k] = (eng.get_tensor(k + "/Adam"), eng.get_tensor(k + "/Adam_1"))
            elif opt == "momentum":
                slots[k] = (eng.get_tensor(k + "/Momentum"),)
        if opt == "adam":
            b1p, b2p = float(eng.get_tensor("beta1_power")), float(eng.get_tensor("beta2_power"))
            assert b1p == float(np.float32(0.9) * np.float32(0.9)) and b2p == float(np.float32(0.999) * np.float32(0.999))
    clip, norm = R.clip_factor(g, clipping_norm)
    assert norm > clipping_norm                                     # the clip is exercised
    f32 = lambda v: float(np.float32(v))                           # TF holds the hyperparameters as float32 constants
    b1, b2, lr = f32(0.9), f32(0.999), f32(lr)
    assert TW in weights and weights[TW].shape == (4, 4, 14, 14)
    for k, w in weights.items():
        gg = g[k] * clip
        w0 = w.astype(np.float64)
        if opt == "adam":
            want, m, v = R.adam(w0, gg, 0.0, 0.0, b1, b2, lr, b1=b1, b2=b2, eps=f32(1e-8))
            np.testing.assert_allclose(slots[k][0], m, rtol=1e-6, atol=1e-6 * np.max(np.abs(m)))
            np.testing.assert_allclose(slots[k][1], v, rtol=1e-6, atol=1e-6 * np.max(np.abs(v)))
        elif opt == "momentum":
            want, a = R.momentum(w0, gg, 0.0, lr, f32(0.9))
            np.testing.assert_allclose(slots[k][0], a, rtol=1e-6, atol=1e-6 * np.max(np.abs(a)))
        else:
            want = R.gd(w0, gg, lr)
        np.testing.assert_allclose(w1[k], want, rtol=1e-6, atol=1e-6 * np.max(np.abs(want)))
    assert not np.array_equal(w1[TW], weights[TW])


def _state(eng, names):
    out = {k: eng.get_tensor(k) for k in names}
    for k in names:
        out[k + "/Adam"] = eng.get_tensor(k + "/Adam")
        out[k + "/Adam_1"] = eng.get_tensor(k + "/Adam_1")
    out["beta1_power"] = eng.get_tensor("beta1_power")
    out["beta2_power"] = eng.get_tensor("beta2_power")
    return out


def _assert_same_bits(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]).view(np.uint32), np.asarray(b[k]).view(np.uint32)), k


def test_two_runs_of_five_steps_with_dropout_are_bit_identical(oracle):
    cfg = T.net("t2r")
    weights = oracle.synthetic_weights(cfg, seed=0)
    batches = [T.batch(cfg, 2, 12, 16, s) for s in range(2)]
    states = []
    for _ in range(2):
        with _engine(cfg, weights, dropout_rate=0.8) as eng:
            for i in range(5):
                eng.train_step(*batches[i % 2], 1e-3, dropout_key=1000 + i)
            states.append(_state(eng, weights))
    _assert_same_bits(states[0], states[1])
    assert not np.array_equal(states[0][TW], weights[TW])


def test_world_of_one_reproduces_train_step_bit_for_bit(oracle):
    """3 clipped adam steps with dropout: train_step on one handle, local_gradients + apply_records(world = 1) on another."""
    cfg = T.net("t2r")
    weights = oracle.synthetic_weights(cfg, seed=0)
    batches = [T.batch(cfg, 2, 12, 16, s) for s in (1, 2, 3)]
    flags = dict(dropout_rate=0.8, clipping_norm=0.01)
    with _engine(cfg, weights, **flags) as one, _engine(cfg, weights, **flags) as rank:
        stream = torch.cuda.Stream()
        record = torch.zeros(rank.train_record_floats(), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for i, batch in enumerate(batches):
            want = one.train_step(*batch, 1e-3, dropout_key=T.KEY + i)
            x, x2, y = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in batch)
            torch.cuda.synchronize()
            rank.train_local_gradients_device(x.data_ptr(), x2.data_ptr(), y.data_ptr(), 2, 12, 16, record.data_ptr(), dropout_key=T.KEY + i,
                                              first_index=0, stream=stream.cuda_stream)
            got = rank.train_apply_records(record.data_ptr(), 1, 1e-3, stream=stream.cuda_stream)
            assert want[2] > 0.01                                             # the clip factor is < 1
            assert np.array_equal(np.array(want).view(np.uint64), np.array(got).view(np.uint64)), (want, got)
            _assert_same_bits(_state(one, weights), _state(rank, weights))


def test_the_gate(oracle):
    from dcscn_amd import engine
    cfg = T.net("t2")
    weights = oracle.synthetic_weights(cfg, seed=0)
    with engine.Engine(cfg, device=0) as eng:
        eng.load_weights(weights)
        with pytest.raises(engine.EngineError) as e:
            eng.train_begin(FLAGS)
        assert e.value.status == 2 and "transposed" in e.value.message
        eng.set_option("train_transposed", 1)                       # the same handle, once the option is set
        eng.train_begin(FLAGS)
        assert eng.get_tensor(TW + "/grad").shape == (4, 4, 14, 14)
    # separable and transposed: both options, and the refusal names the one that is missing
    cfg = T.net("tds")
    weights = oracle.synthetic_weights(cfg, seed=0)
    for have, missing in (("train_transposed", "separable"), ("train_separable", "transposed")):
        with engine.Engine(cfg, device=0) as eng:
            eng.load_weights(weights)
            eng.set_option(have, 1)
            with pytest.raises(engine.EngineError) as e:
                eng.train_begin(FLAGS)
            assert e.value.status == 2 and missing in e.value.message, (have, e.value.message)


def test_the_option_changes_no_bit_of_a_pixel_shuffler_net(oracle):
    from dcscn_amd import engine
    cfg = oracle.make_config(**CONFIGS["L7_F32to8_x2"])
    weights = oracle.synthetic_weights(cfg, seed=0)
    x, x2, y = T.batch(cfg, 2, 12, 16, 1)
    runs = []
    for option in (0, 1):
        with engine.Engine(cfg, device=0) as eng:
            eng.load_weights(weights)
            eng.set_option("train_transposed", option)
            eng.train_begin(dict(FLAGS, dropout_rate=0.8, l2_decay=T.L2_DECAY))
            stats = eng.train_gradients(x, x2, y, dropout_key=T.KEY)
            runs.append((stats, {name: eng.get_tensor(name + "/grad") for name in weights}))
    _assert_same_bits(runs[0][1], runs[1][1])
    assert np.array_equal(np.array(runs[0][0]).view(np.uint64), np.array(runs[1][0]).view(np.uint64))


def test_a_short_run_learns_and_the_forward_uses_the_trained_weights(oracle):
    from dcscn_amd import engine
    cfg = T.net("t2")
    weights = oracle.synthetic_weights(cfg, seed=0)
    batches = [T.batch(cfg, 2, 12, 16, s) for s in (1, 2)]
    x, x2, _ = batches[0]
    with engine.Engine(cfg, device=0) as fresh:
        fresh.load_weights(weights)
        before = fresh.forward(x, x2)
    with _engine(cfg, weights) as eng:
        assert np.array_equal(eng.forward(x, x2), before)          # train_begin alone changes nothing
        losses = [eng.train_step(*batches[i % 2], 1e-3, dropout_key=i)[0] for i in range(60)]
        trained = {k: eng.get_tensor(k) for k in weights}
        after = eng.forward(x, x2)
    first, last = float(np.mean(losses[:10])), float(np.mean(losses[-10:]))
    print("mean image loss: first 10 steps %.4f, last 10 steps %.4f" % (first, last))
    assert last < first
    assert not np.array_equal(after, before) and not np.array_equal(trained[TW], weights[TW])
    ref = oracle.forward(cfg, trained, x, x2, dtype=np.float64)
    assert float(np.max(np.abs(after - ref))) <= 1e-4              # the derived inference filter was rebuilt from the trained Tconv_W


# ---- the driver: SuperResolution with pixel_shuffler = False, in the manner of tests/test_train_separable_hip.py ----------------------

TC = dict(T.NETS["t2"], pixel_shuffler=False, self_ensemble=1)


def _batches(count, n=4, size=12):
    from helper import loader
    d = loader.DynamicDataSets(2, size)
    d.set_data_dir(os.path.join(GOLDEN, "set14"))
    random.seed(0)
    d.init_batch_index()
    return [[d.load_batch_image(255.0) for _ in range(n)] for _ in range(count)]


def _model(ck, weights=None):
    from dcscn_amd.model import SuperResolution
    m = SuperResolution(_flags(checkpoint_dir=ck, batch_num=4, **TC))
    m.build_graph()
    m.build_optimizer()
    if weights is not None:
        m.load_weights(weights)
    m.init_train_step()
    return m


def _steps(m, batches, start, count):
    for i in range(start, start + count):
        m.batch_input, m.batch_input_bicubic, m.batch_true = (list(t) for t in zip(*batches[i]))
        m.train_batch()


def test_the_model_class_trains_saves_reloads_evaluates_and_resumes(oracle, tmp_path):
    from dcscn_amd import ckpt
    cfg = T.net("t2")
    weights = oracle.synthetic_weights(cfg, seed=0)
    batches = _batches(6)
    a = _model(str(tmp_path / "a"), weights)
    _steps(a, batches, 0, 6)
    a.save_model(name="straight")
    a.close()
    b = _model(str(tmp_path / "b"), weights)
    _steps(b, batches, 0, 3)
    assert np.isfinite(b.training_loss_sum) and b.training_step == 3
    b.save_model(name="half")
    b.close()
    half = ckpt.load_checkpoint(str(tmp_path / "b" / "half.ckpt"), include_optimizer_slots=True)
    for k, v in weights.items():
        assert half[k + "/Adam"].shape == v.shape and half[k + "/Adam_1"].shape == v.shape
    assert TW + "/Adam" in half and TW + "/Adam_1" in half and np.any(half[TW + "/Adam"] != 0)
    assert not np.array_equal(half[TW], weights[TW])
    assert float(half["beta1_power"]) == float(np.float32(0.9) ** 4)
    # a model that only evaluates loads the trained variables
    from dcscn_amd.model import SuperResolution
    ev = SuperResolution(_flags(checkpoint_dir=str(tmp_path / "b"), **TC))
    ev.build_graph()
    ev.load_model(name="half")
    psnr, ssim = ev.do_for_evaluate(os.path.join(GOLDEN, "set5", sorted(os.listdir(os.path.join(GOLDEN, "set5")))[0]))
    ev.close()
    assert np.isfinite(psnr) and psnr > 0.0 and np.isfinite(ssim)
    # resumed with the slots restored: the straight run's bits
    c = _model(str(tmp_path / "b"))
    c.load_model(name="half")
    c.step = 3                                              # the resumed run is given its step: same dropout masks
    _steps(c, batches, 3, 3)
    c.save_model(name="resumed")
    c.close()
    want = ckpt.load_checkpoint(str(tmp_path / "a" / "straight.ckpt"), include_optimizer_slots=True)
    got = ckpt.load_checkpoint(str(tmp_path / "b" / "resumed.ckpt"), include_optimizer_slots=True)
    assert set(want) == set(got) and len(want) == 3 * len(weights) + 2
    for k in want:
        assert np.array_equal(np.asarray(want[k]).view(np.uint32), np.asarray(got[k]).view(np.uint32)), k


def test_a_fresh_model_starts_tconv_w_from_the_bilinear_filter(tmp_path):
    from dcscn_amd.model import transposed_conv_initial
    m = _model(str(tmp_path / "fresh"))
    m.init_all_variables()
    start = m._pending_init[TW].copy()                      # what the first train_batch loads, before the step moves it
    assert start.shape == (4, 4, 14, 14) and np.array_equal(start, transposed_conv_initial(2, 14))
    assert start[1, 2, 3, 3] == np.float32(0.75 * 0.75) and start[0, 3, 5, 5] == np.float32(0.25 * 0.25) and not np.any(start[:, :, 3, 5])
    _steps(m, _batches(1), 0, 1)
    assert np.isfinite(m.training_loss_sum) and m.training_step == 1
    now = m._engine.get_tensor(TW)
    m.close()
    assert now.shape == start.shape and np.all(np.isfinite(now)) and not np.array_equal(now, start)
    assert float(np.max(np.abs(now - start))) < 0.1         # one adam step from the bilinear value, not from somewhere else
