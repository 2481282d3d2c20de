"""adadelta, adagrad and rmsprop on the GPU (option "train_optimizers" of include/dcscn.h; kernel topt_more) against the numpy float64
restatement of tests/train_ref_optimizers.py, which extends tests/train_ref.py by the three rules.  The rules and their constants are
written from knowledge of TF 1.x; nothing here has been run against TensorFlow.

The net is the three-layer one of tests/test_train_hip.py::test_refusals at x2, batches of 2 patches of 16 x 16."""
import functools
import os
import random

import numpy as np
import pytest
import torch

from conftest import CONFIGS, GOLDEN
from test_host import _flags
from test_train_hip import FLAGS, _batch
from test_train_surface_hip import _close
import train_ref as R
import train_ref_optimizers as P

pytestmark = pytest.mark.gpu

L3 = dict(layers=3, filters=8, min_filters=4, nin_filters=4, nin_filters2=4)
L3_T = dict(L3, pixel_shuffler=False)
DS = CONFIGS["L7_F32to8_x4_DS"]
LR = {"adagrad": 0.01, "adadelta": 1.0, "rmsprop": 0.001}       # adadelta's unit-free step is about sqrt(1e-8 / 0.05) = 4.5e-4 at first
MU = 0.9
UNSUPPORTED, SHAPE_ERROR = 2, 4


@functools.lru_cache(maxsize=None)
def _net(key="L3"):
    import dcscn_oracle
    cfg = dcscn_oracle.make_config(**{"L3": L3, "L3_T": L3_T, "DS": DS}[key])
    weights = dcscn_oracle.synthetic_weights(cfg, seed=0)
    if key == "L3":
        weights["CNN1/conv_B"] = np.zeros_like(weights["CNN1/conv_B"])      # variables that are exactly 0: the bar is then the update's alone
    for v in weights.values():
        v.setflags(write=False)
    return cfg, weights


def _engine(key="L3", option=True, options=(), **flags):
    from dcscn_amd import engine
    cfg, weights = _net(key)
    eng = engine.Engine(cfg, device=0)
    eng.load_weights(weights)
    for o in options:
        eng.set_option(o, 1)
    if option:
        eng.set_option("train_optimizers", 1)
    try:
        eng.train_begin(dict(FLAGS, **flags))
    except Exception:
        eng.close()
        raise
    return eng


def _names(eng):
    return [name for name, _ in eng.tensor_specs()]


def _flat(eng, suffix=""):
    """Every "<var><suffix>" in dcscn_tensor_info order as one flat float32 vector: the layout of a record and of the slots."""
    return np.concatenate([eng.get_tensor(name + suffix).ravel() for name in _names(eng)])


def _state(eng, opt):
    """{name: array} of the variables and the running optimizer's slots (and adam's powers)."""
    suffixes = dict({"adam": ("/Adam", "/Adam_1"), "momentum": ("/Momentum",), "gd": ()},
                    **{o: tuple(s for s in P.SLOTS[o] if s) for o in P.OPTIMIZERS})[opt]
    out = {n + s: eng.get_tensor(n + s) for n in _names(eng) for s in ("",) + suffixes}
    if opt == "adam":
        out.update(beta1_power=eng.get_tensor("beta1_power"), beta2_power=eng.get_tensor("beta2_power"))
    return out


def _same_bits(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        assert np.array_equal(np.asarray(a[k]).view(np.uint32), np.asarray(b[k]).view(np.uint32)), (what, k)


# ---------------------------------------------------------------------------------------------
# 1. the rule as arithmetic: planted gradient records through train_apply_records at world = 1
# ---------------------------------------------------------------------------------------------
def _records(count, scale, zeros_at):
    """Three records of a world of 1.  The magnitudes differ from step to step, N(0, 1) * 10^U(-4, 1) * scale; the signs are one
    pattern for all three, so the cumulative update of an element is the sum of its steps' magnitudes and no element's update
    cancels; planted in every record: exact zeros (+0 and -0) and values of +-1e-15 (their squares, 1e-30, are still normal
    float32 numbers: a relative bar means nothing below the smallest normal), anywhere and on the eight variables from ``zeros_at``
    on, which are exactly 0."""
    rng = np.random.default_rng(22)
    sign = np.where(rng.random(count) < 0.5, -1.0, 1.0)
    planted = np.sort(rng.choice(count, 16, replace=False))
    recs = []
    for step in range(3):
        g = (np.abs(rng.standard_normal(count)) * 10.0 ** rng.uniform(-4.0, 1.0, count) * scale * sign).astype(np.float32)
        g[planted[0:3]] = 0.0
        g[planted[3:5]] = -0.0
        g[planted[5:8]] = np.float32(1e-15)
        g[planted[8:11]] = np.float32(-1e-15)
        g[zeros_at:zeros_at + 8] = np.float32([0.0, 1e-15, -1e-15, 0.5, -0.5, 3.0, -0.0, 1e-3]) * np.float32(1 + step)
        rec = np.zeros((1, R.record_pad(count) + R.RECORD_TRAILER_FLOATS), np.float32)
        rec[0, :count] = g
        rec[0, R.record_pad(count):] = np.array([2.5, 2.5, 2.0, 2.75]).view(np.float32)     # image_loss, mse, n_local, total loss
        recs.append(rec)
    return recs


def _bar(value, terms):
    return 16.0 * 2.0 ** -24 * (np.abs(value) + terms)


@pytest.mark.parametrize("clipped", [True, False], ids=["clip_below_1", "clip_is_1"])
@pytest.mark.parametrize("opt", P.OPTIMIZERS)
def test_the_rule_is_the_stated_arithmetic(opt, clipped):
    """Three steps from TF's initial slots against the float64 rule applied to g * clip (g and the float32 clip factor restated bit for
    bit by train_ref.reduce_records).  Bar per element of w: 16 * 2^-24 * (|w| + |D|), D the restatement's cumulative update w_3 - w_0:
    a rule is at most ten float32 roundings of at most 2^-24 relative each, on an update of size |D| and a subtraction from w, and the
    factor leaves room for three steps.  The slots take the same 16 * 2^-24 relative to their own value: every one of them is a sum of
    terms of one sign here (rmsprop's mom too, the records keeping each element's sign), so nothing cancels in them."""
    cfg, weights = _net()
    lr, mu = P.f32(LR[opt]), P.f32(MU)
    clipping_norm = 5.0 if clipped else 1e9
    with _engine(optimizer=opt, clipping_norm=clipping_norm, momentum=MU) as eng:
        names = _names(eng)
        count = sum(weights[n].size for n in names)
        zeros_at = sum(weights[n].size for n in names[:names.index("CNN1/conv_B")])
        assert weights["CNN1/conv_B"].size == 8
        m_suffix, v_suffix = P.SLOTS[opt]
        m0, v0 = P.INITIAL[opt]
        for n in names:                                               # TF's initial slots, before the first step
            assert np.all(eng.get_tensor(n + m_suffix) == np.float32(m0)), n
            if v_suffix:
                assert np.all(eng.get_tensor(n + v_suffix) == np.float32(v0)), n
        w_start = _flat(eng).astype(np.float64)
        assert np.count_nonzero(w_start == 0.0) >= 8
        w, m, v = w_start, np.full(count, P.f32(m0)), np.zeros(count)
        assert not np.any(w_start[zeros_at:zeros_at + 8])
        for step, rec in enumerate(_records(count, 1.0 if clipped else 1e-2, zeros_at)):
            g, stats, clip = R.reduce_records(rec, count, clipping_norm)
            assert np.array_equal(g.view(np.uint32), rec[0, :count].view(np.uint32))          # world = 1: the record's own floats
            assert (clip < 1.0 and stats[2] > 5.0) if clipped else clip == 1.0, (step, clip, stats[2])
            dev = torch.from_numpy(rec).cuda()
            torch.cuda.synchronize()
            got = eng.train_apply_records(dev.data_ptr(), 1, LR[opt])
            assert np.float32(got[2]) == stats[2]
            assert np.array_equal(_flat(eng, "/grad").view(np.uint32), g.view(np.uint32))
            w, m, v = P.step(opt, w, g.astype(np.float64) * np.float64(clip), m, v, lr, mu)
        checks = [("w", _flat(eng), w, _bar(w, np.abs(w - w_start))), ("slot" + m_suffix, _flat(eng, m_suffix), m, _bar(m, 0.0))]
        if v_suffix:
            checks.append(("slot" + v_suffix, _flat(eng, v_suffix), v, _bar(v, 0.0)))
        failed = []
        for what, have, want, bar in checks:
            err = np.abs(have.astype(np.float64) - want)
            ratio = np.where(err == 0.0, 0.0, err / np.maximum(bar, 1e-300))
            worst = int(np.argmax(ratio))
            print("%s %s %s: worst error / bar = %.3f at %d (got %r, restated %r)" % (
                opt, "clipped" if clipped else "unclipped", what, ratio[worst], worst, have[worst], want[worst]))
            if ratio[worst] > 1.0:
                failed.append((what, float(ratio[worst]), worst))
        assert np.count_nonzero(w != w_start) > count // 2 and np.all(np.isfinite(w))
        assert not failed, failed


# ---------------------------------------------------------------------------------------------
# 2. / 5. full steps, every update from the state the device really has
# ---------------------------------------------------------------------------------------------
def _check_steps(eng, opt, batches, steps, lr, clipping_norm):
    """tests/test_train_surface_hip.py's comparison: before every step the variables and the slots are read from the device, the
    float64 rule is applied to them with the device's own gradient (train_gradients, same batch and key) times the restated clip
    factor, and the step's result is held to the bar that file and tests/test_train_hip.py use (rtol 1e-6, atol 1e-6 * max)."""
    names = _names(eng)
    m_suffix, v_suffix = P.SLOTS[opt]
    lr32, mu = P.f32(lr), P.f32(MU)
    for step in range(steps):
        x, x2, y = batches[step % len(batches)]
        before = _state(eng, opt)
        eng.train_gradients(x, x2, y, dropout_key=500 + step)
        g = {k: eng.get_tensor(k + "/grad").astype(np.float64) for k in names}
        eng.train_step(x, x2, y, lr, dropout_key=500 + step)
        after = _state(eng, opt)
        clip, norm = R.clip_factor(g, clipping_norm)
        if step == 0:
            assert norm > clipping_norm                               # the clip is exercised
        for k in names:
            what = "%s step %d %s" % (opt, step, k)
            m = before[k + m_suffix].astype(np.float64)
            v = before[k + v_suffix].astype(np.float64) if v_suffix else None
            if step > 0:
                assert np.any(m != P.INITIAL[opt][0]) and (v is None or np.any(v)), what
            w, m, v = P.step(opt, before[k].astype(np.float64), g[k] * clip, m, v, lr32, mu)
            _close(after[k + m_suffix], m, what + m_suffix)
            if v_suffix:
                _close(after[k + v_suffix], v, what + v_suffix)
            _close(after[k], w, what)
        assert sum(not np.array_equal(after[k], before[k]) for k in names) > len(names) // 2, (opt, step)


@pytest.mark.parametrize("opt", P.OPTIMIZERS)
def test_three_full_steps_match_the_rules_from_the_device_state(opt):
    cfg, _ = _net()
    batches = [_batch(cfg, 2, 16, 16, s) for s in (5, 6)]
    with _engine(optimizer=opt, clipping_norm=5.0, dropout_rate=0.8, momentum=MU) as eng:
        _check_steps(eng, opt, batches, 3, LR[opt], 5.0)


@pytest.mark.parametrize("key,option,hw", [("DS", "train_separable", 12), ("L3_T", "train_transposed", 16)])
def test_rmsprop_steps_the_other_topologies(key, option, hw):
    """One rmsprop step of the separable x4 net and of the three-layer transposed-conv net: every variable kind of both
    (depthwise_W, pointwise_W, Tconv_W) goes through the same flat buffers."""
    cfg, weights = _net(key)
    assert any(k.endswith(("/depthwise_W", "/Tconv_W")) for k in weights)
    batches = [_batch(cfg, 2, hw, hw, 5)]
    clipping_norm = 0.01                                              # the separable x4 net's gradient is small
    with _engine(key, options=(option,), optimizer="rmsprop", clipping_norm=clipping_norm, momentum=MU) as eng:
        _check_steps(eng, "rmsprop", batches, 1, LR["rmsprop"], clipping_norm)


# ---------------------------------------------------------------------------------------------
# 3. determinism, and resume through the model class
# ---------------------------------------------------------------------------------------------
def _batches(count, n=2, size=16):
    from helper import loader
    d = loader.DynamicDataSets(2, size)
    d.set_data_dir(os.path.join(GOLDEN, "set14"))
    random.seed(0)
    d.init_batch_index()
    return [[d.load_batch_image(255.0) for _ in range(n)] for _ in range(count)]


def _model(ck, opt, weights=None):
    from dcscn_amd.model import SuperResolution
    m = SuperResolution(_flags(checkpoint_dir=ck, batch_num=2, optimizer=opt, self_ensemble=1, **L3))
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


@pytest.mark.parametrize("opt", P.OPTIMIZERS)
def test_two_runs_agree_and_a_saved_run_resumes_to_the_same_bits(opt, tmp_path):
    """train_batch sets the option by itself; two runs of three steps have one digest; a run saved after step 2 with save_model and
    loaded into a fresh model ends step 3 on the uninterrupted run's bits, variables and slots."""
    from dcscn_amd import ckpt
    weights = dict(_net()[1])
    batches = _batches(3)
    digests = []
    for run in ("a", "a2"):
        m = _model(str(tmp_path / run), opt, weights)
        _steps(m, batches, 0, 3)
        digests.append(m.training_digest())
        m.save_model(name="straight")
        m.close()
    assert digests[0] == digests[1]
    b = _model(str(tmp_path / "b"), opt, weights)
    _steps(b, batches, 0, 2)
    b.save_model(name="two")
    b.close()
    two = ckpt.load_checkpoint(str(tmp_path / "b" / "two.ckpt"), include_optimizer_slots=True)
    slots = [s[1:] for s in P.SLOTS[opt] if s]
    assert set(two) == set(weights) | {k + "/" + s for k in weights for s in slots}
    assert "beta1_power" not in two and "beta2_power" not in two
    for k in weights:
        assert all(two[k + "/" + s].shape == weights[k].shape for s in slots)
    # (not every variable's: 0.1 + g^2 is 0.1 in float32 for the clipped gradient of a small bias)
    assert sum(bool(np.any(two[k + "/" + slots[0]] != np.float32(P.INITIAL[opt][0]))) for k in weights) > len(weights) // 2
    c = _model(str(tmp_path / "b"), opt)
    c.load_model(name="two")
    c.step = 2                                                       # the resumed run is given its step: same dropout masks
    _steps(c, batches, 2, 1)
    assert c.training_digest() == digests[0]
    c.save_model(name="resumed")
    c.close()
    want = ckpt.load_checkpoint(str(tmp_path / "a" / "straight.ckpt"), include_optimizer_slots=True)
    got = ckpt.load_checkpoint(str(tmp_path / "b" / "resumed.ckpt"), include_optimizer_slots=True)
    _same_bits(want, got, opt)
    assert any(not np.array_equal(want[k], two[k]) for k in weights)                      # the third step moved something
    # a model that only evaluates loads the variables and ignores the slots
    from dcscn_amd.model import SuperResolution
    ev = SuperResolution(_flags(checkpoint_dir=str(tmp_path / "b"), self_ensemble=1, **L3))
    ev.build_graph()
    ev.load_model(name="two")
    assert set(ev._weights) == set(weights)
    ev.close()


# ---------------------------------------------------------------------------------------------
# 4. nothing else moved
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", ["adam", "momentum", "gd"])
def test_the_option_leaves_adam_momentum_and_gd_their_bits(opt):
    cfg, _ = _net()
    batches = [_batch(cfg, 2, 16, 16, s) for s in (5, 6)]
    states = []
    for option in (False, True):
        with _engine(option=option, optimizer=opt, dropout_rate=0.8) as eng:
            for step in range(3):
                eng.train_step(*batches[step % 2], 1e-3, dropout_key=500 + step)
            states.append(_state(eng, opt))
    _same_bits(states[0], states[1], opt)
    assert any(not np.array_equal(states[0][k], v) for k, v in _net()[1].items())


def test_refusals_without_the_option_and_of_foreign_slots():
    from dcscn_amd import engine
    for opt in P.OPTIMIZERS:
        with pytest.raises(engine.EngineError) as e:
            _engine(option=False, optimizer=opt)
        assert e.value.status == UNSUPPORTED
        assert e.value.message == "optimizer %s is not implemented (supported: adam, gd, momentum)" % opt, e.value.message
    with _engine(optimizer="rmsprop") as eng:
        for foreign in ("CNN1/conv_W/Adam", "CNN1/conv_W/Adam_1", "CNN1/conv_W/Momentum", "CNN1/conv_W/Adagrad", "CNN1/conv_W/Adadelta_1",
                        "beta1_power"):
            with pytest.raises(engine.EngineError) as e:
                eng.get_tensor(foreign)
            assert e.value.status == SHAPE_ERROR, foreign
        with pytest.raises(engine.EngineError) as e:
            eng.set_train_tensor("CNN1/conv_W/Adam", np.zeros((3, 3, 1, 8), np.float32))
        assert e.value.status == SHAPE_ERROR
        assert eng.get_tensor("CNN1/conv_W/RMSProp").shape == (3, 3, 1, 8)
    with _engine(optimizer="adam") as eng:                             # and the new names are foreign to adam, option or not
        with pytest.raises(engine.EngineError) as e:
            eng.get_tensor("CNN1/conv_W/RMSProp")
        assert e.value.status == SHAPE_ERROR
