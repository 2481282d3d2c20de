"""Training on the GPU (dcscn_train_* of include/dcscn.h) against the float64 restatement of tests/train_ref.py."""
import json
import os
import tempfile

import numpy as np
import pytest
import torch

from conftest import CONFIGS, GOLDEN, synthetic_batch
import train_ref as R

pytestmark = pytest.mark.gpu

K5 = dict(layers=4, filters=16, min_filters=8, cnn_size=5, activator="relu", reconstruct_layers=2, reconstruct_filters=6,
          use_nin=False, scale=2)
L12_X4 = CONFIGS["L12_F196to48_x4"]
FLAGS = dict(optimizer="adam", beta1=0.9, beta2=0.999, epsilon=1e-8, momentum=0.9, l2_decay=1e-4, clipping_norm=5.0,
             dropout_rate=1.0, use_l1_loss=False)


def _batch(cfg, n, h, w, seed):
    x, x2 = synthetic_batch(n, h, w, cfg["scale"], seed=seed)
    rng = np.random.default_rng(seed + 100)
    y = (x2 + rng.normal(0, 8, x2.shape)).astype(np.float32)      # a target the net does not already produce
    return x, x2, y


def _engine(cfg, weights, **flags):
    from dcscn_amd import engine
    eng = engine.Engine(cfg, device=0)
    eng.load_weights(weights)
    f = dict(FLAGS)
    f.update(flags)
    eng.train_begin(f)
    return eng


def _check_grads(oracle, over, n, h, w, l1=False, keep=1.0, key=0, tol=1e-4, seed=0):
    cfg = oracle.make_config(**over)
    weights = oracle.synthetic_weights(cfg, seed=seed)
    x, x2, y = _batch(cfg, n, h, w, seed + 1)
    with _engine(cfg, weights, use_l1_loss=l1, dropout_rate=keep, l2_decay=1e-3) as eng:
        stats = eng.train_gradients(x, x2, y, dropout_key=key)
        got = {name: eng.get_tensor(name + "/grad") for name in weights}
    ref, g64 = R.loss_and_grads(cfg, weights, x, x2, y, keep=keep, key=key, l1=l1, l2_decay=1e-3)
    assert abs(stats[0] - ref["image_loss"]) <= 1e-6 * abs(ref["image_loss"]), (stats, ref)
    assert abs(stats[3] - ref["loss"]) <= 1e-6 * abs(ref["loss"]), (stats, ref)
    _, norm = R.clip_factor(g64, 0.0)
    assert abs(stats[2] - norm) <= 1e-4 * norm, (stats[2], norm)
    bad = []
    for name, g in g64.items():
        err = float(np.max(np.abs(got[name].astype(np.float64) - g)))
        if err > tol * float(np.max(np.abs(g))):
            bad.append((name, err, float(np.max(np.abs(g)))))
    if bad:
        _, g32 = R.loss_and_grads(cfg, {k: v.astype(np.float32) for k, v in weights.items()}, x, x2, y, keep=keep, key=key, l1=l1,
                                  l2_decay=1e-3, dtype=torch.float32)
        msg = ["%s: max err %.3g (bound %.3g); float32 torch err %.3g" % (nm, e, tol * m, float(np.max(np.abs(g32[nm] - g64[nm]))))
               for nm, e, m in bad]
        pytest.fail("\n".join(msg))
    return stats


@pytest.mark.parametrize("name,over,n,hw", [
    ("L7_x2", CONFIGS["L7_F32to8_x2"], 3, 24), ("L7_x3", CONFIGS["L7_F32to8_x3"], 2, 28), ("L7_x4", CONFIGS["L7_F32to8_x4"], 2, 24),
    ("L2_legacy", CONFIGS["L2_F4to4_x2"], 4, 32), ("L8_x2", CONFIGS["L8_F96to48_x2"], 2, 24), ("L12_x4", L12_X4, 2, 24),
    ("k5_relu_r2_nonin", K5, 3, 26)])
def test_gradients_match_float64_autograd(oracle, name, over, n, hw):
    _check_grads(oracle, over, n, hw, hw + 4)


@pytest.mark.parametrize("over", [CONFIGS["L7_F32to8_x2"], K5])
def test_gradients_match_float64_autograd_l1(oracle, over):
    _check_grads(oracle, over, 3, 24, 24, l1=True)


def test_gradients_full_size_batch(oracle):
    _check_grads(oracle, CONFIGS["L7_F32to8_x2"], 20, 48, 48, tol=5e-4)


def test_dropout_gradients_match_the_restated_masks(oracle):
    cfg = oracle.make_config(**CONFIGS["L7_F32to8_x2"])
    _check_grads(oracle, CONFIGS["L7_F32to8_x2"], 3, 24, 24, keep=0.8, key=0x1234567)
    for layer, c in enumerate(oracle.filter_schedule(cfg["layers"], cfg["filters"], cfg["min_filters"], cfg["filters_decay_gamma"])):
        frac = R.dropout_mask(0x1234567, layer, (3, 24, 24, c), 0.8).mean()
        assert abs(frac - 0.8) <= 0.01


def test_dropout_changes_the_gradient(oracle):
    cfg = oracle.make_config(**CONFIGS["L7_F32to8_x2"])
    weights = oracle.synthetic_weights(cfg, seed=0)
    x, x2, y = _batch(cfg, 2, 24, 24, 1)
    with _engine(cfg, weights, dropout_rate=0.8) as eng:
        eng.train_gradients(x, x2, y, dropout_key=1)
        a = eng.get_tensor("CNN3/conv_W/grad")
        eng.train_gradients(x, x2, y, dropout_key=2)
        b = eng.get_tensor("CNN3/conv_W/grad")
        eng.train_gradients(x, x2, y, dropout_key=1)
        c = eng.get_tensor("CNN3/conv_W/grad")
    assert not np.array_equal(a, b) and np.array_equal(a, c)


@pytest.mark.parametrize("opt", ["adam", "momentum", "gd"])
def test_one_optimizer_step_matches_tf_update_rules(oracle, opt):
    cfg = oracle.make_config(**CONFIGS["L7_F32to8_x2"])
    weights = oracle.synthetic_weights(cfg, seed=2)
    x, x2, y = _batch(cfg, 3, 24, 24, 5)
    lr = 1e-3
    with _engine(cfg, weights, optimizer=opt, clipping_norm=5.0) as eng:
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
    clip, norm = R.clip_factor(g, 5.0)
    assert norm > 5.0                                               # the clip is exercised
    f32 = lambda v: float(np.float32(v))                           # TF holds the hyperparameters as float32 constants
    b1, b2, lr = f32(0.9), f32(0.999), f32(lr)
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


def _train(eng, batches, steps, start=0, lr=1e-3):
    for i in range(start, start + steps):
        x, x2, y = batches[i % len(batches)]
        eng.train_step(x, x2, y, lr, dropout_key=1000 + i)


def _state(eng, names, opt="adam"):
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


def test_two_runs_are_bit_identical_and_device_steps_match_host_steps(oracle):
    cfg = oracle.make_config(**CONFIGS["L7_F32to8_x2"])
    weights = oracle.synthetic_weights(cfg, seed=0)
    batches = [_batch(cfg, 4, 24, 24, s) for s in range(3)]
    states = []
    for _ in range(2):
        with _engine(cfg, weights, dropout_rate=0.8) as eng:
            _train(eng, batches, 20)
            states.append(_state(eng, weights))
    _assert_same_bits(states[0], states[1])
    with _engine(cfg, weights, dropout_rate=0.8) as eng:
        dev = [tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in b) for b in batches]
        torch.cuda.synchronize()
        for i in range(20):
            x, x2, y = dev[i % 3]
            eng.train_step_device(x.data_ptr(), x2.data_ptr(), y.data_ptr(), 4, 24, 24, 1e-3, dropout_key=1000 + i,
                                  want_stats=(i == 19))
        _assert_same_bits(states[0], _state(eng, weights))


def test_resume_from_a_checkpoint_reproduces_the_straight_run(oracle):
    from dcscn_amd import ckpt
    cfg = oracle.make_config(**CONFIGS["L7_F32to8_x2"])
    weights = oracle.synthetic_weights(cfg, seed=0)
    batches = [_batch(cfg, 4, 24, 24, s) for s in range(3)]
    with _engine(cfg, weights, dropout_rate=0.8) as eng:
        _train(eng, batches, 20)
        straight = _state(eng, weights)
    with tempfile.TemporaryDirectory() as d:
        prefix = os.path.join(d, "model")
        with _engine(cfg, weights, dropout_rate=0.8) as eng:
            _train(eng, batches, 10)
            ckpt.save_checkpoint(prefix, _state(eng, weights))
        saved = ckpt.load_checkpoint(prefix, include_optimizer_slots=True)
    for k, v in weights.items():
        assert saved[k + "/Adam"].shape == v.shape and saved[k + "/Adam_1"].shape == v.shape
    assert saved["beta1_power"].shape == () and saved["beta2_power"].shape == ()
    with _engine(cfg, {k: saved[k] for k in weights}, dropout_rate=0.8) as eng:
        for k, v in saved.items():
            if k not in weights:
                eng.set_train_tensor(k, v)
        _train(eng, batches, 10, start=10)
        _assert_same_bits(straight, _state(eng, weights))


@pytest.mark.parametrize("name,split16", [("L7_F32to8_x2", True), ("L7_F32to8_x2", False), ("L7_F32to8_x4", True),
                                          ("L7_F32to8_x4", False), ("L12_F196to48_x4", True)])
def test_forward_after_training_uses_the_trained_weights(oracle, name, split16):
    """x4 included: there the inference plan folds the whole tail at pack time (fold_whole_tail / pack_foldx)."""
    from dcscn_amd import engine
    cfg = oracle.make_config(**CONFIGS[name])
    weights = oracle.synthetic_weights(cfg, seed=0)
    x, x2, y = _batch(cfg, 2, 32, 32, 9)
    with engine.Engine(cfg, device=0) as fresh:
        fresh.load_weights(weights, split16=split16)
        before = fresh.forward(x, x2)
    eng = engine.Engine(cfg, device=0)
    eng.load_weights(weights, split16=split16)
    eng.train_begin(FLAGS)
    assert np.array_equal(eng.forward(x, x2), before)              # train_begin alone changes nothing
    for i in range(3):
        eng.train_step(x, x2, y, 1e-3, dropout_key=i)
    trained = {k: eng.get_tensor(k) for k in weights}
    after = eng.forward(x, x2)
    eng.close()
    assert not np.array_equal(after, before)
    with engine.Engine(cfg, device=0) as ref:
        ref.load_weights(trained, split16=split16)
        assert np.array_equal(ref.forward(x, x2), after)


def _set14_batches(scale, n, size, count, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    files = sorted(os.listdir(os.path.join(GOLDEN, "set14")))
    import dcscn_oracle as O
    ys = []
    for f in files:
        im = np.asarray(Image.open(os.path.join(GOLDEN, "set14", f)).convert("RGB"))
        ys.append(O.rgb_to_y(im)[..., 0] if O.rgb_to_y(im).ndim == 3 else O.rgb_to_y(im))
    hr = size * scale
    out = []
    for _ in range(count):
        xs, x2s, yts = [], [], []
        for _ in range(n):
            y = ys[rng.integers(len(ys))]
            t = rng.integers(0, y.shape[0] - hr + 1)
            l = rng.integers(0, y.shape[1] - hr + 1)
            yt = y[t:t + hr, l:l + hr].astype(np.float32)
            if rng.random() < 0.5:
                yt = yt[:, ::-1]
            lr = O.pil_bicubic(yt[..., None], 1.0 / scale)
            xs.append(lr)
            x2s.append(O.pil_bicubic(lr, scale))
            yts.append(yt[..., None])
        out.append((np.stack(xs).astype(np.float32), np.stack(x2s).astype(np.float32), np.stack(yts).astype(np.float32)))
    return out


def _he_init(oracle, cfg, seed):
    """The reference's initial values: He truncated normal filters (utilty.py:360-363, 393-413), zero biases (utilty.py:416),
    PReLU alphas 0.1 (tf_graph.py:91).  synthetic_weights draws the same filters but scales the last one by 0.01: undone."""
    w = oracle.synthetic_weights(cfg, seed=seed)
    last = "R-CNN%d" % cfg["reconstruct_layers"]
    out = {}
    for k, v in w.items():
        if k.endswith("/conv_B"):
            out[k] = np.zeros_like(v)
        elif "/prelu/" in k:
            out[k] = np.full_like(v, 0.1)
        elif k.startswith(last + "/"):
            out[k] = (v.astype(np.float64) * 100.0).astype(np.float32)
        else:
            out[k] = v
    return out


def test_it_learns(oracle):
    from PIL import Image
    cfg = oracle.make_config(**CONFIGS["L7_F32to8_x2"])
    weights = _he_init(oracle, cfg, seed=7)
    batches = _set14_batches(2, 20, 32, 50, seed=0)
    mse = []
    with _engine(cfg, weights, dropout_rate=0.8) as eng:
        for i in range(500):
            x, x2, y = batches[i % len(batches)]
            mse.append(eng.train_step(x, x2, y, 2e-3, dropout_key=i)[1])
        with open(os.path.join(GOLDEN, "goldens.json")) as f:
            g = json.load(f)
        psnr = []
        for name in g["files"]:
            im = np.asarray(Image.open(os.path.join(GOLDEN, "set5", name)).convert("RGB"))
            im = oracle.align(im, 2)
            true_y, out = eng.evaluate_rgb(im)
            psnr.append(oracle.psnr_y(true_y[..., 0], out[..., 0], 2))
    first, last = float(np.mean(mse[:50])), float(np.mean(mse[-50:]))
    bicubic = float(np.mean(g["bicubic"]["x2"]))
    print("it learns: mean training MSE first 50 steps %.3f, last 50 steps %.3f (ratio %.3f); Set5 PSNR %.3f dB (bicubic %.3f dB)"
          % (first, last, last / first, float(np.mean(psnr)), bicubic))
    assert last <= 0.5 * first
    assert float(np.mean(psnr)) > bicubic


def test_refusals(oracle):
    from dcscn_amd import engine
    ds = oracle.make_config(**CONFIGS["L7_F32to8_x4_DS"])
    with engine.Engine(ds, device=0) as eng:
        eng.load_weights(oracle.synthetic_weights(ds, seed=0))
        with pytest.raises(engine.EngineError) as e:
            eng.train_begin(FLAGS)
        assert e.value.status == 2 and "separable" in e.value.message
    tc = oracle.make_config(layers=3, filters=8, min_filters=4, nin_filters=4, nin_filters2=4, pixel_shuffler=False)
    with engine.Engine(tc, device=0) as eng:
        eng.load_weights(oracle.synthetic_weights(tc, seed=0))
        with pytest.raises(engine.EngineError) as e:
            eng.train_begin(FLAGS)
        assert e.value.status == 2 and "transposed" in e.value.message
    cfg = oracle.make_config(**CONFIGS["L7_F32to8_x2"])
    weights = oracle.synthetic_weights(cfg, seed=0)
    x, x2, y = _batch(cfg, 2, 16, 16, 0)
    for opt in ("adadelta", "adagrad", "rmsprop"):
        with engine.Engine(cfg, device=0) as eng:
            eng.load_weights(weights)
            with pytest.raises(engine.EngineError) as e:
                eng.train_begin(dict(FLAGS, optimizer=opt))
            assert e.value.status == 2 and opt in e.value.message
    with engine.Engine(cfg, device=0) as eng:
        with pytest.raises(engine.EngineError) as e:
            eng.train_begin(FLAGS)
        assert e.value.status == 6                                  # before finalize
        eng.load_weights(weights)
        with pytest.raises(engine.EngineError) as e:
            eng.train_step(x, x2, y, 1e-3)
        assert e.value.status == 6 and "train_begin" in e.value.message
        eng.train_begin(FLAGS)
        with pytest.raises(engine.EngineError) as e:
            eng.train_step(x, x2[:, :-2], y, 1e-3)
        assert e.value.status == 4                                  # the binding: arrays that do not form a batch
        with pytest.raises(engine.EngineError) as e:
            eng.train_step(x[:0], x2[:0], y[:0], 1e-3)
        assert e.value.status == 1 and "bad shape" in e.value.message          # the library: an empty batch
        with pytest.raises(engine.EngineError) as e:
            eng.get_tensor("CNN1/conv_W/Momentum")
        assert e.value.status == 4
        eng.set_option("workspace_budget_bytes", 1 << 20)
        with pytest.raises(engine.EngineError) as e:
            eng.train_step(*_batch(cfg, 8, 64, 64, 0), 1e-3)
        assert e.value.status == 7
