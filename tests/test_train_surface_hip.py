"""Training on the GPU over the trainable flag surface, the edge shapes, later steps, re-carved arenas and a caller's stream.

The reference of every comparison is the float64 restatement of tests/train_ref.py (``loss_and_grads`` for gradients and
losses, the numpy update rules for the optimizers); a second run of the library is the reference only where bit-identity is
the stated property.  Every gradient check also evaluates the restatement in torch float32 and prints the device's and
float32 torch's worst ``max|g - g64| / max|g64|`` side by side (``RATIO ...`` lines, pytest -s), so that a bar can be read
against what plain float32 autograd reaches on the same inputs."""
import numpy as np
import pytest
import torch

from conftest import CONFIGS
import train_ref as R
from test_train_hip import K5, _assert_same_bits, _batch, _engine, _state, _train

pytestmark = pytest.mark.gpu

TRANSCENDENTAL = ("sigmoid", "tanh", "selu")
L2_DECAY = 1e-3


def _ratios(got, g64):
    """{name: max|got - g64| / max|g64|}; a reference gradient that is identically zero gives 0 or inf."""
    out = {}
    for name, g in g64.items():
        top = float(np.max(np.abs(g)))
        err = float(np.max(np.abs(np.asarray(got[name], np.float64) - g)))
        out[name] = err / top if top > 0.0 else (0.0 if err == 0.0 else float("inf"))
    return out


def _worst(ratios):
    name = max(ratios, key=lambda k: ratios[k])
    return ratios[name], name


def _compare(label, cfg, weights, x, x2, y, stats, got, keep=1.0, key=0, l1=False, tol=1e-4, context=None, restatement=R):
    """The assertions of the random walk: gradients within ``tol * max|g64|``, exact zeros where the float64 gradient is
    identically zero, image loss / mse / total loss to 1e-6 relative, the global norm to 1e-4 relative, everything finite.
    ``restatement`` is the module whose ``loss_and_grads`` restates the net's graph (tests/train_ref.py; train_ref_transposed.py for
    the separable and the transposed nets).  Returns (device ratio, float32 torch ratio)."""
    ref, g64 = restatement.loss_and_grads(cfg, weights, x, x2, y, keep=keep, key=key, l1=l1, l2_decay=L2_DECAY)
    _, g32 = restatement.loss_and_grads(cfg, {k: v.astype(np.float32) for k, v in weights.items()}, x, x2, y, keep=keep, key=key, l1=l1,
                              l2_decay=L2_DECAY, dtype=torch.float32)
    _, norm = R.clip_factor(g64, 0.0)
    dev, f32 = _ratios(got, g64), _ratios(g32, g64)
    (dr, dn), (fr, fn) = _worst(dev), _worst(f32)
    print("RATIO %s: device %.3g (%s), float32 torch %.3g (%s); float32 torch at the device's tensor %.3g"
          % (label, dr, dn, fr, fn, f32[dn]))
    print("STATS %s: device %r; reference image_loss %.17g mse %.17g norm %.17g loss %.17g"
          % (label, tuple(stats), ref["image_loss"], ref["mse"], norm, ref["loss"]))
    bad = []
    for name, g in g64.items():
        if not np.isfinite(got[name]).all():
            bad.append("%s: not finite" % name)
        elif not np.any(g):
            if np.any(got[name]):
                bad.append("%s: the float64 gradient is identically zero, the device's max is %.3g"
                           % (name, float(np.max(np.abs(got[name])))))
        elif dev[name] > tol:
            bad.append("%s: max err %.3g of max|g64| (bound %.3g); float32 torch %.3g" % (name, dev[name], tol, f32[name]))
    if not np.isfinite(np.asarray(stats)).all():
        bad.append("stats not finite: %r" % (stats,))
    for i, k, rel in ((0, "image_loss", 1e-6), (1, "mse", 1e-6), (3, "loss", 1e-6)):
        if not abs(stats[i] - ref[k]) <= rel * abs(ref[k]):
            bad.append("stats[%d] %.17g, reference %s %.17g (relative %.3g, bound %.3g)"
                       % (i, stats[i], k, ref[k], abs(stats[i] - ref[k]) / abs(ref[k]), rel))
    if not abs(stats[2] - norm) <= 1e-4 * norm:
        bad.append("stats[2] %.17g, float64 global norm %.17g" % (stats[2], norm))
    if bad:
        pytest.fail("%s %s\n%s" % (label, context if context is not None else "", "\n".join(bad)))
    return dr, fr


def _grads_at(eng, weights, x, x2, y, key=0):
    stats = eng.train_gradients(x, x2, y, dropout_key=key)
    return stats, {name: eng.get_tensor(name + "/grad") for name in weights}


def _check(oracle, label, over, n, h, w, l1=False, keep=1.0, key=0, tol=1e-4, seed=0, context=None):
    cfg = oracle.make_config(**over)
    weights = oracle.synthetic_weights(cfg, seed=seed)
    x, x2, y = _batch(cfg, n, h, w, seed + 1)
    if cfg["activator"] in TRANSCENDENTAL:
        x = x / np.float32(255.0)                                   # as test_transcendental_activators: keep exp / tanh off saturation
    with _engine(cfg, weights, use_l1_loss=l1, dropout_rate=keep, l2_decay=L2_DECAY) as eng:
        stats, got = _grads_at(eng, weights, x, x2, y, key)
    return _compare(label, cfg, weights, x, x2, y, stats, got, keep=keep, key=key, l1=l1, tol=tol, context=context)


# ---------------------------------------------------------------------------------------------
# 1. random walk over the flags dcscn_train_begin accepts
# ---------------------------------------------------------------------------------------------
def _draw(rng):
    scale = int(rng.choice([2, 2, 3, 4]))
    layers = int(rng.integers(1, 6))
    filters = int(rng.choice([4, 9, 24, 37, 52, 66]))
    min_filters = min(int(rng.choice([1, 4, 8, 20, 48])), filters)
    gamma = float(rng.choice([1.0, 1.2, 1.5, 2.0]))
    cnn_size = int(rng.choice([3, 3, 3, 3, 1, 5, 7]))
    use_nin = bool(rng.random() < 0.7)
    nin_filters = int(rng.choice([4, 9, 24, 64]))
    nin_filters2 = int(rng.choice([3, 8, 32]))
    reconstruct_layers = int(rng.choice([0, 1, 1, 2, 3]))
    reconstruct_filters = int(rng.choice([4, 12, 32]))
    activator = str(rng.choice(["prelu", "prelu", "relu", "leaky_relu", "sigmoid", "tanh", "selu"]))
    pixel_shuffler_filters = int(rng.choice([0, 0, 1, 5, 16]))
    h, w = int(rng.integers(1, 25)), int(rng.integers(1, 25))
    n = int(rng.integers(1, 5))
    l1 = bool(rng.random() < 0.25)
    keep = float(rng.choice([1.0, 1.0, 0.8, 0.5]))
    flags = dict(scale=scale, layers=layers, filters=filters, min_filters=min_filters, filters_decay_gamma=gamma, cnn_size=cnn_size,
                 use_nin=use_nin, nin_filters=nin_filters, nin_filters2=nin_filters2, reconstruct_layers=reconstruct_layers,
                 reconstruct_filters=reconstruct_filters, activator=activator, pixel_shuffler=True,
                 pixel_shuffler_filters=pixel_shuffler_filters, depthwise_separable=False)
    return flags, n, h, w, l1, keep


@pytest.mark.parametrize("seed", range(200))
def test_random_trainable_flag_surface(oracle, seed):
    """Seeded draws of the net, the batch shape, the loss and the dropout; weights ``synthetic_weights(cfg, seed)``, batch seed
    ``seed + 1`` with the target noise of test_train_hip._batch, ``dropout_key = seed``.  The bar is the 1e-4 * max|g64| of
    DESIGN.md 8: on the host, torch float32 autograd of the same graph stays within 1.54e-5 of float64 on draws 0..199 of this
    generator with these inputs (worst: draw 92, leaky_relu x4 2x14x18 L1 keep 0.5, CNN3/conv_B; then draw 50, sigmoid, 1.31e-5,
    and draw 29, sigmoid, 1.01e-5; typically 1e-6), below the quarter of the bar asked of a draw that is kept.  So the bar leaves
    the kernels 6.5x over plain float32 for their summation order and the device's expf / tanhf.  Draw 21 has a gradient that
    is identically zero (CNN2/prelu/CNN2_prelu).  No draw is skipped: one that the library refuses fails."""
    flags, n, h, w, l1, keep = _draw(np.random.default_rng(3000 + seed))
    _check(oracle, "walk draw %d" % seed, flags, n, h, w, l1=l1, keep=keep, key=seed, seed=seed,
           context="flags %r n %d h %d w %d l1 %r keep %r" % (flags, n, h, w, l1, keep))


# ---------------------------------------------------------------------------------------------
# 2. directed edge shapes: where the pixel, tap, channel and split masks meet
# ---------------------------------------------------------------------------------------------
EDGE_NETS = [
    ("L7_F32to8_x2", CONFIGS["L7_F32to8_x2"]),
    ("odd-channels-x3-ps5", dict(layers=4, filters=37, min_filters=13, nin_filters=21, nin_filters2=10, scale=3, pixel_shuffler_filters=5)),
    ("k5-x4-r2", dict(layers=3, filters=16, min_filters=8, cnn_size=5, scale=4, reconstruct_layers=2, reconstruct_filters=8)),
]
EDGE_BATCHES = [(1, 1, 1), (1, 1, 6), (2, 7, 1), (1, 2, 2), (3, 5, 7), (1, 17, 33), (5, 16, 16)]
K7 = dict(layers=2, filters=12, min_filters=8, cnn_size=7)
EDGE_CASES = [(name, over, nhw) for name, over in EDGE_NETS for nhw in EDGE_BATCHES] + [("k7", K7, (1, 3, 3)), ("k7", K7, (2, 2, 9))]


@pytest.mark.parametrize("name,over,nhw", EDGE_CASES, ids=["%s-%dx%dx%d" % ((c[0],) + c[2]) for c in EDGE_CASES])
def test_edge_shapes(oracle, name, over, nhw):
    """One-pixel images and axes, a batch of one, pixel counts below and across the 16-pixel k-step and the 128-pixel workgroup,
    a 7x7 kernel wider than the image; MSE, no dropout, weights seed 0, batch seed 1.  Bar 1e-4 * max|g64|: torch float32 is
    within 6.2e-6 on every case (worst L7_F32to8_x2 on 2x7x1, B2/prelu/B2_prelu) and no gradient tensor is identically zero."""
    _check(oracle, "edge %s %dx%dx%d" % ((name,) + nhw), over, *nhw)


def test_several_wgrad_splits_at_high_resolution(oracle):
    """L7 x4 on 3x37x50: 5,550 LR and 88,800 HR pixels, several weight-gradient splits at every resolution and split lengths that
    the pixel count does not fill.  A batch of this order has the 5e-4 bar of test_gradients_full_size_batch (the pixel sums are
    f32 chains inside a split), but the device measures 4.7e-7 * max|g64| here (CNN7/prelu/CNN7_prelu; torch float32 8.9e-7,
    CNN1/conv_W), so the bar is the 1e-4 of every other case."""
    dr, fr = _check(oracle, "splits L7_F32to8_x4 3x37x50", CONFIGS["L7_F32to8_x4"], 3, 37, 50, tol=1e-4)
    print("several splits: device ratio %.3g, float32 torch %.3g (bar 1e-4)" % (dr, fr))


# ---------------------------------------------------------------------------------------------
# 3. gradients at weights that are not the loaded ones
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,over", [("L7_F32to8_x2", CONFIGS["L7_F32to8_x2"]), ("k5_relu_r2_nonin", K5)])
def test_gradients_after_the_weights_have_moved(oracle, name, over):
    """tpack_dgrad rebuilds the data-gradient filters from the master copy every step: after 5 Adam steps, and again after
    set_train_tensor has replaced every variable (the resume path), the gradients at the weights read back with get_tensor match
    float64 autograd at those weights."""
    cfg = oracle.make_config(**over)
    weights = oracle.synthetic_weights(cfg, seed=0)
    batches = [_batch(cfg, 3, 20, 24, s) for s in (1, 2)]
    x, x2, y = _batch(cfg, 2, 18, 22, 3)
    with _engine(cfg, weights, dropout_rate=0.8, l2_decay=L2_DECAY) as eng:
        _train(eng, batches, 5)
        moved = {k: eng.get_tensor(k) for k in weights}
        assert all(not np.array_equal(moved[k], weights[k]) for k in weights)
        stats, got = _grads_at(eng, weights, x, x2, y, key=77)
        _compare("moved %s after 5 adam steps" % name, cfg, moved, x, x2, y, stats, got, keep=0.8, key=77)
        other = oracle.synthetic_weights(cfg, seed=5)
        for k, v in other.items():
            eng.set_train_tensor(k, v)
        for k, v in other.items():
            assert np.array_equal(eng.get_tensor(k), v), k
        stats, got = _grads_at(eng, weights, x, x2, y, key=78)
        _compare("moved %s after set_train_tensor" % name, cfg, other, x, x2, y, stats, got, keep=0.8, key=78)


# ---------------------------------------------------------------------------------------------
# 4. every step's update rule, from the state the device really has
# ---------------------------------------------------------------------------------------------
def _f32(v):
    return float(np.float32(v))                                     # TF holds the hyperparameters as float32 constants


def _slot_names(opt):
    return {"adam": ("/Adam", "/Adam_1"), "momentum": ("/Momentum",), "gd": ()}[opt]


def _read(eng, names, opt):
    return {k: eng.get_tensor(k) for k in names}, {k: tuple(eng.get_tensor(k + s) for s in _slot_names(opt)) for k in names}


def _close(got, want, what):
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-6 * np.max(np.abs(want)), err_msg=what)


@pytest.mark.parametrize("opt", ["adam", "momentum", "gd"])
def test_six_steps_match_tf_update_rules_from_the_device_state(oracle, opt):
    """Before every step the variables, the slots and the beta powers are read from the device; the float64 rule is applied to them
    with the device's own gradient (train_gradients with the step's batch and key: bit-reproducible) times the clip factor.  From
    the second step on the slots are not zero, so b1 * m, b2 * v, mu * a and the bias correction of later beta powers are compared."""
    cfg = oracle.make_config(**CONFIGS["L7_F32to8_x2"])
    weights = oracle.synthetic_weights(cfg, seed=2)
    batches = [_batch(cfg, 3, 24, 24, s) for s in (5, 6)]
    lr, b1, b2, mu, eps = _f32(1e-3), _f32(0.9), _f32(0.999), _f32(0.9), _f32(1e-8)
    p1, p2 = np.float32(0.9), np.float32(0.999)
    with _engine(cfg, weights, optimizer=opt, clipping_norm=5.0, dropout_rate=0.8) as eng:
        for step in range(6):
            x, x2, y = batches[step % 2]
            w0, s0 = _read(eng, weights, opt)
            if opt == "adam":
                got_p = (eng.get_tensor("beta1_power"), eng.get_tensor("beta2_power"))
                assert got_p[0].view(np.uint32) == p1.view(np.uint32) and got_p[1].view(np.uint32) == p2.view(np.uint32), (step, got_p, p1, p2)
            eng.train_gradients(x, x2, y, dropout_key=500 + step)
            g = {k: eng.get_tensor(k + "/grad").astype(np.float64) for k in weights}
            eng.train_step(x, x2, y, 1e-3, dropout_key=500 + step)
            w1, s1 = _read(eng, weights, opt)
            clip, norm = R.clip_factor(g, 5.0)
            if step == 0:
                assert norm > 5.0                                   # the clip is exercised
            for k in weights:
                gg, w = g[k] * clip, w0[k].astype(np.float64)
                what = "%s step %d %s" % (opt, step, k)
                if opt == "adam":
                    if step > 0:
                        assert np.any(s0[k][0]) and np.any(s0[k][1]), what
                    want, m, v = R.adam(w, gg, s0[k][0].astype(np.float64), s0[k][1].astype(np.float64), float(p1), float(p2), lr,
                                        b1=b1, b2=b2, eps=eps)
                    _close(s1[k][0], m, what + " m")
                    _close(s1[k][1], v, what + " v")
                elif opt == "momentum":
                    if step > 0:
                        assert np.any(s0[k][0]), what
                    want, a = R.momentum(w, gg, s0[k][0].astype(np.float64), lr, mu)
                    _close(s1[k][0], a, what + " accumulator")
                else:
                    want = R.gd(w, gg, lr)
                _close(w1[k], want, what)
            p1, p2 = p1 * np.float32(0.9), p2 * np.float32(0.999)   # the float32 product chain, one step at a time
        if opt == "adam":
            got_p = (eng.get_tensor("beta1_power"), eng.get_tensor("beta2_power"))
            assert got_p[0].view(np.uint32) == p1.view(np.uint32) and got_p[1].view(np.uint32) == p2.view(np.uint32), (got_p, p1, p2)


LR_UNCLIPPED = 1e-6     # the unclipped gradient of these batches has a norm of about 800: at 1e-3 the loss is not finite after two steps


@pytest.mark.parametrize("clipping_norm", [0.0, 1e9])
@pytest.mark.parametrize("opt", ["momentum", "gd"])
def test_unclipped_steps_are_the_float32_rules_bit_for_bit(oracle, opt, clipping_norm):
    """clipping_norm = 0 (off) and norm <= clipping_norm both give the factor 1.0f exactly (c / fmaxf(norm, c) = c / c).  train.hip
    is compiled with fp contract(off) and topt does one multiply and one add or subtract per term in float32, so g * 1.0f = g and
    the variables and the accumulator equal a numpy float32 emulation with one rounding per operation, bit for bit."""
    cfg = oracle.make_config(**CONFIGS["L7_F32to8_x2"])
    weights = oracle.synthetic_weights(cfg, seed=2)
    batches = [_batch(cfg, 3, 24, 24, s) for s in (5, 6)]
    lr, mu = np.float32(LR_UNCLIPPED), np.float32(0.9)
    with _engine(cfg, weights, optimizer=opt, clipping_norm=clipping_norm, dropout_rate=0.8) as eng:
        for step in range(3):
            x, x2, y = batches[step % 2]
            w0, s0 = _read(eng, weights, opt)
            eng.train_gradients(x, x2, y, dropout_key=600 + step)
            g = {k: eng.get_tensor(k + "/grad") for k in weights}
            _, norm = R.clip_factor({k: v.astype(np.float64) for k, v in g.items()}, 0.0)
            print("unclipped %s clipping_norm %g step %d: gradient norm %.6g" % (opt, clipping_norm, step, norm))
            assert 5.0 < norm < 1e9                                 # a clip at the usual 5.0 would have scaled this gradient
            eng.train_step(x, x2, y, LR_UNCLIPPED, dropout_key=600 + step)
            w1, s1 = _read(eng, weights, opt)
            assert all(np.isfinite(w1[k]).all() for k in weights) and any(not np.array_equal(w1[k], w0[k]) for k in weights)
            want_w, want_a = {}, {}
            for k in weights:
                assert g[k].dtype == np.float32 and w0[k].dtype == np.float32
                if opt == "momentum":
                    a = (mu * s0[k][0]).astype(np.float32) + g[k]
                    want_a[k] = a
                    want_w[k] = w0[k] - (lr * a).astype(np.float32)
                else:
                    want_w[k] = w0[k] - (lr * g[k]).astype(np.float32)
                assert want_w[k].dtype == np.float32
            _assert_same_bits(want_w, w1)
            if opt == "momentum":
                _assert_same_bits(want_a, {k: s1[k][0] for k in weights})


# ---------------------------------------------------------------------------------------------
# 5. a change of batch shape on one handle; steps on a caller's stream
# ---------------------------------------------------------------------------------------------
def _grads_and_stats(eng, names, batch, key):
    stats = eng.train_gradients(*batch, dropout_key=key)
    out = {k + "/grad": eng.get_tensor(k + "/grad") for k in names}
    out["stats"] = np.asarray(stats, np.float64).view(np.uint32)
    return out


def test_a_new_batch_shape_leaves_nothing_of_the_old_one(oracle):
    """carve frees and rebuilds the arena and re-points every buffer when (n, H, W) changes; every reduction's partition depends
    on the shape alone, so a handle that went through a larger and a smaller shape computes the bits of one that did not."""
    cfg = oracle.make_config(**CONFIGS["L7_F32to8_x2"])
    weights = oracle.synthetic_weights(cfg, seed=0)
    a, b, c = _batch(cfg, 4, 24, 24, 1), _batch(cfg, 2, 40, 28, 2), _batch(cfg, 3, 8, 8, 3)
    with _engine(cfg, weights, dropout_rate=0.8) as eng:
        eng.train_step(*a, 1e-3, dropout_key=1)
        after_a = {k: eng.get_tensor(k) for k in weights}
        grads_b = _grads_and_stats(eng, weights, b, 9)             # the larger arena, first use
        eng.train_step(*b, 1e-3, dropout_key=2)
        eng.train_step(*c, 1e-3, dropout_key=3)                     # a smaller one
        moved = {k: eng.get_tensor(k) for k in weights}
        back = _grads_and_stats(eng, weights, a, 4)                 # and the first shape again
    with _engine(cfg, moved, dropout_rate=0.8) as fresh:
        _assert_same_bits(back, _grads_and_stats(fresh, weights, a, 4))
    with _engine(cfg, after_a, dropout_rate=0.8) as fresh:
        _assert_same_bits(grads_b, _grads_and_stats(fresh, weights, b, 9))


def test_device_steps_on_a_callers_stream_match_host_steps(oracle):
    """train_step_device on a stream of the caller's, stats only on the last step, with one change of batch shape in the middle;
    get_tensor then reads on the handle's stream, which the step ordered behind the caller's with an event: the state has the
    bits of the same steps through train_step."""
    cfg = oracle.make_config(**CONFIGS["L7_F32to8_x2"])
    weights = oracle.synthetic_weights(cfg, seed=0)
    shapes = [(4, 24, 24)] * 6 + [(2, 16, 20)] * 6
    batches = [_batch(cfg, *shapes[i], i % 3) for i in range(12)]
    with _engine(cfg, weights, dropout_rate=0.8) as eng:
        for i, (x, x2, y) in enumerate(batches):
            last = eng.train_step(x, x2, y, 1e-3, dropout_key=1000 + i)
        host = _state(eng, weights)
    with _engine(cfg, weights, dropout_rate=0.8) as eng:
        dev = [tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in b) for b in batches]
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        for i, (x, x2, y) in enumerate(dev):
            stats = eng.train_step_device(x.data_ptr(), x2.data_ptr(), y.data_ptr(), *shapes[i], 1e-3, dropout_key=1000 + i,
                                          stream=stream.cuda_stream, want_stats=(i == 11))
        _assert_same_bits(host, _state(eng, weights))
        assert stats == last
        stream.synchronize()
