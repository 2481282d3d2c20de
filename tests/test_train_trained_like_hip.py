"""Training under weights with the value statistics of the trained checkpoints (tests/trained_like.py), and at pre-activations that
are exactly zero, against the float64 restatement of tests/train_ref.py.

Gradients.  tact_fwd / tact_bwd, tconv_gemm(_h) and tconv_wgrad(_h) have only ever seen slopes of U(0.05, 0.3), on which
``max(z, a z)`` and a clamped slope have the gradients of PReLU; tests/test_trained_like_host.py shows that here either moves a
gradient tensor by at least 4740 x the bar.  Judged by test_train_surface_hip._compare at 1e-4 * max|g64|, in the four settings of
("train_split16", "train_split16_wgrad").

Steps.  Three Adam steps from the trained-like state carry a slope of -5.84 and a slope of exactly 0 through the update rule.

Exact zeros.  On a black image with zero biases every pre-activation is exactly 0, and tact_bwd has to take the derivative the
reference's graph takes there: a / 2 (prelu), 1 (leaky_relu), 1.0507 (selu), 0 (relu) -- see tests/train_ref.py: _act and the
"ties" paragraph of include/dcscn.h.  The convention is derived from the reference graph and TensorFlow 1.x's gradient
registrations; TensorFlow was not run."""
import numpy as np
import pytest

import train_ref as R
import train_split16_wgrad_cases as W
import trained_like as T
from test_train_surface_hip import _close, _compare, _f32, _grads_at, _read

pytestmark = pytest.mark.gpu


def _run(label, cfg, weights, x, x2, y, keep, key):
    """The gradients of one batch in the four option settings, each judged by _compare."""
    for s16, wg16 in T.TRAIN_OPTIONS:
        with W.engine_for(cfg, weights, s16, wg16, dropout_rate=keep, l2_decay=T.L2_DECAY) as eng:
            stats, got = _grads_at(eng, weights, x, x2, y, key)
        _compare("%s train_split16 %d wgrad %d" % (label, s16, wg16), cfg, weights, x, x2, y, stats, got, keep=keep, key=key, tol=T.TOL)


@pytest.mark.parametrize("keep", T.KEEPS)
@pytest.mark.parametrize("spread", T.SPREADS)
@pytest.mark.parametrize("name,flags,nhw", T.TRAIN_CASES, ids=[c[0] for c in T.TRAIN_CASES])
def test_gradients_under_trained_like_weights(name, flags, nhw, spread, keep):
    cfg, weights, x, x2, y = T.train_case(flags, nhw, spread)
    _run("trained-like %s %dx%dx%d spread %d keep %.1f" % ((name,) + nhw + (spread, keep)), cfg, weights, x, x2, y, keep, T.TRAIN_KEY)


def test_three_adam_steps_from_the_trained_like_state():
    """test_six_steps_match_tf_update_rules_from_the_device_state's procedure and bars on ODD: before every step the variables, the
    slots and the powers are read from the device and the float64 rule is applied with the device's own gradient times the clip."""
    name, flags, nhw = T.TRAIN_CASES[0]
    cfg, weights, _, _, _ = T.train_case(flags, nhw, T.SPREAD)
    batches = [T.C._batch(cfg, *nhw, s) for s in (5, 6)]
    slopes, _ = T.pools()
    first = weights["CNN1/prelu/CNN1_prelu"]
    assert first[0] == slopes.min() and first[0] < -5.8 and first[2] == 0.0
    lr, b1, b2, eps = _f32(1e-3), _f32(0.9), _f32(0.999), _f32(1e-8)
    p1, p2 = np.float32(0.9), np.float32(0.999)
    with W.engine_for(cfg, weights, 0, 0, optimizer="adam", clipping_norm=5.0, dropout_rate=0.8) as eng:
        for step in range(3):
            x, x2, y = batches[step % 2]
            w0, s0 = _read(eng, weights, "adam")
            if step == 0:
                assert all(np.array_equal(w0[k], weights[k]) for k in weights)
            eng.train_gradients(x, x2, y, dropout_key=700 + step)
            g = {k: eng.get_tensor(k + "/grad").astype(np.float64) for k in weights}
            eng.train_step(x, x2, y, 1e-3, dropout_key=700 + step)
            w1, s1 = _read(eng, weights, "adam")
            clip, norm = R.clip_factor(g, 5.0)
            assert norm > 5.0                                       # the clip is exercised on every step
            for k in weights:
                what = "adam step %d %s" % (step, k)
                want, m, v = R.adam(w0[k].astype(np.float64), g[k] * clip, s0[k][0].astype(np.float64), s0[k][1].astype(np.float64),
                                    float(p1), float(p2), lr, b1=b1, b2=b2, eps=eps)
                _close(s1[k][0], m, what + " m")
                _close(s1[k][1], v, what + " v")
                _close(w1[k], want, what)
            assert w1["CNN1/prelu/CNN1_prelu"][2] != 0.0 and w1["CNN1/prelu/CNN1_prelu"][0] != w0["CNN1/prelu/CNN1_prelu"][0]
            p1, p2 = p1 * np.float32(0.9), p2 * np.float32(0.999)


@pytest.mark.parametrize("act", T.ZERO_ACTS)
@pytest.mark.parametrize("name,flags", T.ZERO_NETS, ids=[n[0] for n in T.ZERO_NETS])
def test_gradients_at_exactly_zero_pre_activations(name, flags, act):
    """Image 0 is black and every bias is zero (tests/test_trained_like_host.py asserts that every float64 pre-activation of that
    image is then exactly 0); its target is not its bicubic image, so the loss gradient reaches every tie."""
    cfg, weights, x, x2, y = T.zero_case(flags, act)
    assert not np.any(x[0]) and np.any(y[0] - x2[0])
    _run("exact zeros %s %s" % (name, act), cfg, weights, x, x2, y, 1.0, 0)
