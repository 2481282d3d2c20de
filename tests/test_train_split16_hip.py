"""Option "train_split16" (include/dcscn.h) on the device: the forward and data-gradient convs of every layer with
min(cin, cout) >= 16 on the f16 matrix pipe as three scaled f16 products (csrc/train_h.hip), everything else the f32 path's.

The reference is the float64 restatement of tests/train_ref.py; a second run of the library is the reference only where bit-identity
is the stated property.  The bars are the f32 path's (tests/train_split16_cases.py says why the mode gets no wider ones).  ``RATIO``
lines (pytest -s) print the device's and float32 torch's worst max|g - g64| / max|g64| side by side.
1 gradient parity per case, 2 small gradients (dz ~ 2e-6), 3 the mode is on where it should be and off where it should be,
4 determinism and state, 5 the entry points, 6 the option itself."""
import numpy as np
import pytest
import torch

import train_ref as R
import train_split16_cases as C
from test_train_hip import FLAGS, _assert_same_bits, _batch, _state, _train
from test_train_surface_hip import _compare

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------
# 1. gradient parity with the option on
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.CASES))
def test_gradients_match_float64_autograd_with_the_option_on(name):
    cfg, weights, x, x2, y = C.inputs(name)
    _, _, _, keep, l1 = C.CASES[name]
    assert C.eligible_layers(cfg), "the case has no eligible layer"
    stats, got = C.device(name, True)
    _compare("train_split16 %s" % name, cfg, weights, x, x2, y, stats, got, keep=keep, key=C.KEY, l1=l1, tol=C.TOL)


# ---------------------------------------------------------------------------------------------
# 2. small gradients: the --max_value 1 scale on 88,800 HR pixels, dz = 2 diff / N ~ 2e-6
# ---------------------------------------------------------------------------------------------
def test_small_gradients_on_the_unit_scale(oracle):
    """The wide odd-channel net as an x4 net on 3x37x50 with inputs and targets on the 0-1 scale.  An unscaled split (lo pieces of dz all
    f16 subnormals) misses the bar by orders of magnitude here; the option-off handle is held to the same bar on the same inputs first."""
    cfg = oracle.make_config(**dict(C.ODD, scale=4))
    weights = oracle.synthetic_weights(cfg, seed=0)
    x, x2, y = (a / np.float32(255.0) for a in _batch(cfg, 3, 37, 50, 1))
    got = {}
    for on in (False, True):
        with C.engine_for(cfg, weights, on, l2_decay=C.L2_DECAY) as eng:
            got[on] = C.grads_and_stats(eng, weights, x, x2, y, key=0)
    n = x2.size
    ref, _ = R.loss_and_grads(cfg, weights, x, x2, y, l2_decay=C.L2_DECAY)
    print("small gradients: mse %.3g, dz ~ 2 sqrt(mse) / N = %.3g" % (ref["mse"], 2.0 * np.sqrt(ref["mse"]) / n))
    assert 2.0 * np.sqrt(ref["mse"]) / n < 1e-5
    for on in (False, True):
        _compare("small gradients, option %s" % ("on" if on else "off"), cfg, weights, x, x2, y, got[on][0], got[on][1], tol=C.TOL)
    assert not C.same_bits(C.bits(*got[False]), C.bits(*got[True]))


# ---------------------------------------------------------------------------------------------
# 3. the mode is really on, and really off
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.NETS)
def test_the_option_changes_bits_where_a_layer_is_eligible(name):
    off, on = C.bits(*C.device(name, False)), C.bits(*C.device(name, True))
    differ = [k for k in off if k != "stats" and not np.array_equal(off[k], on[k])]
    print("%s: %d of %d gradient tensors differ in bits from the option-off handle" % (name, len(differ), len(off) - 1))
    assert differ


def test_a_net_without_an_eligible_layer_keeps_every_bit(oracle):
    cfg = oracle.make_config(**C.NARROW)
    assert not C.eligible_layers(cfg)
    weights = oracle.synthetic_weights(cfg, seed=0)
    x, x2, y = _batch(cfg, 2, 9, 7, 1)
    out = []
    for on in (False, True):
        with C.engine_for(cfg, weights, on, dropout_rate=0.8) as eng:
            out.append(C.bits(*C.grads_and_stats(eng, weights, x, x2, y)))
    assert C.same_bits(out[0], out[1])


@pytest.mark.parametrize("name", ["odd-1x13x11", "mixed-2x8x8"])
def test_toggling_gives_the_bits_of_a_fresh_handle(name):
    cfg, weights, x, x2, y = C.inputs(name)
    fresh = {on: C.bits(*C.device(name, on)) for on in (False, True)}
    with C.engine_for(cfg, weights, True, **C.train_flags(name)) as eng:
        assert C.same_bits(C.bits(*C.grads_and_stats(eng, weights, x, x2, y)), fresh[True])
        eng.set_option("train_split16", 0)
        assert C.same_bits(C.bits(*C.grads_and_stats(eng, weights, x, x2, y)), fresh[False]), "1 -> 0 is not a fresh option-off handle"
        eng.set_option("train_split16", 1)
        assert C.same_bits(C.bits(*C.grads_and_stats(eng, weights, x, x2, y)), fresh[True]), "0 -> 1 is not a fresh option-on handle"
    with C.engine_for(cfg, weights, False, **C.train_flags(name)) as eng:
        assert C.same_bits(C.bits(*C.grads_and_stats(eng, weights, x, x2, y)), fresh[False])
        eng.set_option("train_split16", 1)
        assert C.same_bits(C.bits(*C.grads_and_stats(eng, weights, x, x2, y)), fresh[True]), "0 -> 1 is not a fresh option-on handle"


# ---------------------------------------------------------------------------------------------
# 4. determinism and state
# ---------------------------------------------------------------------------------------------
def _odd(oracle):
    cfg = oracle.make_config(**C.ODD)
    return cfg, oracle.synthetic_weights(cfg, seed=0)


def test_two_handles_agree_over_six_adam_steps_and_the_gradient_there_is_right(oracle):
    cfg, weights = _odd(oracle)
    batches = [_batch(cfg, 2, 12, 10, s) for s in (1, 2, 3)]
    x, x2, y = _batch(cfg, 1, 13, 11, 4)
    states, stats = [], []
    for _ in range(2):
        with C.engine_for(cfg, weights, True, dropout_rate=0.8, l2_decay=C.L2_DECAY) as eng:
            for i in range(6):
                stats.append(eng.train_step(*batches[i % 3], 1e-3, dropout_key=1000 + i))
            states.append(_state(eng, weights))
            if len(states) == 2:
                moved = {k: states[1][k] for k in weights}
                assert all(not np.array_equal(moved[k], weights[k]) for k in weights)
                st, got = C.grads_and_stats(eng, weights, x, x2, y, key=77)
                _compare("train_split16 after 6 adam steps", cfg, moved, x, x2, y, st, got, keep=0.8, key=77, tol=C.TOL)
    _assert_same_bits(states[0], states[1])
    assert stats[:6] == stats[6:]


def test_a_new_batch_shape_leaves_nothing_of_the_old_one(oracle):
    cfg, weights = _odd(oracle)
    a, b = _batch(cfg, 2, 7, 9, 1), _batch(cfg, 2, 16, 15, 2)
    with C.engine_for(cfg, weights, True, dropout_rate=0.8) as eng:
        first = C.bits(*C.grads_and_stats(eng, weights, *a))
        larger = C.bits(*C.grads_and_stats(eng, weights, *b))
        back = C.bits(*C.grads_and_stats(eng, weights, *a))
    assert C.same_bits(first, back)
    with C.engine_for(cfg, weights, True, dropout_rate=0.8) as fresh:
        assert C.same_bits(larger, C.bits(*C.grads_and_stats(fresh, weights, *b)))


# ---------------------------------------------------------------------------------------------
# 5. entry points
# ---------------------------------------------------------------------------------------------
def test_device_steps_and_records_match_host_steps(oracle):
    """train_step_device on a caller's stream = train_step in bits; train_local_gradients_device + train_apply_records at world 1 leave
    the bits of train_step_device."""
    cfg, weights = _odd(oracle)
    shape = (2, 12, 10)
    batches = [_batch(cfg, *shape, s) for s in (1, 2, 3)]
    flags = dict(dropout_rate=0.8, clipping_norm=0.5)
    with C.engine_for(cfg, weights, True, **flags) as eng:
        for i, b in enumerate(batches):
            last = eng.train_step(*b, 1e-3, dropout_key=1000 + i)
        host = _state(eng, weights)
    dev = [tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in b) for b in batches]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with C.engine_for(cfg, weights, True, **flags) as eng:
        for i, (x, x2, y) in enumerate(dev):
            stats = eng.train_step_device(x.data_ptr(), x2.data_ptr(), y.data_ptr(), *shape, 1e-3, dropout_key=1000 + i,
                                          stream=stream.cuda_stream, want_stats=(i == 2))
        _assert_same_bits(host, _state(eng, weights))
        assert stats == last
    with C.engine_for(cfg, weights, True, **flags) as eng:
        rec = torch.zeros((1, eng.train_record_floats()), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for i, (x, x2, y) in enumerate(dev):
            eng.train_local_gradients_device(x.data_ptr(), x2.data_ptr(), y.data_ptr(), *shape, rec.data_ptr(), dropout_key=1000 + i,
                                             first_index=0, stream=stream.cuda_stream)
            stats = eng.train_apply_records(rec.data_ptr(), 1, 1e-3, stream=stream.cuda_stream)
        _assert_same_bits(host, _state(eng, weights))
        assert stats[2] > 0.5 and tuple(stats) == tuple(last)
    stream.synchronize()


def test_forward_after_a_step_uses_the_trained_weights(oracle):
    from dcscn_amd import engine
    cfg, weights = _odd(oracle)
    x, x2, y = _batch(cfg, 2, 12, 10, 9)
    with C.engine_for(cfg, weights, True) as eng:
        before = eng.forward(x, x2)
        for i in range(2):
            eng.train_step(x, x2, y, 1e-3, dropout_key=i)
        trained = {k: eng.get_tensor(k) for k in weights}
        after = eng.forward(x, x2)
    assert not np.array_equal(after, before)
    with engine.Engine(cfg, device=0) as ref:
        ref.load_weights(trained)
        assert np.array_equal(ref.forward(x, x2), after)


# ---------------------------------------------------------------------------------------------
# 6. the option itself
# ---------------------------------------------------------------------------------------------
def test_the_option_is_accepted_before_and_after_train_begin(oracle):
    from dcscn_amd import engine
    cfg, weights = _odd(oracle)
    x, x2, y = _batch(cfg, 1, 4, 4, 1)
    with engine.Engine(cfg, device=0) as eng:
        eng.load_weights(weights)                                   # (finalizes)
        eng.set_option("train_split16", 1)
        eng.set_option("train_split16", 0)
        eng.train_begin(dict(FLAGS))
        eng.set_option("train_split16", 1)
        assert np.isfinite(eng.train_step(x, x2, y, 1e-3)).all()
        eng.set_option("train_split16", 0)
        assert np.isfinite(eng.train_step(x, x2, y, 1e-3)).all()
