"""Host side of option "train_optimizers" (adadelta, adagrad, rmsprop) and of --initializer / --weight_dev: the slot names in
checkpoints, the numpy restatement of the rules (tests/train_ref_optimizers.py) against torch.optim on the CPU where the
definitions coincide, and the initial filters of SuperResolution.init_all_variables."""
import math

import numpy as np
import pytest
import torch

import train_ref_optimizers as P

NEW_SLOTS = ("Adagrad", "Adadelta", "Adadelta_1", "RMSProp", "RMSProp_1")


def test_is_optimizer_slot_knows_the_new_suffixes():
    from dcscn_amd import ckpt
    for var in ("CNN1/conv_W", "CNN3/conv_B", "CNN2/prelu/CNN2_prelu", "CNN2/depthwise_W", "Up-TCNN/Tconv_W"):
        assert not ckpt.is_optimizer_slot(var), var
        for leaf in NEW_SLOTS + ("Adam", "Adam_1"):
            assert ckpt.is_optimizer_slot(var + "/" + leaf), (var, leaf)
    assert ckpt.is_optimizer_slot("beta1_power") and ckpt.is_optimizer_slot("beta2_power")
    for opt in P.OPTIMIZERS:
        assert tuple("/" + s for s in ckpt.OPTIMIZER_SLOTS[opt]) == tuple(s for s in P.SLOTS[opt] if s), opt


def test_a_checkpoint_carries_the_new_slots_and_an_evaluating_load_drops_them(tmp_path):
    from dcscn_amd import ckpt
    rng = np.random.default_rng(0)
    tensors = {"CNN1/conv_W": rng.standard_normal((3, 3, 1, 8)).astype(np.float32), "CNN1/conv_B": np.zeros(8, np.float32)}
    for var in list(tensors):
        for leaf in ("RMSProp", "RMSProp_1"):
            tensors[var + "/" + leaf] = rng.standard_normal(tensors[var].shape).astype(np.float32)
    prefix = str(tmp_path / "model.ckpt")
    ckpt.save_checkpoint(prefix, tensors)
    back = ckpt.load_checkpoint(prefix, include_optimizer_slots=True)
    assert set(back) == set(tensors) and "CNN1/conv_W/RMSProp_1" in back
    for k, v in tensors.items():
        assert back[k].shape == v.shape and np.array_equal(back[k].view(np.uint32), v.view(np.uint32)), k
    assert set(ckpt.load_checkpoint(prefix)) == {"CNN1/conv_W", "CNN1/conv_B"}        # what evaluate.py loads


# ---- the restatement against torch.optim (float64, CPU), three steps from TF's initial slots ---------------------------------
def _torch_steps(make, grads, w0):
    p = torch.nn.Parameter(torch.tensor(w0))
    opt = make([p])
    out = []
    for g in grads:
        p.grad = torch.tensor(g)
        opt.step()
        out.append(p.detach().numpy().copy())
    return out


def _problem():
    rng = np.random.default_rng(7)
    w0 = rng.standard_normal(64)
    grads = [rng.standard_normal(64) * 10.0 ** rng.uniform(-4, 1, 64) for _ in range(3)]
    grads[1][:4] = 0.0
    return w0, grads


def test_adagrad_restatement_agrees_with_torch():
    """Matched: initial_accumulator_value = 0.1 (TF's default, the library's constant); torch's eps = 0 and lr_decay = 0, which TF's
    rule does not have.  Then both are w - lr g / sqrt(acc + g^2)."""
    w0, grads = _problem()
    lr = 0.01
    want = _torch_steps(lambda ps: torch.optim.Adagrad(ps, lr=lr, lr_decay=0.0, initial_accumulator_value=P.ADAGRAD_INITIAL_ACCUMULATOR,
                                                        eps=0.0), grads, w0)
    w, acc = w0, np.full_like(w0, P.ADAGRAD_INITIAL_ACCUMULATOR)
    for g, t in zip(grads, want):
        w, acc = P.adagrad(w, g, acc, lr)
        np.testing.assert_allclose(w, t, rtol=1e-12, atol=1e-14)


def test_adadelta_restatement_agrees_with_torch():
    """Matched: rho = 0.95 and eps = 1e-8 (TF's defaults; torch's own are 0.9 and 1e-6), weight_decay = 0.  Both put eps inside both
    square roots and start both accumulators at 0."""
    w0, grads = _problem()
    lr = 0.5
    want = _torch_steps(lambda ps: torch.optim.Adadelta(ps, lr=lr, rho=P.ADADELTA_RHO, eps=P.ADADELTA_EPS), grads, w0)
    w, acc, upd = w0, np.zeros_like(w0), np.zeros_like(w0)
    for g, t in zip(grads, want):
        w, acc, upd = P.adadelta(w, g, acc, upd, lr, rho=P.ADADELTA_RHO, eps=P.ADADELTA_EPS)
        np.testing.assert_allclose(w, t, rtol=1e-12, atol=1e-14)
    assert np.any(upd != 0)                                          # the second accumulator fed the later steps


def test_rmsprop_restatement_and_torch():
    """torch.optim.RMSprop adds eps OUTSIDE the square root (g / (sqrt(ms) + eps)), TF inside (g / sqrt(ms + eps)), and torch
    starts ms at 0 where TF starts it at 1: with TF's constants the definitions differ, and that comparison is skipped.  They
    coincide at eps = 0 from equal ms, under a constant lr (TF scales g by lr before the momentum accumulator, torch after it),
    so the rest of the rule is compared there: alpha = decay = 0.9, momentum = 0.9, not centred, eps = 0, ms from 0."""
    w0, grads = _problem()
    grads = [np.where(g == 0.0, 1e-3, g) for g in grads]              # eps = 0 and ms = 0: a zero gradient would be 0 / 0
    lr, mu = 0.01, 0.9
    want = _torch_steps(lambda ps: torch.optim.RMSprop(ps, lr=lr, alpha=P.RMSPROP_DECAY, eps=0.0, momentum=mu, centered=False), grads, w0)
    w, ms, mom = w0, np.zeros_like(w0), np.zeros_like(w0)
    for g, t in zip(grads, want):
        w, ms, mom = P.rmsprop(w, g, ms, mom, lr, mu, decay=P.RMSPROP_DECAY, eps=0.0)
        np.testing.assert_allclose(w, t, rtol=1e-12, atol=1e-14)
    # where they differ: TF's placement of its own epsilon, seen on a gradient of its size
    g = np.array([1e-6])
    tf_w, _, _ = P.rmsprop(np.zeros(1), g, np.zeros(1), np.zeros(1), lr, mu, decay=P.RMSPROP_DECAY, eps=1e-10)
    outside = -(g * lr) / (np.sqrt(0.1 * g * g) + 1e-10)
    assert abs(tf_w[0] - outside[0]) > 1e-5 * abs(outside[0])


# ---- --initializer / --weight_dev (utilty.py:348-413) ---------------------------------------------------------------------------
SHAPE = (3, 3, 8, 16)
HE_STD = math.sqrt(2.0 / (3 * 3 * 8))


def _draw(initializer, weight_dev=0.01, seed=3, shape=SHAPE):
    from dcscn_amd.model import initial_filter
    w = initial_filter(shape, initializer, weight_dev, np.random.default_rng(seed))
    assert w.dtype == np.float32 and w.shape == tuple(shape)
    return w


def test_he_is_the_draw_it_always_was():
    """The expression init_all_variables used before --initializer was read, on the same generator: the same bits."""
    rng = np.random.default_rng(3)
    before = np.clip(rng.standard_normal(SHAPE), -2.0, 2.0).astype(np.float32) * np.float32(HE_STD)
    assert np.array_equal(_draw("he").view(np.uint32), before.view(np.uint32))


@pytest.mark.parametrize("initializer,sigma", [("he", HE_STD), ("xavier", math.sqrt(3.0 / (3 * 3 * 8 + 3 * 3 * 16))), ("stddev", 0.037)])
def test_truncated_normals_stay_inside_two_sigma(initializer, sigma):
    w = _draw(initializer, weight_dev=0.037).astype(np.float64)
    s32 = float(np.float32(sigma))
    assert np.max(np.abs(w)) <= 2.0 * s32 * (1 + 2.0 ** -23)            # the clip at 2 sigma, one float32 product
    assert 0.8 * sigma < np.std(w) < sigma                              # a normal truncated at 2 sigma has stddev 0.88 sigma
    assert abs(np.mean(w)) < 0.1 * sigma


def test_uniform_respects_and_approaches_its_bound():
    w = _draw("uniform", weight_dev=0.05).astype(np.float64)
    bound = 2 * 0.05
    assert np.max(np.abs(w)) <= bound * (1 + 2.0 ** -23)
    assert w.max() > 0.98 * bound and w.min() < -0.98 * bound          # 1152 draws: the top 1 % on either side is hit
    assert abs(np.std(w) - bound / math.sqrt(3.0)) < 0.05 * bound


def test_identity_puts_ones_on_the_centre_diagonal():
    w = _draw("identity")
    ones = np.argwhere(w == 1.0)
    assert [tuple(r) for r in ones] == [(1, 1, k, k) for k in range(8)]
    rest = np.array(w)
    rest[1, 1, np.arange(8), np.arange(8)] = 0.0
    assert np.max(np.abs(rest)) <= 2.0 * float(np.float32(HE_STD)) * (1 + 2.0 ** -23) and np.std(rest) > 0.5 * HE_STD   # He elsewhere
    assert np.count_nonzero(_draw("identity", shape=(1, 1, 16, 4)) == 1.0) == 4


def test_an_unknown_initializer_gives_zeros():
    assert not np.any(_draw("zeros")) and not np.any(_draw("anything else"))


def test_init_all_variables_reads_the_flags():
    """The model class passes --initializer and --weight_dev on: conv_W follows them, biases and PReLU slopes do not."""
    from dcscn_amd.model import SuperResolution
    from test_host import _flags

    class Specs:                                                       # stands for the engine: the variable list is all that is asked of it
        def tensor_specs(self):
            return [("CNN2/conv_W", (3, 3, 8, 6)), ("CNN2/conv_B", (6,)), ("CNN2/prelu/CNN2_prelu", (6,)),
                    ("CNN3/depthwise_W", (3, 3, 6, 1)), ("CNN3/pointwise_W", (1, 1, 6, 4))]

    m = SuperResolution(_flags(layers=3, filters=8, min_filters=4, nin_filters=4, nin_filters2=4, initializer="uniform", weight_dev=0.25))
    m._engine = Specs()
    m.init_all_variables()
    t = m._pending_init
    for name in ("CNN2/conv_W", "CNN3/depthwise_W", "CNN3/pointwise_W"):
        top = np.max(np.abs(t[name]))
        assert (0.45 if t[name].size > 50 else 0.25) < top <= 0.5, (name, top)      # U(-0.5, 0.5); 24 draws or more
    assert not np.any(t["CNN2/conv_B"]) and np.all(t["CNN2/prelu/CNN2_prelu"] == np.float32(0.1))
    m.initializer = "none of them"
    m.init_all_variables()
    assert not np.any(m._pending_init["CNN2/conv_W"]) and np.all(m._pending_init["CNN2/prelu/CNN2_prelu"] == np.float32(0.1))
