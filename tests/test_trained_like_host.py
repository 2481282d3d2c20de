"""What tests/test_trained_like_hip.py and tests/test_train_trained_like_hip.py rest on, without a GPU (oracle and train_ref only).

1. The pools are what tests/trained_like.py says they are.
2. The float32 restatement of the oracle stays within BAR / 4 of float64 on every inference case and both weight sets, so the GPU
   file's second clause (4 x the case's own float32 restatement) is never the wider of its two bars.
3. No intermediate of the float64 oracle passes half the f16 maximum, so no image of a GPU case takes the float32 fallback.
4. The probe's power.  Under trained-like weights PReLU computed as max(v, a v), or with the slope clamped to [0, 1], moves the
   bare-branch output by at least 1000 x BAR; under ``oracle.synthetic_weights`` the max form moves it by EXACTLY 0 on every case:
   that is the blind spot these weights close.
5. Training: float32 torch autograd of train_ref stays within TOL / 4 of max|g64| per tensor, no gradient is identically zero, and
   each mutant inside train_ref moves at least one gradient tensor by 100 x TOL of its max|g64|.
6. train_ref at exact zeros: on a black image with zero biases every pre-activation is exactly 0 and the activators, restated as the
   reference writes them, take there the derivatives a / 2 (prelu), 1 (leaky_relu), 1.0507 (selu) and 0 (relu).

Measured (this file, -s; the lines are in profiles/r16_trained_like.txt): float32 restatement 2.0e-7 (separable x4) .. 1.1e-6 (L12 x2,
spread 0) against BAR / 4 = 1.25e-6; largest intermediate 0.24 of the f16 maximum (the net without NIN, spread 0).  The max form moves
the bare branch by 2254 x BAR (separable x4, spread 3) .. 86111 x BAR, the clamped slope by 10171 .. 244080 x BAR.  Training: float32
autograd 4.5e-7 .. 2.9e-6 of max|g64| against TOL / 4 = 2.5e-5; the max form moves a gradient tensor by 4740 .. 30599 x TOL, the
clamped slope by 10035 .. 15781 x TOL; no seed had to be changed."""
import numpy as np
import pytest
import torch

import bare_branch as B
import train_ref as R
import trained_like as T

F16_MAX = 65504.0

_IDS = [c[0] for c in T.INFER_CASES]
_REF = {}


def _case(oracle, case, spread):
    """(cfg, weights, x, x2, float64 reference with its intermediates), computed once per (net, spread)."""
    name, flags, n, hw, _ = case
    if (name, spread) not in _REF:
        cfg, weights, x, x2 = T.bare_case(flags, n, hw, spread)
        ref, inter = oracle.forward(cfg, weights, x, x2, dtype=np.float64, return_intermediates=True)
        ref.flags.writeable = False
        _REF[name, spread] = (cfg, weights, x, x2, ref, max(float(np.max(np.abs(v))) for v in inter.values()))
    return _REF[name, spread]


def test_pools_are_the_shipped_checkpoints():
    slopes, biases = T.pools()
    assert slopes.dtype == np.float32 and biases.dtype == np.float32
    assert slopes.size == 513 and biases.size == 658
    assert abs(float(slopes.min()) + 5.84) < 0.005 and abs(float(slopes.max()) - 1.61) < 0.005
    assert abs(float(biases.min()) + 35.3) < 0.05 and abs(float(biases.max()) - 23.9) < 0.05
    assert int((slopes < 0).sum()) == 59 and int((slopes > 1).sum()) == 5
    assert abs(float(biases.std()) - 8.5) < 0.05


def test_trained_like_weights_are_what_the_helper_says(oracle):
    slopes, biases = T.pools()
    for flags in (T.CONFIGS["L8_F96to48_x2"], T.CONFIGS["L7_F32to8_x4_DS"], T.FLAG_VARIANTS[4][1]):
        cfg = oracle.make_config(**flags)
        base = oracle.synthetic_weights(cfg, seed=0)
        flat, wide = T.trained_like_weights(cfg, 0, 0), T.trained_like_weights(cfg, 0, T.SPREAD)
        assert set(flat) == set(wide) == set(base)
        last = "R-CNN%d/" % cfg["reconstruct_layers"]
        for k, v in base.items():
            assert flat[k].dtype == np.float32 and flat[k].shape == v.shape and wide[k].shape == v.shape, k
            leaf = k.rsplit("/", 1)[-1]
            if "/prelu/" in k:
                assert np.isin(flat[k][4 if v.size >= 4 else 0:], slopes).all() and np.array_equal(flat[k], wide[k]), k
                if v.size >= 4:
                    assert list(flat[k][:4]) == [slopes.min(), slopes.max(), 0.0, 1.0], k
            elif leaf == "conv_B":
                assert np.isin(flat[k], biases).all() and np.array_equal(flat[k], wide[k]), k
            else:
                assert np.array_equal(flat[k], v), k
                if leaf in ("conv_W", "pointwise_W") and not k.startswith(last):
                    top = np.max(np.abs(v.reshape(-1, v.shape[3])), axis=0)
                    ratio = np.max(np.abs(wide[k].reshape(-1, v.shape[3])), axis=0) / top
                    assert np.isin(ratio, [0.0] + [2.0 ** -i for i in range(T.SPREAD + 1)]).all(), (k, ratio)
                    assert int((ratio == 0).sum()) == (1 if v.shape[3] >= 8 else 0), (k, ratio)
                else:
                    assert np.array_equal(wide[k], v), k
        # two draws differ, one draw repeats
        assert np.array_equal(T.trained_like_weights(cfg, 0, T.SPREAD)["CNN1/conv_B"], wide["CNN1/conv_B"])
        assert not np.array_equal(T.trained_like_weights(cfg, 1, 0)["CNN1/conv_B"], flat["CNN1/conv_B"])


@pytest.mark.parametrize("spread", T.SPREADS)
@pytest.mark.parametrize("case", T.INFER_CASES, ids=_IDS)
def test_float32_restatement_and_f16_range(oracle, case, spread):
    cfg, weights, x, x2, ref, top = _case(oracle, case, spread)
    r32 = B.restatement_error(oracle, cfg, weights, x, x2, ref)
    print("RESTATEMENT %s spread %d: %.3g of max|branch| %.3g; largest intermediate %.3g = %.3g of the f16 maximum"
          % (case[0], spread, r32, float(np.max(np.abs(ref))), top, top / F16_MAX))
    assert top <= 0.5 * F16_MAX, (case[0], spread, top)
    assert r32 <= B.BAR / 4, (case[0], spread, r32)


@pytest.mark.parametrize("spread", T.SPREADS)
@pytest.mark.parametrize("case", T.INFER_CASES, ids=_IDS)
def test_a_wrong_prelu_form_is_seen_on_the_bare_branch(oracle, case, spread):
    cfg, weights, x, x2, ref, _ = _case(oracle, case, spread)
    for name in T.MUTANTS:
        with T.mutant(name, oracle=oracle):
            moved = B.rel_error(oracle.forward(cfg, weights, x, x2, dtype=np.float64), ref)
        print("MUTANT %s on %s spread %d: moves y by %.3g of max|y| = %.0f x BAR" % (name, case[0], spread, moved, moved / B.BAR))
        assert moved >= 1000 * B.BAR, (case[0], spread, name, moved)


@pytest.mark.parametrize("case", T.INFER_CASES, ids=_IDS)
def test_the_max_form_is_invisible_under_synthetic_weights(oracle, case):
    """The record of the blind spot: slopes of U(0.05, 0.3) make max(v, a v) the same function, bit for bit."""
    name, flags, n, hw, _ = case
    cfg = oracle.make_config(**flags)
    weights = B.bare_weights(cfg, oracle.synthetic_weights(cfg, seed=T.BARE_SEED))
    x, x2 = B.bare_batch(n, hw[0], hw[1], cfg["scale"], T.BARE_SEED + 1)
    ref = oracle.forward(cfg, weights, x, x2, dtype=np.float64)
    with T.mutant("max", oracle=oracle):
        assert np.array_equal(oracle.forward(cfg, weights, x, x2, dtype=np.float64), ref), name


def test_the_mutants_are_not_the_identity_and_restore_the_activator(oracle):
    v, a = np.array([-2.0, -0.0, 3.0]), np.array([-5.0, 1.5, 0.5])
    keep = (oracle.activate, R._act)
    with T.mutant("max", oracle=oracle, train_ref=R):
        assert list(oracle.activate(v, "prelu", a)) == [10.0, 0.0, 3.0]
        assert list(oracle.activate(v, "relu")) == [0.0, 0.0, 3.0]
    with T.mutant("clamp", oracle=oracle, train_ref=R):
        assert list(oracle.activate(v, "prelu", a)) == [0.0, 0.0, 3.0]
    assert (oracle.activate, R._act) == keep
    assert list(oracle.activate(v, "prelu", a)) == [10.0, 0.0, 3.0]


# ---- training -----------------------------------------------------------------------------------------------------------------------
_TIDS = [c[0] for c in T.TRAIN_CASES]


def _ratios(got, g64):
    return {k: float(np.max(np.abs(got[k] - g))) / float(np.max(np.abs(g))) for k, g in g64.items()}


@pytest.mark.parametrize("keep", T.KEEPS)
@pytest.mark.parametrize("spread", T.SPREADS)
@pytest.mark.parametrize("case", T.TRAIN_CASES, ids=_TIDS)
def test_float32_autograd_and_the_mutants_on_training_cases(case, spread, keep):
    name, flags, nhw = case
    cfg, weights, x, x2, y = T.train_case(flags, nhw, spread)
    kw = dict(keep=keep, key=T.TRAIN_KEY, l2_decay=T.L2_DECAY)
    _, g64 = R.loss_and_grads(cfg, weights, x, x2, y, **kw)
    assert all(np.any(g) for g in g64.values()), [k for k, g in g64.items() if not np.any(g)]
    _, g32 = R.loss_and_grads(cfg, weights, x, x2, y, dtype=torch.float32, **kw)
    f32 = _ratios(g32, g64)
    worst = max(f32, key=f32.get)
    print("AUTOGRAD32 %s spread %d keep %.1f: %.3g of max|g64| (%s)" % (name, spread, keep, f32[worst], worst))
    assert f32[worst] <= T.TOL / 4, (name, spread, keep, worst, f32[worst])
    for m in T.MUTANTS:
        with T.mutant(m, train_ref=R):
            _, gm = R.loss_and_grads(cfg, weights, x, x2, y, **kw)
        moved = _ratios(gm, g64)
        top = max(moved, key=moved.get)
        print("MUTANT %s on %s spread %d keep %.1f: moves %s by %.3g of its max|g64| = %.0f x TOL" % (m, name, spread, keep, top, moved[top], moved[top] / T.TOL))
        assert moved[top] >= 100 * T.TOL, (name, spread, keep, m, top, moved[top])


# ---- exact zeros --------------------------------------------------------------------------------------------------------------------
TIE = {"prelu": None, "leaky_relu": 1.0, "selu": 1.0507009873554805, "relu": 0.0}     # prelu: half the layer's slope


@pytest.mark.parametrize("act", T.ZERO_ACTS)
@pytest.mark.parametrize("net", T.ZERO_NETS, ids=[n[0] for n in T.ZERO_NETS])
def test_a_black_image_without_biases_sits_on_the_tie(oracle, net, act):
    """Every float64 pre-activation of image 0 is exactly 0 (+0 or -0), and train_ref's dz / dh there is the reference graph's."""
    cfg, weights, x, x2, y = T.zero_case(net[1], act)
    layers = [op for op in oracle.build_topology(cfg) if op["op"] == "conv" and op["act"]]
    assert len(layers) >= 3
    taps = {op["var"]: None for op in layers}
    leaves = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in weights.items()}
    out = R.forward(cfg, leaves, x, x2, taps=taps)
    assert not np.any(out.detach().numpy()[0] - np.transpose(x2, (0, 3, 1, 2))[0])          # the branch of image 0 is 0: y_ = x2
    for op in layers:
        z, h = taps[op["var"]]
        assert not np.any(z.detach().numpy()[0]) and np.any(z.detach().numpy()[1]), op["var"]
        dh = torch.autograd.grad(h[0].sum(), z, retain_graph=True)[0][0].numpy()          # elementwise: d h / d z at the tie
        want = TIE[act]
        if want is None:
            want = 0.5 * weights[op["var"] + "/prelu/" + op["name"] + "_prelu"].astype(np.float64)[:, None, None]
        assert np.array_equal(dh, np.broadcast_to(want, dh.shape)), (op["var"], act, dh.ravel()[:4])
    _, g64 = R.loss_and_grads(cfg, weights, x, x2, y, l2_decay=T.L2_DECAY)
    assert all(np.isfinite(g).all() and np.any(g) for g in g64.values())
