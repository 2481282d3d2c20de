"""Option "fast16_stream" (include/dcscn.h) on the device, through the C ABI: every MFMA contraction of a feat3_stream launch (CNN2 .. CNNL
and, with A1 || B1 and B2 inside the launch, those too) takes ONE f16 product per multiply-accumulate (wh * xh) instead of split16's three.
Independent of "fast16", which governs the layer kernels.

What is asserted, and against what (the bars are those derived in tests/test_fast16_hip.py; E_model is the rms error of the CPU restatement
tests/fast16_model.py on the same input and the same set of convs, tests/fast16_stream_cases.py):
1. off means off: fast16_stream = 0, = 1 under split16 = 0 or stream_dense = 0, 1 -> 0 toggles (plain launches and replayed graphs) and
   fast16 = 1 beside fast16_stream = 0 give the bits they gave without the option;
2. it is on, and only as wrong as it should be: device rms against the float64 oracle in [0.5, 2] x E_model, max-abs <= 8 x E_model, output
   differs from the option-off output -- for the stream alone (the LOWER bound proves the lo products are gone: with them the error is
   about 1e-6) and for both options; on every <octets, tiles> instantiation the dispatch can reach and on the pair / NIN roles;
3. default plans with folded tails (x3, x4), both options: rms <= 2 x E_model, output differs from (fast16 1, fast16_stream 0);
4. against the one-product LAYER-BY-LAYER plan (stream_dense = 0, fast16 = 1) on the same one-product set (a 32 .. 24 x3 net: c-DCSCN's
   layer-by-layer plan keeps its narrow layers on a float32 kernel, so its sets differ): both round the same operands
   to f16 and differ in the order of the f32 accumulation, so the outputs differ by a few rounding flips downstream -- a flip needs the f32
   value within about 1e-7 relative of a boundary spaced 4.9e-4, about one value in a thousand, about 0.1 x E_model in rms: the bar is
   rms(difference) <= 0.5 x E_model;
5. two runs give the same bits, an image alone the bits it has in a batch of three, debug_poison = 3 the same bits again;
6. overflow inside the streamed launch (a feature layer, B1): the flagged image has the bits of its split16 = 0 run, bystanders those of a
   fast16_stream run without it, which are not the option-off bits;
7. the shipped c-DCSCN x2 weights on the golden crop, default plan: the band of 2 without a max-abs condition (the restatement's own
   max / rms is 8.3 .. 11.8 there), and through SuperResolution(--fast16 --fast16_stream) a PSNR against the ground truth within
   20 log10(1 + 2 E_model / sqrt(MSE)) of the default's.

Measured on an MI355X (profiles/r14_fast16_stream_numerics.txt): device rms / E_model 0.994 .. 1.013 for the
stream alone on every net and shape of test 2, 0.85 .. 1.41 with both options; 0.36 .. 0.90 in test 3; 0.143 in test 4 (3014 of 5049
values differ); 0.983 and 0.525 in test 7, PSNR delta -9.3e-5 dB against a bound of 1.0e-2 dB."""
import os

import numpy as np
import pytest

import dcscn_oracle
import fast16_model as M
import fast16_stream_cases as S
import overflow_cases as C
import test_hip_parity as P
from conftest import CONFIGS, GOLDEN, synthetic_batch
from test_fast16_host import golden_crop, psnr_delta_bound
from test_host import _flags

pytestmark = pytest.mark.gpu

_NETS = {}


def _net(oracle, name):
    if name not in _NETS:
        cfg = oracle.make_config(**S.NETS[name])
        _NETS[name] = (cfg, oracle.synthetic_weights(cfg, seed=0))
    return _NETS[name]


def _engine(cfg, weights, options=()):
    from dcscn_amd import engine
    eng = engine.Engine(cfg, device=0)
    try:
        for key, value in options:
            eng.set_option(key, value)
        eng.load_weights(weights)
    except Exception:
        eng.close()
        raise
    return eng


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


def _kernels(eng):
    return [o["kernel"] for o in eng.ops()]


def _set(eng, fast16, fast16_stream):
    eng.set_option("fast16", fast16)
    eng.set_option("fast16_stream", fast16_stream)


def _measure(oracle, label, eng, cfg, weights, x, x2, key, fast16):
    """(y of (fast16, 1), y of (fast16, 0), y of (0, 0), rms and max-abs error of the first against the float64 oracle, E_model of the
    one-product set of (fast16, 1)); prints the figures."""
    selected = S.one_product_set(oracle, cfg, eng.ops(), fast16, 1)
    assert S.streamed_set(oracle, cfg, eng.ops()) and selected >= S.streamed_set(oracle, cfg, eng.ops()), _kernels(eng)
    ref, mod, e_model = M.model_error(oracle, key, cfg, weights, x, x2, selected)
    _set(eng, fast16, 1)
    y1 = eng.forward(x, x2)
    _set(eng, fast16, 0)
    y0 = eng.forward(x, x2)
    _set(eng, 0, 0)
    off = eng.forward(x, x2)
    rms, mx = M.rms(y1, ref), M.max_abs(y1, ref)
    print("FAST16_STREAM %s | fast16 %d fast16_stream 1 | device rms %.4g max-abs %.4g | E_model %.4g (max-abs %.4g) | rms / E_model %.3f | "
          "max-abs / E_model %.2f | (%d, 0): rms %.3g | (0, 0): rms %.3g | %d convs on one product"
          % (label, fast16, rms, mx, e_model, M.max_abs(mod, ref), rms / e_model if e_model else float("nan"),
             mx / e_model if e_model else float("nan"), fast16, M.rms(y0, ref), M.rms(off, ref), len(selected)))
    assert np.isfinite(y1).all()
    return y1, y0, off, rms, mx, e_model


# ---------------------------------------------------------------------------------------------
# 1. off means off
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["L7_F32to8_x2", "L7_F32to8_x4", "L2_F32to8"])
def test_off_means_off(oracle, name):
    cfg, weights = _net(oracle, name)
    n, h, w = 2, 19, 35
    x, x2 = synthetic_batch(n, h, w, cfg["scale"], seed=21)
    with _engine(cfg, weights) as eng:                             # handles that never hear of the option
        assert "feat3_stream" in _kernels(eng), _kernels(eng)
        default = eng.forward(x, x2)
    with _engine(cfg, weights, (("stream_dense", 0),)) as eng:
        assert "feat3_stream" not in _kernels(eng), _kernels(eng)
        dense0 = eng.forward(x, x2)
    with _engine(cfg, weights, (("fast16", 1),)) as eng:
        fast = eng.forward(x, x2)
    assert not _same(fast, default)
    with _engine(cfg, weights, (("stream_dense", 0), ("fast16_stream", 1))) as eng:
        assert "feat3_stream" not in _kernels(eng), _kernels(eng)
        assert _same(eng.forward(x, x2), dense0), "fast16_stream = 1 under stream_dense = 0 is not the stream_dense = 0 forward"
    hip = P._Hip()
    try:
        with _engine(cfg, weights) as eng:
            eng.set_option("fast16_stream", 0)
            assert _same(eng.forward(x, x2), default)
            eng.set_option("split16", 0)
            assert "feat3_stream" not in _kernels(eng), _kernels(eng)
            y32 = eng.forward(x, x2)
            eng.set_option("fast16_stream", 1)
            assert _same(eng.forward(x, x2), y32), "fast16_stream = 1 under split16 = 0 is not the split16 = 0 forward"
            eng.set_option("split16", 1)
            assert "feat3_stream" in _kernels(eng), _kernels(eng)
            y1 = eng.forward(x, x2)
            assert not _same(y1, default), "fast16_stream = 1 changed nothing"
            eng.set_option("fast16_stream", 0)
            assert _same(eng.forward(x, x2), default), "1 -> 0 does not give the default bits"
            # beside fast16 = 1: the bits of a handle that only ever set fast16 = 1
            eng.set_option("fast16", 1)
            assert _same(eng.forward(x, x2), fast), "fast16 = 1, fast16_stream = 0 is not the fast16 = 1 forward"
            eng.set_option("fast16_stream", 1)
            assert not _same(eng.forward(x, x2), fast), "fast16_stream = 1 beside fast16 = 1 changed nothing"
            eng.set_option("fast16_stream", 0)
            assert _same(eng.forward(x, x2), fast), "fast16 = 1: 1 -> 0 does not give the fast16 = 1 bits"
            eng.set_option("fast16", 0)
            # the same toggles through replayed graphs: every call repeated so that the capture (second call) and a replay (third) happen
            dx, dx2, dy, st = hip.upload(x), hip.upload(x2), hip.alloc(default.nbytes), hip.stream()
            eng.set_option("graph_replay", 1)
            for value, want in ((1, y1), (0, default), (1, y1), (0, default)):
                eng.set_option("fast16_stream", value)
                for call in range(3):
                    eng.forward_device(dx, dx2, dy, n, h, w, stream=st)
                    eng.synchronize()
                    assert _same(hip.download(dy, default.shape), want), "graph_replay, fast16_stream = %d, call %d" % (value, call)
    finally:
        hip.close()


# ---------------------------------------------------------------------------------------------
# 2. it is on, and only as wrong as it should be
# ---------------------------------------------------------------------------------------------
def _band(label, y1, y0, off, rms, mx, e_model):
    assert not _same(y1, off), "%s: the option-off output" % label
    assert not _same(y1, y0), "%s: fast16_stream = 1 gives the fast16_stream = 0 output" % label
    assert 0.5 * e_model <= rms <= 2.0 * e_model, "%s: device rms %.4g outside [0.5, 2] x E_model %.4g" % (label, rms, e_model)
    assert mx <= 8.0 * e_model, "%s: device max-abs %.4g above 8 x E_model %.4g" % (label, mx, e_model)


@pytest.mark.parametrize("fast16", [0, 1], ids=["stream_alone", "both_on"])
@pytest.mark.parametrize("shape", S.BAND_SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("net,stream_nin", S.BAND_NETS, ids=["%s-nin%d" % c for c in S.BAND_NETS])
def test_one_product_error_band(oracle, net, stream_nin, shape, fast16):
    """Stream alone against E_model(streamed set); both options against E_model(union with the layer kernels' set)."""
    assert set(S.assert_coverage(oracle)) >= {name for name, _ in S.BAND_NETS}
    cfg, weights = _net(oracle, net)
    n, h, w = shape
    x, x2 = synthetic_batch(n, h, w, cfg["scale"], seed=S.BAND_SEED)
    with _engine(cfg, weights, (("stream_nin", stream_nin),)) as eng:
        ops = eng.ops()
        assert ops[0]["kernel"] == "feat3_stream" and ops[0]["name"] == S.streamed_launch_name(cfg, stream_nin), ops[0]
        if net.startswith("L7") and not stream_nin:
            assert S.streamed_set(oracle, cfg, ops) == {"CNN%d" % i for i in range(2, 8)}
        label = "%s stream_nin %d %dx%dx%d" % (net, stream_nin, n, h, w)
        _band(label, *_measure(oracle, label, eng, cfg, weights, x, x2, ("stream band", net) + shape, fast16))


# ---------------------------------------------------------------------------------------------
# 3. default plans with folded tails
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 17, 33)], ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("name", ["L7_F32to8_x3", "L7_F32to8_x4"])
def test_default_plans_stay_within_twice_the_model(oracle, name, shape):
    cfg, weights = _net(oracle, name)
    n, h, w = shape
    x, x2 = synthetic_batch(n, h, w, cfg["scale"], seed=7)
    with _engine(cfg, weights) as eng:
        kernels = _kernels(eng)
        assert "feat3_stream" in kernels and "conv5_h" in kernels, kernels
        label = "%s default plan %dx%dx%d" % (name, n, h, w)
        y1, y0, off, rms, mx, e_model = _measure(oracle, label, eng, cfg, weights, x, x2, ("stream plan", name) + shape, 1)
    assert not _same(y1, y0), "%s: (1, 1) gives the (1, 0) output" % label
    assert rms <= 2.0 * e_model, "%s: device rms %.4g above 2 x E_model %.4g" % (label, rms, e_model)


# ---------------------------------------------------------------------------------------------
# 4. against the one-product layer-by-layer plan
# ---------------------------------------------------------------------------------------------
def test_streamed_and_layer_by_layer_one_product_plans_agree(oracle):
    """Not c-DCSCN x3: its layer-by-layer plan keeps CNN5 .. CNN7 and B2 (fewer than 24 input channels) on conv_igemm, so the streamed
    plan's one-product set is larger by those four.  The net used is the x3 net of five layers 32 .. 24 with B2 24 -> 24, on which every
    conv behind CNN1 is on an f16 kernel in both plans (tests/fast16_stream_cases.py); the sets are asserted equal first."""
    name = "L5_F32to24_x3"
    cfg, weights = _net(oracle, name)
    n, h, w = 1, 17, 33
    x, x2 = synthetic_batch(n, h, w, cfg["scale"], seed=7)
    with _engine(cfg, weights, (("fast16", 1), ("fast16_stream", 1))) as eng:
        assert "feat3_stream" in _kernels(eng), _kernels(eng)
        streamed = S.one_product_set(oracle, cfg, eng.ops(), 1, 1)
        print("FAST16_STREAM streamed plan: %s" % [(o["name"], o["kernel"]) for o in eng.ops()])
        ya = eng.forward(x, x2)
    with _engine(cfg, weights, (("fast16", 1), ("stream_dense", 0))) as eng:
        assert "feat3_stream" not in _kernels(eng), _kernels(eng)
        layered = S.one_product_set(oracle, cfg, eng.ops(), 1, 0)
        print("FAST16_STREAM layer-by-layer plan: %s" % [(o["name"], o["kernel"]) for o in eng.ops()])
        yb = eng.forward(x, x2)
    assert streamed == layered, "the two plans' one-product sets differ: %s" % sorted(streamed ^ layered)
    ref, mod, e_model = M.model_error(oracle, ("stream plan", name, n, h, w), cfg, weights, x, x2, streamed)
    d = M.rms(ya, yb)
    print("FAST16_STREAM %s %dx%dx%d streamed vs layer by layer, both on one product (%d convs): rms of the difference %.4g = %.3f x E_model %.4g | "
          "device rms %.4g (streamed) %.4g (layer by layer) | values that differ %d of %d"
          % (name, n, h, w, len(streamed), d, d / e_model, e_model, M.rms(ya, ref), M.rms(yb, ref), int((ya != yb).sum()), ya.size))
    assert d <= 0.5 * e_model, "rms of the difference %.4g above 0.5 x E_model %.4g" % (d, e_model)


# ---------------------------------------------------------------------------------------------
# 5. determinism and batch independence
# ---------------------------------------------------------------------------------------------
def test_same_bits_twice_alone_and_poisoned(oracle):
    cfg, weights = _net(oracle, "L7_F32to8_x2")
    x, x2 = synthetic_batch(3, 17, 19, cfg["scale"], seed=9)
    with _engine(cfg, weights, (("fast16", 1), ("fast16_stream", 1))) as eng:
        assert "feat3_stream" in _kernels(eng)
        y = eng.forward(x, x2)
        assert _same(eng.forward(x, x2), y)
        for i in range(3):
            assert _same(eng.forward(x[i:i + 1], x2[i:i + 1])[0], y[i]), "image %d alone differs from the one in the batch" % i
        eng.set_option("debug_poison", 3)
        assert _same(eng.forward(x, x2), y), "the output depends on what LDS or registers held before the launch"
        eng.set_option("debug_poison", 0)
        eng.set_option("fast16_stream", 0)
        assert not _same(eng.forward(x, x2), y)


# ---------------------------------------------------------------------------------------------
# 6. overflow inside the streamed launch
# ---------------------------------------------------------------------------------------------
OVERFLOW = [("L7_F32to8_x2", C.SHAPE_A, "CNN4"), ("L7_F32to8_x2", C.SHAPE_A, "B1")]


@pytest.mark.parametrize("net,shape,target", OVERFLOW, ids=["%s-%s" % (c[0], c[2]) for c in OVERFLOW])
def test_flagged_image_takes_the_float32_plan_and_bystanders_keep_their_bits(oracle, net, shape, target):
    assert (net, shape, target, True) in C.cases_a(dcscn_oracle, CONFIGS)
    case = C.directed_case(dcscn_oracle, CONFIGS, net, shape, target)
    i, n = case.i, case.x.shape[0]
    rest = [j for j in range(n) if j != i]
    with _engine(case.cfg, case.weights, (("fast16_stream", 1),)) as eng:
        assert target in S.streamed_set(dcscn_oracle, case.cfg, eng.ops()), eng.ops()[0]
        assert C.flag_expected(dcscn_oracle, case.cfg, eng.ops(), target) in (True, None)
        y = eng.forward(case.xb, case.x2)
        without = eng.forward(np.ascontiguousarray(case.xb[rest]), np.ascontiguousarray(case.x2[rest]))
        eng.set_option("fast16_stream", 0)
        three = eng.forward(np.ascontiguousarray(case.xb[rest]), np.ascontiguousarray(case.x2[rest]))
        eng.set_option("fast16_stream", 1)
        eng.set_option("split16", 0)
        y32 = eng.forward(case.xb, case.x2)
    assert np.isfinite(y).all()
    assert _same(y[i], y32[i]), "the flagged image differs from its split16 = 0 run in %d values" % int((y[i] != y32[i]).sum())
    for k, j in enumerate(rest):
        assert _same(y[j], without[k]), "bystander %d differs from the fast16_stream run without the flagged image in %d values" % (j, int((y[j] != without[k]).sum()))
    assert not _same(without, three), "the bystanders carry three-product bits"


# ---------------------------------------------------------------------------------------------
# 7. trained weights and the flags
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast16", [0, 1], ids=["stream_alone", "both_on"])
def test_trained_weights_error_band(oracle, fast16):
    cfg, weights, lr, bic, _ = golden_crop(oracle)
    with _engine(cfg, weights) as eng:
        assert "feat3_stream" in _kernels(eng), _kernels(eng)
        label = "c-DCSCN x2 trained weights, golden crop, default plan"
        y1, y0, off, rms, mx, e_model = _measure(oracle, label, eng, cfg, weights, lr, bic, ("golden crop",), fast16)
    assert not _same(y1, y0) and not _same(y1, off)
    assert 0.5 * e_model <= rms <= 2.0 * e_model, "%s: device rms %.4g outside [0.5, 2] x E_model %.4g" % (label, rms, e_model)


def _model(tmp_path, on):
    """SuperResolution from flags on the golden c-DCSCN x2 weights, default plan."""
    import json
    from dcscn_amd.model import SuperResolution
    with open(os.path.join(GOLDEN, "goldens.json")) as f:
        flags = dict(json.load(f)["models"]["L7_x2"]["flags"])
    flags.update(checkpoint_dir=str(tmp_path / "models"), self_ensemble=1, fast16=on, fast16_stream=on)
    m = SuperResolution(_flags(**flags))
    m.build_graph()
    m.init_all_variables()
    m.load_weights(dict(np.load(os.path.join(GOLDEN, "weights_L7_x2.npz"))))
    assert "feat3_stream" in _kernels(m._engine)
    return m


def test_both_flags_through_the_model(oracle, tmp_path):
    cfg, weights, lr, bic, truth = golden_crop(oracle)
    outs = {}
    for on in (False, True):
        m = _model(tmp_path, on)
        try:
            assert m.fast16 is on and m.fast16_stream is on
            outs[on] = np.asarray(m.do(lr[0], bic[0]), np.float64)
            selected = S.one_product_set(oracle, cfg, m._engine.ops(), 1, 1)
        finally:
            m.close()
    _, _, e_model = M.model_error(oracle, ("golden crop",), cfg, weights, lr, bic, selected)
    assert outs[False].shape == truth.shape and not _same(outs[True], outs[False])
    mse = {k: float(np.mean((v - truth) ** 2)) for k, v in outs.items()}
    psnr = {k: 10.0 * np.log10(255.0 ** 2 / v) for k, v in mse.items()}
    delta = psnr[True] - psnr[False]
    bound = psnr_delta_bound(e_model, mse[False])
    print("FAST16_STREAM model path, golden crop: PSNR %.6f dB (fast16 + fast16_stream) vs %.6f dB, delta %+.3g dB, bound %.3g dB, rms between the two %.4g, E_model %.4g"
          % (psnr[True], psnr[False], delta, bound, M.rms(outs[True], outs[False]), e_model))
    assert abs(delta) <= bound
