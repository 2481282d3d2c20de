"""Option "fast16" (include/dcscn.h) on the device, through the C ABI: every launch on conv3_h, conv3_h8, conv_nin_h or conv5_h takes ONE
f16 product per multiply-accumulate (wh * xh) instead of split16's three.

What is asserted, and against what:
1. off means off: fast16 = 0, fast16 = 1 under split16 = 0, and 1 -> 0 toggles (plain launches and replayed graphs) give the default bits;
2. it is on, and only as wrong as it should be: the device's rms error against the float64 oracle lies in [0.5, 2] x E_model, the rms
   error of the CPU restatement tests/fast16_model.py on the same input and the same set of layers (Engine.ops()); max-abs <= 8 x E_model.
   The band is derived, not tuned: accumulating in float32 per 32-deep block as the instruction does moves the restatement's rms by under
   2 %, rounding flips move single pixels; the factor 2 is slack for the edges of the eligible set.  The LOWER bound is what proves the lo
   products are gone: with them the rms error is about 1e-6.  The restatement's own max / rms ratio is about 4 (tests/test_fast16_host.py);
3. default plans (folded tails, whole-tail fold, one-tile layers): rms <= 2 x E_model only -- the fold rounds COMPOSED kernels, the
   restatement the layers they replace;
4. two runs give the same bits; an image alone gives the bits it has in a batch of three;
5. overflow (the cases of tests/overflow_cases.py): the flagged image has the bits of its split16 = 0 run, bystanders those of a
   fast16 run without it;
6. the shipped c-DCSCN x2 weights on the golden crop: the band of 2, and through SuperResolution(--fast16) a PSNR against the ground
   truth within 20 log10(1 + 2 E_model / sqrt(MSE)) of the default's (triangle inequality on the band).

Measured on an MI355X (profiles/r11_fast16_numerics.txt): device rms / E_model 1.002 (1 x 19 x 35) and 0.989
(3 x 7 x 9) in test 2, the same bits for all eight option combinations; 0.38 .. 1.28 in test 3 (folded tails below the restatement, which
rounds a depth_to_space map the launch never forms; 1 x 1 images are 4 .. 16 samples); 0.533 in test 6, whose plan keeps the folded tail
(device 1.52e-3 rms, 1.33e-2 max-abs against E_model 2.85e-3), PSNR delta -1.6e-5 dB against a bound of 9.6e-3 dB."""
import os

import numpy as np
import pytest

import dcscn_oracle
import fast16_model as M
import overflow_cases as C
import test_hip_parity as P
from conftest import CONFIGS, GOLDEN, synthetic_batch
from test_fast16_host import golden_crop, psnr_delta_bound
from test_host import _flags

pytestmark = pytest.mark.gpu

_NETS = {}


def _net(oracle, name):
    if name not in _NETS:
        cfg = oracle.make_config(**CONFIGS[name])
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


def _measure(oracle, label, eng, cfg, weights, x, x2, key):
    """(y of fast16 = 1, y of fast16 = 0, rms and max-abs error of the former against the float64 oracle, E_model); prints the figures."""
    selected = M.selected_by_ops(oracle, cfg, eng.ops())
    assert selected, _kernels(eng)
    ref, mod, e_model = M.model_error(oracle, key, cfg, weights, x, x2, selected)
    eng.set_option("fast16", 1)
    y1 = eng.forward(x, x2)
    eng.set_option("fast16", 0)
    y0 = eng.forward(x, x2)
    rms, mx = M.rms(y1, ref), M.max_abs(y1, ref)
    print("FAST16 %s | device rms %.4g max-abs %.4g | E_model %.4g (max-abs %.4g) | rms / E_model %.3f | fast16 0: rms %.3g | %d layers on one product"
          % (label, rms, mx, e_model, M.max_abs(mod, ref), rms / e_model if e_model else float("nan"), M.rms(y0, ref), len(selected)))
    assert np.isfinite(y1).all()
    return y1, y0, rms, mx, e_model


# ---------------------------------------------------------------------------------------------
# 1. off means off
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["L12_F196to48_x2", "L7_F32to8_x4"])
def test_off_means_off(oracle, name):
    cfg, weights = _net(oracle, name)
    n, h, w = 2, 19, 35
    x, x2 = synthetic_batch(n, h, w, cfg["scale"], seed=21)
    with _engine(cfg, weights) as eng:                             # a handle that never hears of the option
        default = eng.forward(x, x2)
    hip = P._Hip()
    try:
        with _engine(cfg, weights) as eng:
            eng.set_option("fast16", 0)
            assert _same(eng.forward(x, x2), default)
            eng.set_option("split16", 0)
            y32 = eng.forward(x, x2)
            eng.set_option("fast16", 1)
            assert _same(eng.forward(x, x2), y32), "fast16 = 1 under split16 = 0 is not the split16 = 0 forward"
            eng.set_option("split16", 1)
            y1 = eng.forward(x, x2)
            assert not _same(y1, default), "fast16 = 1 changed nothing"
            eng.set_option("fast16", 0)
            assert _same(eng.forward(x, x2), default), "1 -> 0 does not give the default bits"
            # the same toggles through replayed graphs: every call repeated so that the capture (second call) and a replay (third) happen
            dx, dx2, dy, st = hip.upload(x), hip.upload(x2), hip.alloc(default.nbytes), hip.stream()
            eng.set_option("graph_replay", 1)
            for value, want in ((1, y1), (0, default), (1, y1), (0, default)):
                eng.set_option("fast16", value)
                for call in range(3):
                    eng.forward_device(dx, dx2, dy, n, h, w, stream=st)
                    eng.synchronize()
                    assert _same(hip.download(dy, default.shape), want), "graph_replay, fast16 = %d, call %d" % (value, call)
    finally:
        hip.close()


# ---------------------------------------------------------------------------------------------
# 2. it is on, and only as wrong as it should be
# ---------------------------------------------------------------------------------------------
BAND_SHAPES = [(1, 19, 35), (3, 7, 9)]


def _band(label, y1, y0, rms, mx, e_model):
    assert not _same(y1, y0), "%s: fast16 = 1 gives the fast16 = 0 output" % label
    assert 0.5 * e_model <= rms <= 2.0 * e_model, "%s: device rms %.4g outside [0.5, 2] x E_model %.4g" % (label, rms, e_model)
    assert mx <= 8.0 * e_model, "%s: device max-abs %.4g above 8 x E_model %.4g" % (label, mx, e_model)


@pytest.mark.parametrize("nin_h8", [0, 1])
@pytest.mark.parametrize("h8", [0, 1])
@pytest.mark.parametrize("p16", [0, 1])
@pytest.mark.parametrize("shape", BAND_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_one_product_error_band(oracle, shape, p16, h8, nin_h8):
    """L12 x2, layer by layer (fold_linear_tail = 0): packed tails of 1, 2 and 3 octets, a chunk with no tail, two-group layers on
    conv3_h8 (or conv3_h), the 1301-channel GEMM on either workgroup size."""
    cfg, weights = _net(oracle, "L12_F196to48_x2")
    n, h, w = shape
    x, x2 = synthetic_batch(n, h, w, cfg["scale"], seed=5)
    with _engine(cfg, weights, (("fold_linear_tail", 0), ("p16", p16), ("conv3_h8", h8), ("nin_h8", nin_h8))) as eng:
        kernels = _kernels(eng)
        assert "conv3_h" in kernels and "conv_nin_h" in kernels and ("conv3_h8" in kernels) == bool(h8) and "conv5_h" not in kernels, kernels
        label = "L12 x2 unfolded %dx%dx%d p16 %d conv3_h8 %d nin_h8 %d" % (n, h, w, p16, h8, nin_h8)
        _band(label, *_measure(oracle, label, eng, cfg, weights, x, x2, ("band",) + shape))


# ---------------------------------------------------------------------------------------------
# 3. default plans
# ---------------------------------------------------------------------------------------------
DEFAULT_PLANS = [("L12_F196to48_x2", (), "conv5_h"), ("L12_F196to48_x4", (), "conv5_h"), ("L8_F96to48_x2", (), "conv5_h"),
                 ("L7_F32to8_x3", (("stream_dense", 0),), "conv3_h")]


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 17, 33)], ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("name,options,kernel", DEFAULT_PLANS, ids=[p[0] for p in DEFAULT_PLANS])
def test_default_plans_stay_within_twice_the_model(oracle, name, options, kernel, shape):
    cfg, weights = _net(oracle, name)
    n, h, w = shape
    x, x2 = synthetic_batch(n, h, w, cfg["scale"], seed=7)
    with _engine(cfg, weights, options) as eng:
        kernels = _kernels(eng)
        assert kernel in kernels and ("feat3_stream" not in kernels or not options), kernels
        label = "%s default plan %dx%dx%d" % (name, n, h, w)
        y1, y0, rms, mx, e_model = _measure(oracle, label, eng, cfg, weights, x, x2, ("plan", name) + shape)
    assert not _same(y1, y0), "%s: fast16 = 1 gives the fast16 = 0 output" % label
    assert rms <= 2.0 * e_model, "%s: device rms %.4g above 2 x E_model %.4g" % (label, rms, e_model)


# ---------------------------------------------------------------------------------------------
# 4. determinism and batch independence
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["L12_F196to48_x2", "L12_F196to48_x4"])
def test_same_bits_twice_and_alone(oracle, name):
    """17 x 19: 323 pixels per image, so the 128- and 256-pixel blocks of the GEMM straddle images; x4: the corner jobs of fold_border
    take the same corner of up to 16 images."""
    cfg, weights = _net(oracle, name)
    x, x2 = synthetic_batch(3, 17, 19, cfg["scale"], seed=9)
    with _engine(cfg, weights, (("fast16", 1),)) as eng:
        y = eng.forward(x, x2)
        assert _same(eng.forward(x, x2), y)
        for i in range(3):
            assert _same(eng.forward(x[i:i + 1], x2[i:i + 1])[0], y[i]), "image %d alone differs from the one in the batch" % i
        eng.set_option("fast16", 0)
        assert not _same(eng.forward(x, x2), y)


# ---------------------------------------------------------------------------------------------
# 5. overflow
# ---------------------------------------------------------------------------------------------
OVERFLOW = [("L12_F196to48_x2", C.SHAPE_A, "CNN2"), ("L12_F196to48_x2", C.SHAPE_A, "CNN9"), ("L12_F196to48_x2", C.SHAPE_A, "A1"),
            ("L12_F196to48_x4", C.SHAPE_A, "B2")]


@pytest.mark.parametrize("net,shape,target", OVERFLOW, ids=["%s-%s" % (c[0], c[2]) for c in OVERFLOW])
def test_flagged_image_takes_the_float32_plan_and_bystanders_keep_their_bits(oracle, net, shape, target):
    assert (net, shape, target, True) in C.cases_a(dcscn_oracle, CONFIGS)
    case = C.directed_case(dcscn_oracle, CONFIGS, net, shape, target)
    i, n = case.i, case.x.shape[0]
    rest = [j for j in range(n) if j != i]
    with _engine(case.cfg, case.weights, (("fast16", 1),)) as eng:
        assert C.flag_expected(dcscn_oracle, case.cfg, eng.ops(), target) in (True, None)
        y = eng.forward(case.xb, case.x2)
        without = eng.forward(np.ascontiguousarray(case.xb[rest]), np.ascontiguousarray(case.x2[rest]))
        eng.set_option("fast16", 0)
        three = eng.forward(np.ascontiguousarray(case.xb[rest]), np.ascontiguousarray(case.x2[rest]))
        eng.set_option("fast16", 1)
        eng.set_option("split16", 0)
        y32 = eng.forward(case.xb, case.x2)
    assert np.isfinite(y).all()
    assert _same(y[i], y32[i]), "the flagged image differs from its split16 = 0 run in %d values" % int((y[i] != y32[i]).sum())
    for k, j in enumerate(rest):
        assert _same(y[j], without[k]), "bystander %d differs from the fast16 run without the flagged image in %d values" % (j, int((y[j] != without[k]).sum()))
    assert not _same(without, three), "the bystanders carry three-product bits"


# ---------------------------------------------------------------------------------------------
# 6. trained weights and the flag
# ---------------------------------------------------------------------------------------------
def test_trained_weights_error_band(oracle):
    cfg, weights, lr, bic, _ = golden_crop(oracle)
    with _engine(cfg, weights, (("stream_dense", 0),)) as eng:
        kernels = _kernels(eng)
        assert "feat3_stream" not in kernels and "conv3_h" in kernels, kernels
        label = "c-DCSCN x2 trained weights, golden crop, stream_dense 0"
        _band(label, *_measure(oracle, label, eng, cfg, weights, lr, bic, ("golden crop",)))


def _model(tmp_path, fast16):
    """SuperResolution from flags on the golden c-DCSCN x2 weights, layer by layer (stream_dense = 0) like the test above."""
    import json
    from dcscn_amd.model import SuperResolution
    with open(os.path.join(GOLDEN, "goldens.json")) as f:
        flags = dict(json.load(f)["models"]["L7_x2"]["flags"])
    flags.update(checkpoint_dir=str(tmp_path / "models"), self_ensemble=1, fast16=fast16)
    m = SuperResolution(_flags(**flags))
    m.build_graph()
    m._engine.set_option("stream_dense", 0)
    m.init_all_variables()
    m.load_weights(dict(np.load(os.path.join(GOLDEN, "weights_L7_x2.npz"))))
    assert "feat3_stream" not in _kernels(m._engine)
    return m


def test_fast16_flag_through_the_model(oracle, tmp_path):
    cfg, weights, lr, bic, truth = golden_crop(oracle)
    outs = {}
    for fast16 in (False, True):
        m = _model(tmp_path, fast16)
        try:
            assert m.fast16 is fast16
            outs[fast16] = np.asarray(m.do(lr[0], bic[0]), np.float64)
            selected = M.selected_by_ops(oracle, cfg, m._engine.ops())
        finally:
            m.close()
    _, _, e_model = M.model_error(oracle, ("golden crop",), cfg, weights, lr, bic, selected)
    assert outs[False].shape == truth.shape and not _same(outs[True], outs[False])
    mse = {k: float(np.mean((v - truth) ** 2)) for k, v in outs.items()}
    psnr = {k: 10.0 * np.log10(255.0 ** 2 / v) for k, v in mse.items()}
    delta = psnr[True] - psnr[False]
    bound = psnr_delta_bound(e_model, mse[False])
    print("FAST16 model path, golden crop: PSNR %.6f dB (fast16) vs %.6f dB, delta %+.3g dB, bound %.3g dB, rms between the two %.4g, E_model %.4g"
          % (psnr[True], psnr[False], delta, bound, M.rms(outs[True], outs[False]), e_model))
    assert abs(delta) <= bound
