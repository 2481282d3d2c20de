"""Option "fast16_separable" (include/dcscn.h) on the device, through the C ABI: every MFMA contraction of a feat_stream or tail_stream
launch of the depthwise-separable narrow nets (the pointwise stage of CNN2 .. CNNL and B2, A1 || B1, Up-PS, Up-PS2) takes ONE f16 product
per multiply-accumulate (wh * xh) instead of split16's three.  Independent of "fast16" (the layer kernels) and "fast16_stream" (feat3_stream).

What is asserted, and against what (the bars are those derived in tests/test_fast16_hip.py; E_model is the rms error of the CPU restatement
tests/fast16_separable_model.py on the same input and the same set of convs; every band runs on the bare branch -- x2 = 0, the last conv
not attenuated -- or on trained weights, where E_model is 250 .. 3300 x the float32 floor: tests/test_fast16_separable_host.py):
1. off means off, on C5 in its three plans (feat_stream + conv5_h, feat_stream + tail_stream, layer by layer): a handle that never hears
   of the option, option = 0 and a 1 -> 0 toggle give the same bits, by plain launches and under graph_replay; option = 1 under
   split16 = 0, on the layer-by-layer plan, on c-DCSCN x2 and on the STREAM_VARIANTS entries that do not stream changes nothing; fast16 = 1
   and fast16_stream = 1 beside option = 0 give the bits they give without it;
2. it is on, and only as wrong as it should be: device rms against the float64 oracle in [0.5, 2] x E_model, max-abs <= 8 x E_model, output
   differs from the option-off output (the LOWER bound proves the lo products are gone: with them the error is at the 1e-7-relative
   floor) -- C5 on four shapes, every streaming STREAM_VARIANTS net and the net that reaches stream_conv_role<8, 1> on one;
3. tail_stream on its own (stream_features = 0, fold_whole_tail = 0: the set is {Up-PS, Up-PS2}), then feat_stream + tail_stream on the union;
4. with fast16 on C5's default plan: rms <= 2 x E_model of the union (the fold modelled as the layers it replaces), output differs from
   (1, 0) and from (0, 1);
5. two runs give the same bits, an image alone the bits it has in a batch of three, debug_poison = 3 the same bits again;
6. overflow (the middle image x 4000): the flagged image has the bits of its split16 = 0 run, bystanders those of an option-on run
   without it, which are not the option-off bits; the next clean forward has the clean option-on bits;
7. the trained DS weights on a 48 x 48 LR crop with its bicubic x2, default plan: the band of 2 on the rms with the option alone and with
   fast16, no max-abs condition; through SuperResolution(--fast16 --fast16_separable) a PSNR against the ground truth within
   20 log10(1 + 2 E_model / sqrt(MSE)) of the default's.

Measured on an MI355X: profiles/r18_fast16_separable_numerics.txt, DESIGN.md section 3.13."""
import os

import numpy as np
import pytest

import dcscn_oracle
import fast16_model as M
import fast16_separable_model as F
import test_hip_parity as P
from conftest import CONFIGS, GOLDEN, synthetic_batch
from test_fast16_host import psnr_delta_bound
from test_host import _flags

pytestmark = pytest.mark.gpu

STREAMING = F.streaming(dcscn_oracle, P.STREAM_VARIANTS) + F.EXTRA_VARIANTS
NOT_STREAMING = [v for v in P.STREAM_VARIANTS if not F.streams(dcscn_oracle, v)]
_vid = lambda v: "L%d_F%dto%d_x%d" % (v[0], v[1], v[2], v[6])
_sid = lambda s: "%dx%dx%d" % s

# C5's three plans: options set before the weights are loaded, and the kernel list each must show
PLANS = {
    "default": ((), ["feat_stream", "conv5_h"]),
    "tail_stream": ((("fold_whole_tail", 0),), ["feat_stream", "tail_stream"]),
    "layer_by_layer": ((("stream_features", 0), ("stream_tail", 0)), None),
}
TAIL_ALONE = (("stream_features", 0), ("stream_tail", 1), ("fold_whole_tail", 0))


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


def _streamed(eng):
    return [k for k in _kernels(eng) if k in F.STREAM_KERNELS]


def _set(eng, fast16, separable):
    eng.set_option("fast16", fast16)
    eng.set_option("fast16_separable", separable)


def _measure(oracle, label, eng, cfg, weights, x, x2, key, fast16):
    """(y of (fast16, 1), y of (fast16, 0), y of (0, 0), rms and max-abs error of the first against the float64 oracle, E_model of the
    one-product set of (fast16, 1)); prints the figures."""
    selected, separable = F.one_product_set(oracle, cfg, eng.ops(), fast16, 1)
    assert separable and separable == F.streamed_set(oracle, cfg, eng.ops()), _kernels(eng)
    ref, mod, e_model = F.model_error(oracle, key, cfg, weights, x, x2, selected, separable)
    _set(eng, fast16, 1)
    y1 = eng.forward(x, x2)
    _set(eng, fast16, 0)
    y0 = eng.forward(x, x2)
    _set(eng, 0, 0)
    off = eng.forward(x, x2)
    rms, mx, scale = M.rms(y1, ref), M.max_abs(y1, ref), float(np.abs(ref).max())
    print("FAST16_SEPARABLE %s | %s | fast16 %d fast16_separable 1 | output scale %.4g | device rms %.4g max-abs %.4g | E_model %.4g (max-abs %.4g) | "
          "rms / E_model %.3f | max-abs / E_model %.2f | (%d, 0): rms %.3g | (0, 0): rms %.3g | %d convs on one product"
          % (label, "+".join(_kernels(eng)), fast16, scale, rms, mx, e_model, M.max_abs(mod, ref), rms / e_model if e_model else float("nan"),
             mx / e_model if e_model else float("nan"), fast16, M.rms(y0, ref), M.rms(off, ref), len(selected)))
    assert np.isfinite(y1).all()
    return y1, y0, off, rms, mx, e_model


def _band(label, y1, y0, off, rms, mx, e_model, max_abs=True):
    assert not _same(y1, off), "%s: the option-off output" % label
    assert not _same(y1, y0), "%s: fast16_separable = 1 gives the fast16_separable = 0 output" % label
    assert 0.5 * e_model <= rms <= 2.0 * e_model, "%s: device rms %.4g outside [0.5, 2] x E_model %.4g" % (label, rms, e_model)
    if max_abs:
        assert mx <= 8.0 * e_model, "%s: device max-abs %.4g above 8 x E_model %.4g" % (label, mx, e_model)


def _c5_input(cfg, shape):
    n, h, w = shape
    return F.bare_input(n, h, w, cfg["scale"], seed=h + w)


# ---------------------------------------------------------------------------------------------
# 1. off means off
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", sorted(PLANS))
def test_off_means_off(oracle, plan):
    cfg, weights = F.c5(oracle)
    options, kernels = PLANS[plan]
    streamed = kernels is not None
    n, h, w = F.SHAPES[0]
    x, x2 = _c5_input(cfg, F.SHAPES[0])

    def check_plan(eng):
        if streamed:
            assert _kernels(eng) == kernels, _kernels(eng)
        else:
            assert not _streamed(eng) and len(_kernels(eng)) > 2, _kernels(eng)

    with _engine(cfg, weights, options) as eng:                    # handles that never hear of the option
        check_plan(eng)
        default = eng.forward(x, x2)
    with _engine(cfg, weights, options + (("fast16", 1),)) as eng:
        fast = eng.forward(x, x2)
    with _engine(cfg, weights, options + (("fast16_stream", 1),)) as eng:
        fstream = eng.forward(x, x2)
    hip = P._Hip()
    try:
        with _engine(cfg, weights, options) as eng:
            eng.set_option("fast16_separable", 0)
            assert _same(eng.forward(x, x2), default)
            eng.set_option("split16", 0)
            assert "feat_stream" in _kernels(eng) if streamed else not _streamed(eng), _kernels(eng)      # (one name for the float32 instantiation)
            y32 = eng.forward(x, x2)
            eng.set_option("fast16_separable", 1)
            assert _same(eng.forward(x, x2), y32), "fast16_separable = 1 under split16 = 0 is not the split16 = 0 forward"
            eng.set_option("split16", 1)
            check_plan(eng)
            y1 = eng.forward(x, x2)
            if streamed:
                assert not _same(y1, default), "fast16_separable = 1 changed nothing"
            else:
                assert _same(y1, default), "fast16_separable = 1 changed the layer-by-layer plan's bits"
            eng.set_option("fast16_separable", 0)
            assert _same(eng.forward(x, x2), default), "1 -> 0 does not give the default bits"
            # beside the other two options: the bits of handles that only ever set those
            eng.set_option("fast16", 1)
            assert _same(eng.forward(x, x2), fast), "fast16 = 1, fast16_separable = 0 is not the fast16 = 1 forward"
            eng.set_option("fast16_separable", 1)
            assert _same(eng.forward(x, x2), fast) == (not streamed)
            eng.set_option("fast16_separable", 0)
            assert _same(eng.forward(x, x2), fast), "fast16 = 1: 1 -> 0 does not give the fast16 = 1 bits"
            eng.set_option("fast16", 0)
            eng.set_option("fast16_stream", 1)
            assert _same(eng.forward(x, x2), fstream), "fast16_stream = 1, fast16_separable = 0 is not the fast16_stream = 1 forward"
            eng.set_option("fast16_stream", 0)
            # the same toggles through replayed graphs: every call repeated so that the capture (second call) and a replay (third) happen
            dx, dx2, dy, st = hip.upload(x), hip.upload(x2), hip.alloc(default.nbytes), hip.stream()
            eng.set_option("graph_replay", 1)
            for value, want in ((1, y1), (0, default), (1, y1), (0, default)):
                eng.set_option("fast16_separable", value)
                for call in range(3):
                    eng.forward_device(dx, dx2, dy, n, h, w, stream=st)
                    eng.synchronize()
                    assert _same(hip.download(dy, default.shape), want), "graph_replay, fast16_separable = %d, call %d" % (value, call)
    finally:
        hip.close()


def test_option_is_ignored_on_a_non_separable_net(oracle):
    cfg = oracle.make_config(**CONFIGS["L7_F32to8_x2"])
    weights = oracle.synthetic_weights(cfg, seed=0)
    x, x2 = synthetic_batch(2, 19, 35, cfg["scale"], seed=21)
    with _engine(cfg, weights) as eng:
        assert not _streamed(eng) and "feat3_stream" in _kernels(eng), _kernels(eng)
        default = eng.forward(x, x2)
        eng.set_option("fast16_separable", 1)
        assert _same(eng.forward(x, x2), default), "fast16_separable = 1 changed c-DCSCN x2"


@pytest.mark.parametrize("v", NOT_STREAMING, ids=_vid)
def test_option_is_ignored_on_separable_nets_that_do_not_stream(oracle, v):
    """The (4, 20, 16, ...) entry of STREAM_VARIANTS (it would need stream_conv_role<5, 2>) and the two with a 6-quad layer of one output
    tile: depthwise / conv_igemm launches, which the option does not govern."""
    assert (4, 20, 16, 1.0, 16, 16, 2, "prelu") in NOT_STREAMING
    cfg, weights = F.variant(oracle, v)
    n, h, w = F.VARIANT_SHAPE
    x, x2 = F.bare_input(n, h, w, cfg["scale"], seed=5)
    with _engine(cfg, weights) as eng:
        assert "feat_stream" not in _kernels(eng), _kernels(eng)
        default = eng.forward(x, x2)
        eng.set_option("fast16_separable", 1)
        if "tail_stream" not in _kernels(eng):
            assert _same(eng.forward(x, x2), default), "fast16_separable = 1 changed a net without a streamed launch"
        else:                                                      # (an x4 net keeps its streamed tail: that launch the option does govern)
            assert not _same(eng.forward(x, x2), default)


# ---------------------------------------------------------------------------------------------
# 2. it is on, and only as wrong as it should be
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", F.SHAPES, ids=_sid)
def test_one_product_error_band_c5(oracle, shape):
    cfg, weights = F.c5(oracle)
    x, x2 = _c5_input(cfg, shape)
    with _engine(cfg, weights) as eng:
        assert _kernels(eng) == PLANS["default"][1], _kernels(eng)
        assert F.streamed_set(oracle, cfg, eng.ops()) == F.FEAT_SET_C5
        label = "C5 bare %dx%dx%d" % shape
        _band(label, *_measure(oracle, label, eng, cfg, weights, x, x2, ("c5 bare",) + shape, 0))


@pytest.mark.parametrize("v", STREAMING, ids=_vid)
def test_one_product_error_band_variants(oracle, v):
    cfg, weights = F.variant(oracle, v)
    n, h, w = F.VARIANT_SHAPE
    x, x2 = F.bare_input(n, h, w, cfg["scale"], seed=5)
    # (an x4 variant's tail would stream too: kept layer by layer here, so that the set is feat_stream's, as on the host)
    with _engine(cfg, weights, (("stream_tail", 0),)) as eng:
        assert _streamed(eng) == ["feat_stream"] and eng.ops()[0]["name"] == "CNN1..B2 (streamed)", _kernels(eng)
        label = "variant %s bare %dx%dx%d" % ((v,) + F.VARIANT_SHAPE)
        _band(label, *_measure(oracle, label, eng, cfg, weights, x, x2, ("variant", v), 0))


# ---------------------------------------------------------------------------------------------
# 3. tail_stream on its own, then both streamed launches
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", F.TAIL_SHAPES, ids=_sid)
def test_tail_stream_alone_and_with_feat_stream(oracle, shape):
    """Without the first plan a tail_stream left on three products would hide inside feat_stream's error."""
    cfg, weights = F.c5(oracle)
    x, x2 = _c5_input(cfg, shape)
    key = ("c5 bare",) + shape
    with _engine(cfg, weights, TAIL_ALONE) as eng:
        assert _kernels(eng)[-1] == "tail_stream" and "feat_stream" not in _kernels(eng), _kernels(eng)
        assert F.streamed_set(oracle, cfg, eng.ops()) == F.TAIL_SET_C5
        label = "C5 bare tail_stream alone %dx%dx%d" % shape
        tail_on, _, tail_off, rms, mx, e_model = _measure(oracle, label, eng, cfg, weights, x, x2, key, 0)
        _band(label, tail_on, tail_off, tail_off, rms, mx, e_model)
    with _engine(cfg, weights, PLANS["tail_stream"][0]) as eng:
        assert _kernels(eng) == PLANS["tail_stream"][1], _kernels(eng)
        assert F.streamed_set(oracle, cfg, eng.ops()) == F.FEAT_SET_C5 | F.TAIL_SET_C5
        label = "C5 bare feat_stream + tail_stream %dx%dx%d" % shape
        both_on, _, both_off, rms, mx, e_model = _measure(oracle, label, eng, cfg, weights, x, x2, key, 0)
        _band(label, both_on, both_off, both_off, rms, mx, e_model)
    with _engine(cfg, weights, (("fast16_separable", 1),)) as eng:     # the default plan: feat_stream alone on one product
        assert _kernels(eng) == PLANS["default"][1]
        feat_on = eng.forward(x, x2)
    for other, what in ((tail_off, "tail_stream-alone plan, option off"), (tail_on, "tail_stream alone on one product"),
                        (feat_on, "feat_stream alone on one product")):
        assert not _same(both_on, other), "feat_stream + tail_stream on one product gives the output of: %s" % what


# ---------------------------------------------------------------------------------------------
# 4. with fast16
# ---------------------------------------------------------------------------------------------
def test_with_fast16_on_the_default_plan(oracle):
    cfg, weights = F.c5(oracle)
    shape = F.SHAPES[0]
    x, x2 = _c5_input(cfg, shape)
    with _engine(cfg, weights) as eng:
        assert _kernels(eng) == PLANS["default"][1], _kernels(eng)
        assert F.one_product_set(oracle, cfg, eng.ops(), 1, 1) == (F.FEAT_SET_C5 | F.FOLD_SET_C5, F.FEAT_SET_C5)
        label = "C5 bare default plan %dx%dx%d" % shape
        y11, y10, off, rms, mx, e_model = _measure(oracle, label, eng, cfg, weights, x, x2, ("c5 bare",) + shape, 1)
        _set(eng, 0, 1)
        y01 = eng.forward(x, x2)
    assert not _same(y11, y10), "(1, 1) gives the (1, 0) output"
    assert not _same(y11, y01), "(1, 1) gives the (0, 1) output"
    assert not _same(y11, off)
    assert rms <= 2.0 * e_model, "%s: device rms %.4g above 2 x E_model %.4g" % (label, rms, e_model)


# ---------------------------------------------------------------------------------------------
# 5. determinism and batch independence
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", ["default", "tail_stream"])
def test_same_bits_twice_alone_and_poisoned(oracle, plan):
    cfg, weights = F.c5(oracle)
    x, x2 = F.bare_input(3, 17, 19, cfg["scale"], seed=9)
    with _engine(cfg, weights, PLANS[plan][0] + (("fast16_separable", 1),)) as eng:
        assert _kernels(eng) == PLANS[plan][1], _kernels(eng)
        y = eng.forward(x, x2)
        assert _same(eng.forward(x, x2), y)
        for i in range(3):
            assert _same(eng.forward(x[i:i + 1], x2[i:i + 1])[0], y[i]), "image %d alone differs from the one in the batch" % i
        eng.set_option("debug_poison", 3)
        assert _same(eng.forward(x, x2), y), "the output depends on what LDS or registers held before the launch"
        eng.set_option("debug_poison", 0)
        eng.set_option("fast16_separable", 0)
        assert not _same(eng.forward(x, x2), y)


# ---------------------------------------------------------------------------------------------
# 6. overflow
# ---------------------------------------------------------------------------------------------
def test_flagged_image_takes_the_float32_plan_and_bystanders_keep_their_bits(oracle):
    """Set up as test_hip_parity.test_whole_tail_fold_flagged_image_takes_the_float32_plan sets it up for L7_F32to8_x4_DS."""
    cfg = oracle.make_config(**CONFIGS[F.C5])
    weights = oracle.synthetic_weights(cfg, seed=9)
    x, x2 = synthetic_batch(3, 21, 50, cfg["scale"], seed=10)
    xb = x.copy()
    xb[1] *= 4000.0
    rest = [0, 2]
    with _engine(cfg, weights, (("fast16_separable", 1),)) as eng:
        assert _kernels(eng) == PLANS["default"][1], _kernels(eng)
        clean = eng.forward(x, x2)
        y = eng.forward(xb, x2)
        again = eng.forward(x, x2)
        without = eng.forward(np.ascontiguousarray(xb[rest]), np.ascontiguousarray(x2[rest]))
        eng.set_option("fast16_separable", 0)
        three = eng.forward(np.ascontiguousarray(xb[rest]), np.ascontiguousarray(x2[rest]))
        eng.set_option("fast16_separable", 1)
        eng.set_option("split16", 0)
        y32 = eng.forward(xb, x2)
    assert np.isfinite(y).all()
    assert _same(y[1], y32[1]), "the flagged image differs from its split16 = 0 run in %d values" % int((y[1] != y32[1]).sum())
    for k, j in enumerate(rest):
        assert _same(y[j], without[k]), "bystander %d differs from the option-on run without the flagged image in %d values" % (j, int((y[j] != without[k]).sum()))
        assert _same(y[j], clean[j])
    assert not _same(without, three), "the bystanders carry three-product bits"
    assert _same(again, clean), "the forward after the flagged one does not have the clean option-on bits"


# ---------------------------------------------------------------------------------------------
# 7. trained weights and the flags
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast16", [0, 1], ids=["option_alone", "with_fast16"])
def test_trained_weights_error_band(oracle, fast16):
    cfg, weights, lr, bic, _ = F.golden_crop_ds(oracle)
    with _engine(cfg, weights) as eng:
        assert _kernels(eng) == PLANS["default"][1], _kernels(eng)
        label = "C5 trained weights, golden DS crop, default plan"
        y1, y0, off, rms, mx, e_model = _measure(oracle, label, eng, cfg, weights, lr, bic, ("ds crop",), fast16)
    _band(label, y1, y0, off, rms, mx, e_model, max_abs=False)


def _model(tmp_path, on):
    """SuperResolution from flags on the golden DS x4 weights, default plan."""
    import json
    from dcscn_amd.model import SuperResolution
    with open(os.path.join(GOLDEN, "goldens.json")) as f:
        flags = dict(json.load(f)["models"]["L7_x4_DS"]["flags"])
    flags.update(checkpoint_dir=str(tmp_path / "models"), self_ensemble=1, fast16=on, fast16_separable=on)
    m = SuperResolution(_flags(**flags))
    m.build_graph()
    m.init_all_variables()
    m.load_weights(dict(np.load(os.path.join(GOLDEN, "weights_L7_x4_DS.npz"))))
    assert _kernels(m._engine) == PLANS["default"][1], _kernels(m._engine)
    return m


def test_both_flags_through_the_model(oracle, tmp_path):
    cfg, weights, lr, bic, truth = F.golden_crop_ds(oracle)
    outs = {}
    for on in (False, True):
        m = _model(tmp_path, on)
        try:
            assert m.fast16 is on and m.fast16_separable is on and m.fast16_stream is False
            outs[on] = np.asarray(m.do(lr[0], bic[0]), np.float64)
            selected, separable = F.one_product_set(oracle, cfg, m._engine.ops(), 1, 1)
        finally:
            m.close()
    _, _, e_model = F.model_error(oracle, ("ds crop",), cfg, weights, lr, bic, selected, separable)
    assert outs[False].shape == truth.shape and not _same(outs[True], outs[False])
    mse = {k: float(np.mean((v - truth) ** 2)) for k, v in outs.items()}
    psnr = {k: 10.0 * np.log10(255.0 ** 2 / v) for k, v in mse.items()}
    delta = psnr[True] - psnr[False]
    bound = psnr_delta_bound(e_model, mse[False])
    print("FAST16_SEPARABLE model path, golden DS crop: PSNR %.6f dB (fast16 + fast16_separable) vs %.6f dB, delta %+.3g dB, bound %.3g dB, "
          "rms between the two %.4g, E_model %.4g" % (psnr[True], psnr[False], delta, bound, M.rms(outs[True], outs[False]), e_model))
    assert abs(delta) <= bound
