"""Option "fast16_separable" (include/dcscn.h), host side (no GPU): the --fast16_separable switch, the coverage of feat_stream's
instantiations and MFMA forms by the nets the device tests use, and what the device tests of tests/test_fast16_separable_hip.py presuppose,
checked on the CPU restatement (tests/fast16_separable_model.py) ALONE for every net and input they use:

* E_model >= 100 x the rms error of oracle.forward(..., dtype=float32): the band [0.5, 2] x E_model then says something about the mode and
  not about float32 arithmetic (on the attenuated synthetic weights it would not: the model's docstring);
* model max-abs <= 8 x E_model: the device's max-abs bar is not below what the restatement itself shows.

Measured here: E_model / max |ref| 4.7e-5 .. 1.9e-4 on the bare branch (float32 floor 3.5e-8 .. 1.2e-7: a ratio of 860 .. 3300), max-abs / rms
3.7 .. 6.2; trained weights on the 0-255 scale 1.1e-3 (feat_stream's set) and 2.3e-3 (with the folded tail) against a float32 floor of 4.5e-6."""
import numpy as np
import pytest

import fast16_model as M
import fast16_separable_model as F
from test_host import _flags
from test_hip_parity import STREAM_VARIANTS

import dcscn_oracle

NOT_STREAMING = (4, 20, 16, 1.0, 16, 16, 2, "prelu")
STREAMING = F.streaming(dcscn_oracle, STREAM_VARIANTS) + F.EXTRA_VARIANTS


def test_fast16_separable_flag_parses_and_defaults_to_false(tmp_path):
    from helper import args
    from dcscn_amd.model import SuperResolution
    assert "fast16_separable" in args.FLAGS
    flag = args.FLAGS._flags["fast16_separable"]
    assert flag.default is False and flag.kind == "boolean" and args.FLAGS.fast16_separable is False
    others = [args.FLAGS._flags[k] for k in ("fast16", "fast16_stream")]
    saved = [(f.value, f.present) for f in [flag] + others] + [args.FLAGS.is_parsed()]
    try:
        assert args.FLAGS(["prog", "--fast16_separable"]) == ["prog"] and args.FLAGS.fast16_separable is True
        assert args.FLAGS.fast16 is False and args.FLAGS.fast16_stream is False, "--fast16_separable must switch neither --fast16 nor --fast16_stream"
        assert args.FLAGS(["prog", "--fast16_separable=false"]) == ["prog"] and args.FLAGS.fast16_separable is False
        assert args.FLAGS(["prog", "--fast16_separable", "true"]) == ["prog", "true"] and args.FLAGS.fast16_separable is True
        assert args.FLAGS(["prog", "--nofast16_separable"]) == ["prog"] and args.FLAGS.fast16_separable is False
        assert args.FLAGS(["prog", "--fast16", "--fast16_stream", "--nofast16_separable"]) == ["prog"]
        assert args.FLAGS.fast16 is True and args.FLAGS.fast16_stream is True and args.FLAGS.fast16_separable is False
    finally:
        for f, (value, present) in zip([flag] + others, saved[:3]):
            f.value, f.present = value, present
        object.__setattr__(args.FLAGS, "_parsed", saved[3])
    m = SuperResolution(_flags(checkpoint_dir=str(tmp_path / "models")))
    assert m.fast16_separable is False and m.fast16 is False and m.fast16_stream is False
    m = SuperResolution(_flags(checkpoint_dir=str(tmp_path / "models"), fast16_separable=True))
    assert m.fast16_separable is True and m.fast16 is False and m.fast16_stream is False
    m = SuperResolution(_flags(checkpoint_dir=str(tmp_path / "models"), fast16=True, fast16_stream=True))
    assert m.fast16_separable is False and m.fast16 is True and m.fast16_stream is True


def test_the_nets_reach_every_instantiation_and_every_last_chunk_width(oracle):
    """STREAM_VARIANTS was laid out for the instantiations; the (4, 20, 16, ...) entry would need <5, 2>, which is not instantiated: it does
    not stream and is the option's no-op case on a separable net.  So are the relu and leaky_relu entries: both hold a 6-quad layer
    with one output tile, which graph.hip: stream_conv_supported sends layer by layer.  The four that stream reach every instantiation
    but <8, 1> (no 8-quad layer of theirs has <= 16 outputs), which the extra 32 -> 12 net reaches."""
    assert NOT_STREAMING in STREAM_VARIANTS and not F.streams(oracle, NOT_STREAMING) and (5, 2) in F.conv_pairs(oracle, NOT_STREAMING)
    not_streaming = [v for v in STREAM_VARIANTS if not F.streams(oracle, v)]
    assert len(not_streaming) == 3 and all((6, 1) in F.conv_pairs(oracle, v) for v in not_streaming if v != NOT_STREAMING), not_streaming
    assert len(STREAMING) == 5 and all(F.streams(oracle, v) for v in F.EXTRA_VARIANTS)
    assert (8, 1) not in set().union(*[set(F.conv_pairs(oracle, v)) for v in F.streaming(oracle, STREAM_VARIANTS)])
    reached, widths, k16, k32 = set(), set(), False, False
    for v in STREAMING:
        assert F.streams(oracle, v), (v, F.conv_pairs(oracle, v))
        reached |= set(F.conv_pairs(oracle, v))
        widths |= set(F.last_chunk_quads(oracle, v))
        forms = F.chunk_parities(oracle, v)
        k16, k32 = k16 or forms["k16"], k32 or forms["k32"]
    print("FAST16_SEPARABLE host: stream_conv_role<quads, tiles> reached %s, last-chunk quads of the A1 || B1 sources %s" % (sorted(reached), sorted(widths)))
    assert reached == F.INSTANTIATED, sorted(F.INSTANTIATED - reached)
    assert widths == {1, 2, 3, 4}
    assert k16 and k32, "both MFMA forms: chunk pairs on K = 32 and an odd last chunk on K = 16"
    # C5 itself: 32 -> 26 -> 22 -> 18 -> 14 -> 11 -> 8 and B2 8 -> 8; Up-PS and Up-PS2 read 8 quads (two chunk pairs)
    cfg, _ = F.c5(oracle)
    assert oracle.filter_schedule(7, 32, 8, 1.2) == [32, 26, 22, 18, 14, 11, 8] and cfg["nin_filters"] + cfg["nin_filters2"] == 32


def test_one_product_sets(oracle):
    cfg, _ = F.c5(oracle)
    feat = dict(name="CNN1..B2 (streamed)", kernel="feat_stream")
    tail = dict(name="Up-PS..R-CNN1 (streamed)", kernel="tail_stream")
    fold = dict(name="Up-PS..R-CNN1 (folded)", kernel="conv5_h")
    assert F.streamed_set(oracle, cfg, [feat]) == F.FEAT_SET_C5
    assert F.streamed_set(oracle, cfg, [tail]) == F.TAIL_SET_C5
    assert F.streamed_set(oracle, cfg, [feat, tail]) == F.FEAT_SET_C5 | F.TAIL_SET_C5
    assert F.streamed_set(oracle, cfg, [feat, fold]) == F.FEAT_SET_C5
    assert F.one_product_set(oracle, cfg, [feat, fold], 0, 0) == (frozenset(), frozenset())
    assert F.one_product_set(oracle, cfg, [feat, fold], 1, 0) == (F.FOLD_SET_C5, frozenset())
    assert F.one_product_set(oracle, cfg, [feat, fold], 0, 1) == (F.FEAT_SET_C5, F.FEAT_SET_C5)
    assert F.one_product_set(oracle, cfg, [feat, fold], 1, 1) == (F.FEAT_SET_C5 | F.FOLD_SET_C5, F.FEAT_SET_C5)
    layered = [dict(name="CNN2/depthwise", kernel="depthwise"), dict(name="CNN2", kernel="conv_igemm")]
    assert F.one_product_set(oracle, cfg, layered, 0, 1) == (frozenset(), frozenset())


def test_the_restatement_of_a1_b1_is_the_devices_not_the_layer_kernels(oracle):
    """One scale over both folded filters, the ring value rounded without the depthwise factor: differs from fast16_model.restate on the
    same set, and is the same where A1 and B1 are not selected."""
    cfg, weights = F.c5(oracle)
    n, h, w = F.SHAPES[0]
    x, x2 = F.bare_input(n, h, w, cfg["scale"], seed=h + w)
    mine = F.restate(oracle, cfg, weights, x, x2, F.FEAT_SET_C5)
    theirs = M.restate(oracle, cfg, weights, x, x2, F.FEAT_SET_C5)
    assert not np.array_equal(mine, theirs)
    rest = F.FEAT_SET_C5 - {"A1", "B1"}
    assert np.array_equal(F.restate(oracle, cfg, weights, x, x2, rest), M.restate(oracle, cfg, weights, x, x2, rest))
    assert np.array_equal(F.restate(oracle, cfg, weights, x, x2, F.FEAT_SET_C5, frozenset()), theirs)
    s = F.nin_scale(weights, ["A1", "B1"])
    both = np.concatenate([F.folded_nin(weights, v).ravel() for v in ("A1", "B1")])
    assert 2.0 ** 13 <= np.abs(both).max() * s < 2.0 ** 14


def _presupposed(oracle, label, key, cfg, weights, x, x2, selected, separable=None, max_abs=True):
    ref, mod, e = F.model_error(oracle, key, cfg, weights, x, x2, selected, separable)
    floor = M.rms(oracle.forward(cfg, weights, x, x2, dtype=np.float32), ref)
    mx, scale = M.max_abs(mod, ref), float(np.abs(ref).max())
    print("FAST16_SEPARABLE host %s: output scale %.4g | E_model %.4g (%.3g x scale) | model max-abs / rms %.2f | float32 oracle rms %.4g (%.3g x scale) | "
          "E_model / float32 %.0f | %d convs" % (label, scale, e, e / scale, mx / e, floor, floor / scale, e / floor, len(selected)))
    assert np.isfinite(mod).all() and e >= 100.0 * floor, "%s: E_model %.4g is not 100 x the float32 floor %.4g" % (label, e, floor)
    if max_abs:
        assert mx <= 8.0 * e, "%s: the restatement's own max-abs %.4g is above 8 x E_model %.4g" % (label, mx, e)


@pytest.mark.parametrize("shape", F.SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_device_conditions_hold_for_the_restatement_alone_c5(oracle, shape):
    cfg, weights = F.c5(oracle)
    n, h, w = shape
    x, x2 = F.bare_input(n, h, w, cfg["scale"], seed=h + w)
    key = ("c5 bare",) + shape
    _presupposed(oracle, "C5 bare feat_stream %dx%dx%d" % shape, key, cfg, weights, x, x2, F.FEAT_SET_C5)
    if shape in F.TAIL_SHAPES:
        _presupposed(oracle, "C5 bare tail_stream %dx%dx%d" % shape, key, cfg, weights, x, x2, F.TAIL_SET_C5)
        _presupposed(oracle, "C5 bare feat_stream + tail_stream %dx%dx%d" % shape, key, cfg, weights, x, x2, F.FEAT_SET_C5 | F.TAIL_SET_C5)
    if shape == F.SHAPES[0]:
        _presupposed(oracle, "C5 bare feat_stream + folded tail (fast16) %dx%dx%d" % shape, key, cfg, weights, x, x2, F.FEAT_SET_C5 | F.FOLD_SET_C5,
                     F.FEAT_SET_C5, max_abs=False)


@pytest.mark.parametrize("v", STREAMING, ids=lambda v: "L%d_F%dto%d_x%d" % (v[0], v[1], v[2], v[6]))
def test_device_conditions_hold_for_the_restatement_alone_variants(oracle, v):
    cfg, weights = F.variant(oracle, v)
    n, h, w = F.VARIANT_SHAPE
    x, x2 = F.bare_input(n, h, w, cfg["scale"], seed=5)
    names = [o["name"] for o in F.C.convs(oracle, cfg)]
    selected = F.streamed_set_of(oracle, cfg, "feat_stream", "CNN1..B2 (streamed)")
    assert selected == set(names[1:names.index("B2") + 1])
    _presupposed(oracle, "variant %s bare feat_stream" % (v,), ("variant", v), cfg, weights, x, x2, selected)


def test_device_conditions_hold_on_the_trained_weights(oracle):
    """The golden DS crop with its real bicubic x2: no max-abs condition is put on the device there."""
    cfg, weights, lr, bic, truth = F.golden_crop_ds(oracle)
    assert lr.shape == (1, 48, 48, 1) and bic.shape == (1, 192, 192, 1) and truth.shape == (192, 192, 1)
    _presupposed(oracle, "trained DS crop feat_stream", ("ds crop",), cfg, weights, lr, bic, F.FEAT_SET_C5, max_abs=False)
    _presupposed(oracle, "trained DS crop feat_stream + folded tail (fast16)", ("ds crop",), cfg, weights, lr, bic, F.FEAT_SET_C5 | F.FOLD_SET_C5,
                 F.FEAT_SET_C5, max_abs=False)
    ref = F.reference(oracle, ("ds crop",), cfg, weights, lr, bic)
    assert float(np.mean((ref[0] - truth) ** 2)) > 1.0          # a real super-resolution error to compare PSNRs against
