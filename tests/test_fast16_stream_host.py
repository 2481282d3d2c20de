"""Option "fast16_stream" (include/dcscn.h), host side (no GPU): the --fast16_stream switch, the coverage of feat3_stream's
instantiations by the nets of tests/fast16_stream_cases.py, and the conditions the device tests of tests/test_fast16_stream_hip.py put on
the device output (a nonzero error, max-abs <= 8 x rms), checked first on the CPU restatement (tests/fast16_model.py) restricted to the
streamed set alone, on the seeded inputs those tests use."""
import numpy as np
import pytest

import fast16_model as M
import fast16_stream_cases as S
from conftest import synthetic_batch
from test_host import _flags


def test_fast16_stream_flag_parses_and_defaults_to_false(tmp_path):
    from helper import args
    from dcscn_amd.model import SuperResolution
    assert "fast16_stream" in args.FLAGS
    flag = args.FLAGS._flags["fast16_stream"]
    assert flag.default is False and flag.kind == "boolean" and args.FLAGS.fast16_stream is False
    other = args.FLAGS._flags["fast16"]
    saved = (flag.value, flag.present, other.value, other.present, args.FLAGS.is_parsed())
    try:
        assert args.FLAGS(["prog", "--fast16_stream"]) == ["prog"] and args.FLAGS.fast16_stream is True
        assert args.FLAGS.fast16 is False, "--fast16_stream must not switch --fast16 on"
        assert args.FLAGS(["prog", "--fast16_stream=false"]) == ["prog"] and args.FLAGS.fast16_stream is False
        assert args.FLAGS(["prog", "--fast16_stream", "true"]) == ["prog", "true"] and args.FLAGS.fast16_stream is True
        assert args.FLAGS(["prog", "--nofast16_stream"]) == ["prog"] and args.FLAGS.fast16_stream is False
        assert args.FLAGS(["prog", "--fast16", "--nofast16_stream"]) == ["prog"] and args.FLAGS.fast16 is True and args.FLAGS.fast16_stream is False
    finally:
        flag.value, flag.present, other.value, other.present = saved[:4]
        object.__setattr__(args.FLAGS, "_parsed", saved[4])
    m = SuperResolution(_flags(checkpoint_dir=str(tmp_path / "models")))
    assert m.fast16_stream is False and m.fast16 is False
    m = SuperResolution(_flags(checkpoint_dir=str(tmp_path / "models"), fast16_stream=True))
    assert m.fast16_stream is True and m.fast16 is False
    m = SuperResolution(_flags(checkpoint_dir=str(tmp_path / "models"), fast16=True))
    assert m.fast16_stream is False and m.fast16 is True


def test_the_nets_reach_every_reachable_instantiation(oracle):
    got = S.assert_coverage(oracle)
    print({k: v for k, v in got.items()})
    assert {name for name, _ in S.BAND_NETS} == {"L7_F32to8_x2", "L8_F32to1", "L2_F32to8"}


def test_streamed_sets(oracle):
    cfg = oracle.make_config(**S.NETS["L7_F32to8_x2"])
    assert S.streamed_launch_name(cfg, 1) == "CNN1..B2 (streamed)" and S.streamed_launch_name(cfg, 0) == "CNN1..CNN7 (streamed)"
    assert S.streamed_set_of(oracle, cfg, "CNN1..B2 (streamed)") == {"CNN%d" % i for i in range(2, 8)} | {"A1", "B1", "B2"}
    assert S.streamed_set_of(oracle, cfg, "CNN1..CNN7 (streamed)") == {"CNN%d" % i for i in range(2, 8)}
    cfg = oracle.make_config(**S.NETS["L8_F32to1"])
    assert S.streamed_launch_name(cfg, 1) == "CNN1..CNN8 (streamed)"
    ops = [dict(name="CNN1..CNN7 (streamed)", kernel="feat3_stream"), dict(name="B1+A1", kernel="conv_nin_h"), dict(name="B2", kernel="conv3_h")]
    cfg = oracle.make_config(**S.NETS["L7_F32to8_x2"])
    assert S.one_product_set(oracle, cfg, ops, 0, 0) == frozenset()
    assert S.one_product_set(oracle, cfg, ops, 1, 0) == {"A1", "B1", "B2"}
    assert S.one_product_set(oracle, cfg, ops, 0, 1) == {"CNN%d" % i for i in range(2, 8)}
    assert S.one_product_set(oracle, cfg, ops, 1, 1) == {"CNN%d" % i for i in range(2, 8)} | {"A1", "B1", "B2"}
    ops[0]["kernel"] = "layer by layer"                          # split16 = 0 / stream_dense = 0: nothing for the option to govern
    assert S.one_product_set(oracle, cfg, ops, 0, 1) == frozenset()


@pytest.mark.parametrize("shape", S.BAND_SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("net,stream_nin", S.BAND_NETS, ids=["%s-nin%d" % c for c in S.BAND_NETS])
def test_device_conditions_hold_for_the_restatement_on_the_streamed_set_alone(oracle, net, stream_nin, shape):
    cfg = oracle.make_config(**S.NETS[net])
    weights = oracle.synthetic_weights(cfg, seed=0)
    n, h, w = shape
    x, x2 = synthetic_batch(n, h, w, cfg["scale"], seed=S.BAND_SEED)
    selected = S.streamed_set_of(oracle, cfg, S.streamed_launch_name(cfg, stream_nin))
    assert selected and "CNN1" not in selected
    ref, mod, e = M.model_error(oracle, ("stream band", net) + shape, cfg, weights, x, x2, selected)
    mx = M.max_abs(mod, ref)
    print("FAST16_STREAM host %s stream_nin %d %dx%dx%d: E_model %.4g max-abs %.4g max / rms %.2f (%d convs)" % (
        net, stream_nin, n, h, w, e, mx, mx / e, len(selected)))
    assert e > 1e-6 and mx <= 8 * e


def test_device_conditions_hold_on_the_trained_weights(oracle):
    """The golden crop: no max-abs condition is put on the device there (the restatement's own max / rms is above 8)."""
    from test_fast16_host import golden_crop
    cfg, weights, lr, bic, _ = golden_crop(oracle)
    selected = S.streamed_set_of(oracle, cfg, S.streamed_launch_name(cfg, 1))
    ref, mod, e = M.model_error(oracle, ("golden crop",), cfg, weights, lr, bic, selected)
    print("FAST16_STREAM host golden crop: E_model %.4g max-abs %.4g" % (e, M.max_abs(mod, ref)))
    assert e > 1e-6 and np.isfinite(mod).all()
