"""The constructions of tests/overflow_cases.py on the CPU: every hot case tests/test_overflow_hip.py parametrizes meets its
conditions on the float64 oracle, the cases left out are exactly the ones that cannot, the relay nets carry the input's bits, and the
float32 restatement of a hot case is where tests/bare_branch.py says a float32 restatement is.  No GPU."""
import math

import numpy as np
import pytest

import overflow_cases as C
from conftest import CONFIGS

RESTATEMENT_BAR = 1.25e-6               # tests/test_bare_branch_host.py: a float32 restatement within 1.02e-6 on the 200 draws


def test_the_edge_values():
    """65504 and the float32 below 65520 round to a finite f16, 65520 and the float32 above it do not."""
    for v, beyond in C.edge_values():
        with np.errstate(over="ignore"):
            assert bool(np.isinf(np.float16(v))) == beyond, v
    assert C.LIM_LO < C.HOT_PIXEL / 0.85 and C.HOT_PIXEL < C.LIM_LO < C.F16_MAX < C.F16_EDGE < C.LIM_HI


def test_scaling_by_a_power_of_two_is_exact_and_homogeneous(oracle):
    """The guess of first_overflow_at: the target's output at 2^e is 2^e times its output at e = 0, bit for bit in float64."""
    cfg, weights, x, base = C.directed_base(oracle, CONFIGS, "L7_F32to8_x2", C.SHAPE_A)
    for target, e in (("CNN3", 5), ("A1", -3), ("Up-PS_CNN", 7)):
        w = C.scaled_weights(oracle, cfg, weights, target, e)
        _, t = oracle.forward(cfg, w, base["x"], base["x2"], return_intermediates=True)
        assert np.array_equal(t[target], base[target] * math.ldexp(1.0, e))
        for name in C.tensors_before(oracle, cfg, target):
            assert np.array_equal(t[name], base[name])


@pytest.mark.parametrize("net", C.NETS)
def test_leg_a_cases_are_the_feasible_ones(oracle, net):
    """Every conv of the topology either has an exponent in -6 .. 13 (and is a case of leg A, with its conditions asserted on the
    reference's own tensors) or is listed in LEFT_OUT_A."""
    listed = [(shape, t) for n, shape, t, _ in C.cases_a(oracle, CONFIGS) if n == net]
    cfg = oracle.make_config(**CONFIGS[net])
    for shape in (C.SHAPE_A,) + ((C.SHAPE_A_L12,) if net.startswith("L12") else ()):
        cfg, weights, x, base = C.directed_base(oracle, CONFIGS, net, shape)
        for t in C.conv_names(oracle, cfg):
            found = C.first_overflow_at(oracle, cfg, weights, x, shape[3], t, base=base)
            assert (found is not None) == ((shape, t) in listed), (net, shape, t, found and found[1])
            if found is not None:
                assert found[1] in C.DIRECTED_EXPONENTS
    assert all(t in C.conv_names(oracle, cfg) for t in C.LEFT_OUT_A.get(net, ()))


def test_leg_b_cases_are_the_feasible_ones(oracle):
    """One hot pixel: the listed targets admit an exponent at every pixel position, the left-out ones at none."""
    for net, h, w in C.NETS_B:
        for px in C.pixels_b(h, w):
            shape = (3, h, w, (1,) + px)
            cfg, weights, x, base = C.directed_base(oracle, CONFIGS, net, shape)
            for t in C.TARGETS_B[net]:
                case = C.directed_case(oracle, CONFIGS, net, shape, t)
                assert float(np.max(np.abs(case.xb[1]))) == np.float32(C.HOT_PIXEL) and np.array_equal(case.xb[0], case.x[0])
                assert int(np.sum(case.xb != case.x)) == 1
            for t in C.LEFT_OUT_B.get(net, ()):
                assert C.first_overflow_at(oracle, cfg, weights, x, shape[3], t, base=base) is None, (net, px, t)
    assert len(C.cases_b()) == 3 * (4 + 4 + 1)


def test_pass_structure_cases_are_feasible(oracle):
    """Leg D: five images with the hot one first, in the middle and last; a hot pixel on 40 x 33; every flip of the self-ensemble."""
    for net in ("L8_F96to48_x2", "L7_F32to8_x4"):
        for hot in (0, 2, 4):
            assert C.directed_case(oracle, CONFIGS, net, (5, 17, 19, hot), "B1").peak >= C.LIM_HI
        for px in C.pixels_b(40, 33):
            assert C.directed_case(oracle, CONFIGS, net, (2, 40, 33, (1,) + px), "B1").peak >= C.LIM_HI
        cfg, weights = C.shipped_net(oracle, CONFIGS, net)
        x, _ = C.bare_batch(1, 13, 18, cfg["scale"], C.BATCH_SEED)
        for n_ens in (5, 8):
            case = C.EnsembleCase(oracle, cfg, weights, x[0], "B1", n_ens)
            assert np.array_equal(case.ref, oracle.do(cfg, case.weights, case.xb, case.x2, self_ensemble=n_ens))


def test_the_walk_leaves_out_few_draws_and_reaches_many_tensors(oracle):
    """The draws left out are exactly WALK_LEFT_OUT, at most 5 % of 200; the others reach at least 10 distinct target tensors."""
    left, targets = [], {}
    for seed in range(200):
        flags, cfg, weights, x, target, opts = C.walk_setup(oracle, seed)
        assert np.array_equal(x[0], x[1])
        found = C.first_overflow_at(oracle, cfg, weights, x, 1, target, C.WALK_EXPONENTS)
        if found is None:
            left.append(seed)
        else:
            targets[target] = targets.get(target, 0) + 1
    print("WALK left out %r; targets %r" % (left, targets))
    assert tuple(left) == C.WALK_LEFT_OUT
    assert len(left) <= 0.05 * 200
    assert len(targets) >= 10, targets


RELAY_NETS = ("L8_F96to48_x2", "L7_F32to8_x2")


@pytest.mark.parametrize("net", RELAY_NETS)
def test_relay_nets_carry_the_input_bit_for_bit(oracle, net):
    """CNN1[..., channel] is x[..., 0] bit for bit in the float32 restatement, for every edge value at a corner and in the middle, and
    only the relayed value is >= 65504 in any operand; no other value leaves LIM_LO."""
    cfg, weights = C.shipped_net(oracle, CONFIGS, net)
    x, x2 = C.bare_batch(2, 17, 33, cfg["scale"], C.BATCH_SEED)
    for channel in (0, weights["CNN1/conv_W"].shape[3] - 1):
        relay = C.relay_weights(cfg, weights, channel)
        for row, col in ((0, 0), (8, 16)):
            for v, _ in C.edge_values():
                _, t = oracle.forward(cfg, relay, C.relay_input(x, 1, row, col, v), x2, dtype=np.float32, return_intermediates=True)
                assert C.relay_conditions(t, 1, row, col, channel, v) is None, (net, channel, row, col, v, C.relay_conditions(t, 1, row, col, channel, v))


SAMPLE = [("L7_F32to8_x2", C.SHAPE_A, "CNN4"), ("L7_F32to8_x4_DS", C.SHAPE_A, "B2"), ("L8_F96to48_x2", C.SHAPE_A, "A1"),
          ("L8_F96to48_x2", (3, 17, 33, (1, 8, 16)), "CNN8"), ("L12_F196to48_x2", C.SHAPE_A_L12, "CNN12"), ("L7_F32to8_x4", C.SHAPE_A, "Up-PS2_CNN")]


@pytest.mark.parametrize("net,shape,target", SAMPLE, ids=["%s-%s" % (s[0], s[2]) for s in SAMPLE])
def test_float32_restatement_of_a_hot_case(oracle, net, shape, target):
    """Scaling by a power of two moves no rounding: the float32 restatement of a hot case is within 1.25e-6 of float64 on the hot
    image, like the restatements of the clean draws."""
    case = C.directed_case(oracle, CONFIGS, net, shape, target)
    y32 = oracle.forward(case.cfg, case.weights, case.xb, case.x2, dtype=np.float32)
    rel = C.rel_error(y32[case.i], case.ref[case.i])
    print("RESTATEMENT %s %s: %.3g" % (net, target, rel))
    assert np.isfinite(y32).all() and rel <= RESTATEMENT_BAR


def test_launch_names_map_to_the_topology(oracle):
    """launches_around on launch lists as graph.hip names them: which launches write and read a tensor."""
    cfg = oracle.make_config(**CONFIGS["L7_F32to8_x4_DS"])
    ops = [dict(name="CNN1..B2 (streamed)", kernel="feat_stream"), dict(name="Up-PS..R-CNN1 (folded)", kernel="conv5_h")]
    assert [len(v) for v in C.launches_around(oracle, cfg, ops, "CNN3")] == [1, 1]
    writes, reads = C.launches_around(oracle, cfg, ops, "A1")
    assert writes[0]["kernel"] == "feat_stream" and [o["kernel"] for o in reads] == ["conv5_h"]
    streamed_tail = ops[:1] + [dict(name="Up-PS..R-CNN1 (streamed)", kernel="tail_stream")]
    assert C.flag_expected(oracle, cfg, ops, "B2") and not C.flag_expected(oracle, cfg, streamed_tail, "B2", 3)
    assert C.flag_expected(oracle, cfg, ops, "CNN3") and not C.flag_expected(oracle, cfg, ops, "Up-PS_CNN")         # held in LDS; never held
    # a separable 3x3 conv reads through its float32 depthwise stage: on tail_stream neither Concat2 nor the shuffled maps are operands of a contraction
    assert not C.flag_expected(oracle, cfg, streamed_tail, "Up-PS_CNN") and not C.flag_expected(oracle, cfg, streamed_tail, "R-CNN1")
    assert not C.flag_expected(oracle, cfg, streamed_tail, "A1") and not C.flag_expected(oracle, cfg, ops, "B1") and C.flag_expected(oracle, cfg, ops, "CNN7")
    lbl = [dict(name="CNN1..B2 (streamed)", kernel="layer by layer"), dict(name="Up-PS/Up-PS_CNN", kernel="conv_igemm")]
    dense = oracle.make_config(**CONFIGS["L7_F32to8_x2"])
    assert C.flag_expected(oracle, dense, lbl, "CNN4", 3) is None and C.flag_expected(oracle, dense, lbl, "B2", 3) is False
    cfg = oracle.make_config(**CONFIGS["L8_F96to48_x2"])
    ops = [dict(name="CNN%d" % i, kernel="conv_cin1" if i == 1 else "conv3_h") for i in range(1, 9)]
    ops += [dict(name="B1+A1", kernel="conv_nin_h"), dict(name="B2", kernel="conv3_h"), dict(name="Up-PS/Up-PS_CNN+R-CNN1 (folded)", kernel="conv5_h")]
    writes, reads = C.launches_around(oracle, cfg, ops, "CNN1")
    assert [o["name"] for o in writes] == ["CNN1"] and [o["name"] for o in reads] == ["CNN2", "B1+A1"]
    writes, reads = C.launches_around(oracle, cfg, ops, "B1")
    assert [o["name"] for o in writes] == ["B1+A1"] and [o["name"] for o in reads] == ["B2"]
    writes, reads = C.launches_around(oracle, cfg, ops, "Up-PS_CNN")
    assert [o["kernel"] for o in writes] == ["conv5_h"] and [o["kernel"] for o in reads] == ["conv5_h"]
    assert C.flag_expected(oracle, cfg, ops, "B2") and not C.flag_expected(oracle, cfg, ops, "Up-PS_CNN") and not C.flag_expected(oracle, cfg, ops, "R-CNN1")
    assert C.flag_expected(oracle, cfg, ops, "CNN5", 3) and not C.flag_expected(oracle, cfg, [dict(o, kernel="conv_wino2") if o["kernel"] == "conv3_h" else o for o in ops], "B1", 3)
