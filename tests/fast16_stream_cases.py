"""Nets, one-product sets and coverage of the engine option "fast16_stream" (include/dcscn.h), shared by tests/test_fast16_stream_host.py
and tests/test_fast16_stream_hip.py.

With fast16_stream = 1 every MFMA contraction of a feat3_stream launch (csrc/feat3_stream.hpp: NP = 1) is the single product wh * xh:
CNN2 .. CNNL on s3_conv_role<octets of the input, output tiles>, and with A1 || B1 and B2 inside the launch (option "stream_nin", the
c-DCSCN shape only) also those, on s3_pair_role / s3_nin_role.  CNN1 stays float32 VALU work.  The CPU restatement is
tests/fast16_model.py's, on the set of convs below.

The dispatch of the launch instantiates <octets, tiles> for octets 1 .. 4 and tiles 1, 2; a filter schedule never widens, so two tiles
(>= 17 outputs) behind one or two octets (<= 16 inputs) cannot occur.  The three nets below reach the other six."""
import fast16_model as M
import overflow_cases as C
from conftest import CONFIGS

_NIN = dict(nin_filters=24, nin_filters2=8)
NETS = {
    "L7_F32to8_x2": CONFIGS["L7_F32to8_x2"],                    # c-DCSCN: 32, 26, 22, 18, 14, 11, 8
    "L7_F32to8_x3": CONFIGS["L7_F32to8_x3"],
    "L7_F32to8_x4": CONFIGS["L7_F32to8_x4"],
    "L8_F32to1": dict(layers=8, filters=32, min_filters=1, filters_decay_gamma=1.5, **_NIN),      # 32, 23, 18, 14, 10, 7, 4, 1
    "L2_F32to8": dict(layers=2, filters=32, min_filters=8, **_NIN),                               # 32, 8
    # 32, 28, 26, 25, 24 and B2 24 -> 24: every 3x3 conv behind CNN1 reads >= 24 channels, which is what the layer-by-layer plan asks of a
    # layer before it leaves the float32 kernels (graph.hip: wino_eligible / h16_direct_eligible) -- on c-DCSCN x3 CNN5 .. CNN7 and B2 stay
    # on conv_igemm, so its two plans' one-product sets differ; on this net they coincide
    "L5_F32to24_x3": dict(scale=3, layers=5, filters=32, min_filters=24, nin_filters=24, nin_filters2=24, reconstruct_layers=0,
                          pixel_shuffler_filters=1),
}
REACHABLE = frozenset((o, t) for o in (1, 2, 3, 4) for t in (1, 2)) - {(1, 2), (2, 2)}


def schedule(oracle, flags):
    return oracle.filter_schedule(flags["layers"], flags["filters"], flags["min_filters"], flags.get("filters_decay_gamma", 1.5))


def instantiations(oracle, flags):
    """[(octets of the input ring, 16-channel output tiles)] of CNN2 .. CNNL, the template arguments of s3_conv_role."""
    s = schedule(oracle, flags)
    return [((s[i] + 7) // 8, (s[i + 1] + 15) // 16) for i in range(len(s) - 1)]


def assert_coverage(oracle):
    """The three nets reach every instantiation the dispatch can; the schedules are the ones the tests were laid out for."""
    assert schedule(oracle, NETS["L7_F32to8_x2"]) == [32, 26, 22, 18, 14, 11, 8]
    assert schedule(oracle, NETS["L8_F32to1"]) == [32, 23, 18, 14, 10, 7, 4, 1]
    assert schedule(oracle, NETS["L2_F32to8"]) == [32, 8]
    for scale in (3, 4):
        assert schedule(oracle, NETS["L7_F32to8_x%d" % scale]) == schedule(oracle, NETS["L7_F32to8_x2"])
    got = {name: instantiations(oracle, flags) for name, flags in NETS.items()}
    assert got["L7_F32to8_x2"] == [(4, 2), (4, 2), (3, 2), (3, 1), (2, 1), (2, 1)], got
    assert got["L2_F32to8"] == [(4, 1)], got
    assert (1, 1) in got["L8_F32to1"], got
    for name, flags in NETS.items():
        s = schedule(oracle, flags)
        assert max(s) <= 32 and s == sorted(s, reverse=True), (name, s)
    reached = set().union(*[set(v) for v in got.values()])
    assert reached == REACHABLE, sorted(REACHABLE - reached)
    return got


def streamed_launch_name(cfg, stream_nin=True):
    """The name graph.hip gives the feat3_stream launch of ``cfg``: A1 || B1 and B2 are inside it for the c-DCSCN shape only."""
    nin_on = stream_nin and cfg["layers"] == 7 and cfg["nin_filters"] == 24 and cfg["nin_filters2"] == 8
    return "CNN1..%s (streamed)" % ("B2" if nin_on else "CNN%d" % cfg["layers"])


def _names(oracle, cfg):
    convs = C.convs(oracle, cfg)
    return [o["name"] for o in convs], [o["var"] for o in convs]


def streamed_set_of(oracle, cfg, launch_name):
    """The convs a feat3_stream launch of that name takes on one product: all it computes but CNN1."""
    names, vars_ = _names(oracle, cfg)
    return frozenset(C._covered(launch_name, names, vars_)) - {"CNN1"}


def streamed_set(oracle, cfg, ops):
    """The same from Engine.ops(): empty where the plan has no feat3_stream launch."""
    out = set()
    for op in ops:
        if op["kernel"] == "feat3_stream":
            assert op["name"].startswith("CNN1..") and op["name"].endswith(" (streamed)"), op
            out |= streamed_set_of(oracle, cfg, op["name"])
    return frozenset(out)


def one_product_set(oracle, cfg, ops, fast16, fast16_stream):
    """The convs on one product under the two options, from Engine.ops() of a handle at split16 = 1."""
    out = set()
    if fast16_stream:
        out |= streamed_set(oracle, cfg, ops)
    if fast16:
        out |= M.selected_by_ops(oracle, cfg, ops)
    return frozenset(out)


BAND_SHAPES = [(1, 19, 35), (3, 7, 9), (2, 50, 51)]            # 50 x 51: two column strips (strips are 48 pixels wide)
BAND_SEED = 0
# (net, stream_nin): c-DCSCN with the pair and NIN roles, and on the plain conv roles; the two nets that complete the instantiations
BAND_NETS = [("L7_F32to8_x2", 1), ("L7_F32to8_x2", 0), ("L8_F32to1", 1), ("L2_F32to8", 1)]
