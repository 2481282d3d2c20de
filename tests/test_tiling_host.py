"""What tests/test_tiling_hip.py rests on, without a GPU (oracle only).

1. With the weights of tests/reach_weights.py the output reaches exactly as far as the reference graph implies, on both
   diagonals: the expected radius is written out per net in ``NETS``.
2. The float32 restatement of the oracle stays within BAR / 4 of float64 on these weights, so the GPU file needs no
   restatement clause.
3. The probe's power: an image cropped one pixel nearer than the true reach, as a window with a halo one pixel short would cut
   it, changes the outermost owned pixels by at least 100 x BAR; cropped at the true reach it changes nothing.
4. Printed beside it, not asserted: the same crop under ``bare_weights(synthetic_weights)``, the weights of every other tiled
   test of the suite -- 0.008 x BAR on the separable x4 net, 1 .. 42 x BAR on the other shipped nets of seven layers or more,
   against 1400 x BAR or more here -- which is why reach weights are needed.

Measured: float32 restatement 9.1e-8 .. 3.4e-7 (L7 x3, (-, -)) against BAR / 4 = 1.25e-6; crop at reach - 1 between 1372 x BAR
(separable x4 net, (-, -)) and 98760 x BAR (L2); crop at the reach itself at most 3.6e-16."""
import numpy as np
import pytest

import bare_branch as B
import reach_weights as RW
from conftest import CONFIGS

_SMALL = dict(layers=3, filters=16, min_filters=8)
# (id, flags, the true reach in LR pixels).  A k x k conv at resolution r adds floor(k / 2) / r; a fraction of an LR pixel at the
# end of the chain reaches into one more LR pixel, so the reach is the sum rounded up.
NETS = [
    ("L12_F196to48_x2", CONFIGS["L12_F196to48_x2"], 15),       # 12 + B2 + Up-PS_CNN + R-CNN1 / 2 = 14.5
    ("L12_F196to48_x4", CONFIGS["L12_F196to48_x4"], 15),       # 12 + 1 + 1 + Up-PS2_CNN / 2 + R-CNN1 / 4 = 14.75
    ("L8_F96to48_x2", CONFIGS["L8_F96to48_x2"], 11),           # 8 + 1 + 1 + 1 / 2
    ("L7_F32to8_x2", CONFIGS["L7_F32to8_x2"], 10),             # 7 + 1 + 1 + 1 / 2
    ("L7_F32to8_x3", CONFIGS["L7_F32to8_x3"], 10),             # 7 + 1 + 1 + 1 / 3
    ("L7_F32to8_x4", CONFIGS["L7_F32to8_x4"], 10),             # 7 + 1 + 1 + 1 / 2 + 1 / 4
    ("L7_F32to8_x4_DS", CONFIGS["L7_F32to8_x4_DS"], 10),
    ("L2_F4to4_x2", CONFIGS["L2_F4to4_x2"], 4),                # no B2: 2 + 1 + 1 / 2
    ("small", _SMALL, 6),                                      # 3 + 1 + 1 + 1 / 2
    ("cnn_size5", dict(_SMALL, cnn_size=5), 10),               # B2 stays 3 x 3: 6 + 1 + 2 + 2 / 2
    ("cnn_size7", dict(_SMALL, cnn_size=7), 15),               # 9 + 1 + 3 + 3 / 2 = 14.5
    ("reconstruct2", dict(_SMALL, reconstruct_layers=2), 6),   # 3 + 1 + 1 + 2 / 2
    ("no_nin", dict(_SMALL, use_nin=False), 5),                # C is 1 x 1: 3 + 1 + 1 / 2
    # transposed conv of scale s, k = 2 s - s % 2, padding p = (k - s) // 2: HR pixel Y takes LR pixel (Y + p - ky) / s where that
    # is whole.  With the 3 x 3 R-CNN1 behind it HR pixel Y reads Y - 1 .. Y + 1, hence LR pixels floor((Y - 1 + p - (k - 1)) / s) ..
    # floor((Y + 1 + p) / s): one LR pixel to either side at x2 (k 4, p 1), x3 (k 5, p 1) and x4 (k 8, p 2).  3 + B2 + 1
    ("transposed_x2", dict(_SMALL, pixel_shuffler=False), 5),
    ("transposed_x3", dict(_SMALL, pixel_shuffler=False, scale=3), 5),
    ("transposed_x4", dict(_SMALL, pixel_shuffler=False, scale=4), 5),
    ("separable5", dict(_SMALL, depthwise_separable=True, cnn_size=5), 10),
    ("tiny", dict(layers=2, filters=8, min_filters=8), 5),     # the window-geometry net: 2 + 1 + 1 + 1 / 2
]


def _diagonals(name):
    """The directions the GPU file uses: both main diagonals, and all four on the window-geometry net."""
    return RW.DIAGONALS if name == "tiny" else RW.DIAGONALS[:2]


_IDS = [n[0] for n in NETS]


def _weights(oracle, flags, sy, sx):
    cfg = oracle.make_config(**flags)
    return cfg, RW.reach_weights(cfg, sy, sx, seed=3)


@pytest.mark.parametrize("name,flags,reach", NETS, ids=_IDS)
def test_true_reach_is_the_radius_the_graph_implies(oracle, name, flags, reach):
    for sy, sx in _diagonals(name):
        cfg, weights = _weights(oracle, flags, sy, sx)
        got = RW.true_reach(oracle, cfg, weights, sy, sx)
        num, den = RW.implied_radius(oracle, cfg)
        print("REACH %s (%+d, %+d): rows %d, columns %d; graph %d / %d" % (name, sy, sx, got[0], got[1], num, den))
        assert got == (reach, reach), (name, sy, sx, got)
        # implied_radius is exact through the pixel shuffler and an upper bound through the transposed conv
        assert reach == -(-num // den) if cfg["pixel_shuffler"] else reach <= -(-num // den), (name, num, den)


@pytest.mark.parametrize("name,flags,reach", NETS, ids=_IDS)
def test_float32_restatement_is_a_quarter_of_the_bar_on_reach_weights(oracle, name, flags, reach):
    for sy, sx in _diagonals(name):
        cfg, weights = _weights(oracle, flags, sy, sx)
        x, x2 = RW.reach_batch(1, 2 * reach + 11, 2 * reach + 17, cfg["scale"], seed=5)
        ref = oracle.forward(cfg, weights, x, x2, dtype=np.float64)
        rel = B.restatement_error(oracle, cfg, weights, x, x2, ref)
        print("RESTATEMENT %s (%+d, %+d): %.3g of max|branch| %.3g" % (name, sy, sx, rel, float(np.max(np.abs(ref)))))
        assert rel <= RW.BAR / 4, (name, sy, sx, rel)


@pytest.mark.parametrize("name,flags,reach", NETS, ids=_IDS)
def test_a_crop_one_pixel_short_of_the_reach_is_seen(oracle, name, flags, reach):
    cfg = oracle.make_config(**flags)
    bare = B.bare_weights(cfg, oracle.synthetic_weights(cfg, seed=7))
    for sy, sx in _diagonals(name):
        cfg, weights = _weights(oracle, flags, sy, sx)
        short = RW.crop_change(oracle, cfg, weights, sy, sx, reach - 1)
        exact = RW.crop_change(oracle, cfg, weights, sy, sx, reach)
        he = RW.crop_change(oracle, cfg, bare, sy, sx, reach - 1)
        print("CROP %s (%+d, %+d) at reach - 1: rows %.3g, columns %.3g (%.0f x BAR); at reach: %.3g, %.3g; "
              "synthetic weights at reach - 1: rows %.3g, columns %.3g (%.2g x BAR)"
              % (name, sy, sx, short[0], short[1], min(short) / RW.BAR, exact[0], exact[1], he[0], he[1], max(he) / RW.BAR))
        assert min(short) >= 100 * RW.BAR, (name, sy, sx, short)
        assert max(exact) <= 1e-12, (name, sy, sx, exact)      # float64 rounding: the oracle sums in an order its matmul picks per shape
