"""Option "train_split16_wgrad" (include/dcscn.h), host side (no GPU): the --train_split16_wgrad switch, the restated split rule of
csrc/train_wgrad_h.hpp and a CPU model of one weight-gradient dot product."""
import os
import re

import numpy as np
import pytest

import train_split16_wgrad_cases as G
from test_host import _flags

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dcscn-super-resolution_amd", "csrc")


def test_train_split16_wgrad_flag_parses_and_defaults_to_false(tmp_path):
    from helper import args
    from dcscn_amd.model import SuperResolution
    assert "train_split16_wgrad" in args.FLAGS
    flag = args.FLAGS._flags["train_split16_wgrad"]
    assert flag.default is False and flag.kind == "boolean" and args.FLAGS.train_split16_wgrad is False
    saved = (flag.value, flag.present, args.FLAGS.is_parsed())
    try:
        assert args.FLAGS(["prog", "--train_split16_wgrad"]) == ["prog"] and args.FLAGS.train_split16_wgrad is True
        assert args.FLAGS.train_split16 is False                                    # (independent of the other switch)
        assert args.FLAGS(["prog", "--notrain_split16_wgrad"]) == ["prog"] and args.FLAGS.train_split16_wgrad is False
    finally:
        flag.value, flag.present = saved[0], saved[1]
        object.__setattr__(args.FLAGS, "_parsed", saved[2])
    m = SuperResolution(_flags(checkpoint_dir=str(tmp_path / "models")))
    assert m.train_split16_wgrad is False and m.train_split16 is False
    m = SuperResolution(_flags(checkpoint_dir=str(tmp_path / "models"), train_split16_wgrad=True))
    assert m.train_split16_wgrad is True and m.train_split16 is False


def test_the_model_sets_the_option_on_its_training_engine(tmp_path):
    """model.py passes the switch on: the engine it trains with sees set_option("train_split16_wgrad", 1), and not without the switch."""
    import inspect
    from dcscn_amd import model
    src = inspect.getsource(model.SuperResolution)
    at = src.index('eng.set_option("train_split16_wgrad", 1)')
    guard = src.rfind("if self.train_split16_wgrad:", 0, at)
    assert guard >= 0 and src[guard:at].count("\n") == 1
    assert src.index('eng.set_option("train_split16", 1)') < at


def test_the_restated_constants_are_the_headers():
    text = open(os.path.join(CSRC, "train_wgrad_h.hpp")).read()
    value = lambda name: eval(re.search(r"constexpr \w+ %s = ([0-9 *]+);" % name, text).group(1))
    assert (value("kWgHBlock"), value("kWgHPitch"), value("kWgHLdsBudget"), value("kWgHLdsMax")) == (G.BLOCK, G.PITCH, G.LDS_BUDGET, G.LDS_MAX)
    assert G.PITCH % 8 == 0 and (G.PITCH // 4) % 64 == 8 and G.PITCH >= 4 * G.BLOCK


SHAPES = [(ks, cin, cout, n, H, W) for ks in (1, 3, 5, 7) for cin, cout in ((16, 16), (40, 19), (104, 64), (196, 196), (1301, 64))
          for n, H, W in ((1, 1, 1), (2, 7, 9), (1, 1, 150), (1, 150, 1), (1, 72, 71), (3, 148, 200), (20, 48, 48), (20, 96, 96), (1, 2401, 1))]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_split_rule_partitions_every_shape_within_the_lds_budget(shape):
    ks, cin, cout, n, H, W = shape
    p = G.wgrad_h_plan(*shape)
    assert 1 <= p.tr <= min(H, 8) and 1 <= p.tc <= W and p.tcp == p.tc + ks - 1
    assert p.kpad % 32 == 0 and p.kpad >= p.tr * p.tcp > p.kpad - 32
    # the farthest position a tap reads: the last dz position moved by the last tap
    assert p.in_cap % 16 == 0 and p.in_cap >= p.kpad + (ks - 1) * p.tcp + (ks - 1) and p.in_cap >= (p.tr + ks - 1) * p.tcp
    assert p.lds_bytes == (p.kpad + p.in_cap) * G.PITCH <= G.LDS_MAX
    assert p.tr == 1 or p.lds_bytes <= G.LDS_BUDGET
    assert p.tiles == n * p.tiles_y * p.tiles_x and p.tiles_y * p.tr >= H > (p.tiles_y - 1) * p.tr and p.tiles_x * p.tc >= W > (p.tiles_x - 1) * p.tc
    assert p.tg * p.groups == ks * ks
    assert p.splits >= 1 and (p.splits - 1) * p.tps < p.tiles <= p.splits * p.tps          # every split has a tile, every tile a split


def test_the_split_rule_on_the_shapes_the_device_tests_rely_on():
    # L12 x2 on 20 x 48^2, a 3x3 layer of 196 -> 196: 3 rows of 50 positions (4 rows would take 161,280 bytes), 16 splits of 20 tiles
    p = G.wgrad_h_plan(3, 196, 196, 20, 48, 48)
    assert (p.tr, p.tc, p.tcp, p.kpad, p.in_cap, p.tiles, p.tps, p.splits) == (3, 48, 50, 160, 272, 320, 20, 16) and p.lds_bytes == 124416
    # one pixel wide: tiles of 8 pixels, two per split
    for H, tiles, splits in ((2399, 300, 150), (2400, 300, 150), (2401, 301, 151)):
        p = G.wgrad_h_plan(3, 40, 26, 1, H, 1)
        assert (p.tr, p.tc, p.kpad, p.tiles, p.tps, p.splits) == (8, 1, 32, tiles, 2, splits), (H, p)
    # the small-gradient case, ODD at x4: the Up-PS2 conv (41 -> 164) runs on 3 x 74 x 100
    p = G.wgrad_h_plan(3, 41, 164, 3, 74, 100)
    assert (p.tr, p.tc, p.tiles_x, p.kpad, p.tiles, p.tps, p.splits) == (2, 64, 2, 160, 222, 3, 74) and p.tr * p.tcp == 132


MAGNITUDES = (1e-4, 1e-5, 1e-6, 1e-7, 1e-8, 1e-9)


@pytest.mark.parametrize("K", [2048, 46080])
def test_the_scaled_split_is_no_worse_than_the_f32_chain_on_a_weight_gradient_dot_product(K):
    """One element of a weight gradient, sum over K pixels of in[p] * dz[p]: in = PReLU(N(0, 1)) with slope 0.1 clipped to +-4, dz = N(0, 1)
    times 1e-4 .. 1e-9; 16 dot products per magnitude.  Error relative to max|exact| over the 16:
        K = 2,048:   scaled split 9.5e-8 .. 3.0e-7, f32 chain 4.6e-7 .. 1.6e-6
        K = 46,080:  scaled split 4.4e-7 .. 1.4e-6, f32 chain 2.8e-6 .. 5.1e-6
    (what is left of the split's error is the f32 accumulator's rounding, once per chunk of 32 instead of once per element), so one split
    may run over all 46,080 pixels of the L12 batch: the split count need not bound the chunk length."""
    rng = np.random.default_rng(K)
    for mag in MAGNITUDES:
        z = rng.standard_normal((16, K))
        a = np.clip(np.where(z > 0.0, z, 0.1 * z), -4.0, 4.0).astype(np.float32)
        b = (rng.standard_normal((16, K)) * mag).astype(np.float32)
        exact, split, chain = G.dot_models(a, b)
        top = float(np.max(np.abs(exact)))
        es, ec = float(np.max(np.abs(split - exact))) / top, float(np.max(np.abs(chain - exact))) / top
        print("MODEL K %d dz %.0e: scaled split %.3g, f32 chain %.3g of max|exact|" % (K, mag, es, ec))
        assert es <= ec, (K, mag, es, ec)
