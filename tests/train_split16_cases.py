"""Shared cases of tests/test_train_split16_hip.py (test helper, not a test): option "train_split16" of include/dcscn.h.

Every case is a net, a batch shape, an activator, a dropout keep probability and a loss.  The float64 reference of a case
(train_ref.loss_and_grads) and the device's gradients with the option off and on are computed once per process and shared; the
returned arrays are not to be written to.  The bar is the f32 path's own: every gradient tensor within 1e-4 * max|g64|, the loss
stats within 1e-6 relative (test_train_surface_hip._compare also asks for exact zeros where the float64 gradient is identically
zero, a finite everything and the global norm to 1e-4).  A CPU model of one data-gradient dot product (K = 9 * 196, weights
N(0, 0.03), hi = f16(x), lo = f16(x - hi), exact products, f32 accumulation per chunk of 32) puts split16 with both operands scaled by
a power of two at 2.6e-7 .. 3.4e-7 of max|exact| for dz of 1e-4 .. 1e-9, the f32 chain at 1.2e-6 .. 1.4e-6 and the UNSCALED split at
1.5e-4 .. 1.0: the mode has no excuse for a wider bar than the f32 path, and an unscaled port fails it."""
import functools

import numpy as np

from conftest import CONFIGS
import dcscn_oracle as O
import train_ref as R
from test_train_hip import FLAGS, _batch

L2_DECAY = 1e-3
TOL = 1e-4

# layers 3, filters 40 -> 19 (odd, no multiples of 8), NIN 24 / 17, 3x3: every layer but CNN1 and the last conv is eligible
ODD = dict(layers=3, filters=40, min_filters=19, nin_filters=24, nin_filters2=17, scale=2)
# 5x5 without NIN (the 1x1 "C" layer instead), x3, 5 pixel-shuffler filters
K5 = dict(layers=2, filters=33, min_filters=17, cnn_size=5, use_nin=False, scale=3, pixel_shuffler_filters=5)
# x4 with two reconstruction layers of 18 filters in front of the last conv: eligible layers at 4x the resolution, both Up-PS data gradients eligible
X4R = dict(layers=2, filters=20, min_filters=16, nin_filters=18, nin_filters2=16, scale=4, reconstruct_layers=3, reconstruct_filters=18)
# c-DCSCN x2, filters 32 -> 8: eligible and ineligible layers in one step
MIXED = CONFIGS["L7_F32to8_x2"]
# no eligible layer at all (one pixel-shuffler filter: the Up-PS conv is 16 -> 4)
NARROW = dict(layers=2, filters=12, min_filters=8, nin_filters=8, nin_filters2=8, scale=2, pixel_shuffler_filters=1)

#        name          net    activator  (n, h, w)    keep  l1
CASES = {
    "odd-2x7x9":     (ODD,   "prelu",   (2, 7, 9),   1.0, False),    # 126 pixels: less than one 128-pixel tile
    "odd-1x13x11":   (ODD,   "selu",    (1, 13, 11), 0.8, False),    # 143 pixels: one tile and a ragged one
    "k5-1x6x5":      (K5,    "relu",    (1, 6, 5),   1.0, True),
    "x4r-1x5x4":     (X4R,   "prelu",   (1, 5, 4),   0.8, False),
    "mixed-2x8x8":   (MIXED, "prelu",   (2, 8, 8),   0.8, True),
    "mixed-1x1x1":   (MIXED, "prelu",   (1, 1, 1),   1.0, False),
}
NETS = ("odd-2x7x9", "k5-1x6x5", "x4r-1x5x4", "mixed-2x8x8")       # one case per net
KEY = 0x5117


def eligible(cin, cout):
    return min(cin, cout) >= 16


def eligible_layers(cfg):
    return [op["var"] for op in O.build_topology(cfg) if op["op"] == "conv" and eligible(op["cin"], op["cout"])]


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(cfg, weights, x, x2, y) of a case: synthetic weights seed 0, the batch of test_train_hip._batch seed 1; selu takes x / 255 as the
    surface tests do (exp off saturation)."""
    over, act, (n, h, w), _, _ = CASES[name]
    cfg = O.make_config(**dict(over, activator=act))
    weights = O.synthetic_weights(cfg, seed=0)
    x, x2, y = _batch(cfg, n, h, w, 1)
    if act == "selu":
        x = x / np.float32(255.0)
    return cfg, weights, x, x2, y


def train_flags(name):
    _, _, _, keep, l1 = CASES[name]
    return dict(FLAGS, use_l1_loss=l1, dropout_rate=keep, l2_decay=L2_DECAY)


def engine_for(cfg, weights, on, **flags):
    """A training handle with the option set BEFORE dcscn_train_begin."""
    from dcscn_amd import engine
    eng = engine.Engine(cfg, device=0)
    eng.load_weights(weights)
    eng.set_option("train_split16", 1 if on else 0)
    eng.train_begin(dict(FLAGS, **flags))
    return eng


def grads_and_stats(eng, names, x, x2, y, key=KEY):
    stats = eng.train_gradients(x, x2, y, dropout_key=key)
    return stats, {k: eng.get_tensor(k + "/grad") for k in names}


@functools.lru_cache(maxsize=None)
def device(name, on):
    """(stats, {name: gradient}) of the case on a fresh handle with the option off / on."""
    cfg, weights, x, x2, y = inputs(name)
    with engine_for(cfg, weights, on, **train_flags(name)) as eng:
        return grads_and_stats(eng, weights, x, x2, y)


def bits(stats, grads):
    out = {k: np.asarray(v).view(np.uint32) for k, v in grads.items()}
    out["stats"] = np.asarray(stats, np.float64).view(np.uint32)
    return out


def same_bits(a, b):
    return set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
