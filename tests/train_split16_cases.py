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

# The edge cases of tests/test_train_split16_edges_hip.py (tests/test_train_split16_edges_host.py classifies their convs together with
# CASES above).  Schedule 48, 32, 24: the concat buffer has stride 104, CNN3 reads a 16-byte-aligned slice at offset 48, A1 and B1 have
# K = 104 (three chunks of 32 and 8), Up-PS is 48 -> 64 (exactly one column group) and Concat2 = [B2 | A1] has stride 48
ALIGNED = dict(layers=3, filters=48, min_filters=24, nin_filters=32, nin_filters2=16, scale=2, pixel_shuffler_filters=16)
#             name                 net      (n, h, w)
EDGE_SHAPES = {
    "odd-2x7x9":         (ODD,     (2, 7, 9)),       # magnitudes, zero / tiny / non-finite tensors, the maximum's place in a filter
    "odd-1x1x150":       (ODD,     (1, 1, 150)),     # one row: an outlier pixel stays inside one chunk of the reduction
    "odd-3x7x9":         (ODD,     (3, 7, 9)),       # shards 2 + 1
    "odd-5x8x8":         (ODD,     (5, 8, 8)),       # the patch route: 5 patches of 8 x 8
    "aligned-2x8x8":     (ALIGNED, (2, 8, 8)),
    "aligned-1x72x71":   (ALIGNED, (1, 72, 71)),     # 5112 pixels x 104 channels: past the reduction's block clamp
    "aligned-1x1x5112":  (ALIGNED, (1, 1, 5112)),    # the same count in one row
}
EDGE_KEEP = 0.8
ABS_MAX_BLOCKS, ABS_MAX_CHUNK = 256, 2048           # kAbsMaxBlocks and launch_texp's elements per block (csrc/train_h.hip)


def texp_partition(count):
    """(blocks, chunk) of launch_texp for a tensor of ``count`` elements: ceil(count / 2048) blocks clamped to [1, 256], each over
    chunk = ceil(count / blocks) consecutive elements of the flat [row][column] order."""
    blocks = min(max(-(-count // ABS_MAX_CHUNK), 1), ABS_MAX_BLOCKS)
    return blocks, -(-count // blocks)


def split16_exponent(top):
    """texp_final's exponent for a tensor whose largest magnitude is ``top`` (as float32): 13 - floor(log2 top) clamped to +-126 (a
    subnormal maximum has the exponent field 0), 0 for an all-zero tensor."""
    m = int(np.float32(top).view(np.uint32)) & 0x7fffffff
    return 0 if m == 0 else int(np.clip(13 - ((m >> 23) - 127), -126, 126))


# +-40 and +-60 carry B2's input exponent to -56 and B1's dz exponent to 84, but e_in + e_w no further than 100 (B2's data gradient at
# k = 60); +-90 carry it to 130, past what a constructed power of two can undo, with gradient tensors whose maxima run from 7e-30 to 4e27: from the float64
# activations, asserted in tests/test_train_split16_edges_host.py
REBALANCE = (40, -40, 60, -60, 90, -90)


def rebalanced(weights, k):
    """B1 (1x1) feeds only B2 (3x3) through a PReLU, which is positively homogeneous: B1's filter and bias times 2^k and B2's filter
    times 2^-k leave the net's function and every other gradient unchanged, exactly, while nothing leaves the float32 range."""
    out = dict(weights)
    out["B1/conv_W"], out["B1/conv_B"] = np.ldexp(weights["B1/conv_W"], k), np.ldexp(weights["B1/conv_B"], k)
    out["B2/conv_W"] = np.ldexp(weights["B2/conv_W"], -k)
    return out


def undo_rebalancing(grads, k):
    """The gradients at rebalanced(weights, k) brought back to those at k = 0 (exact: powers of two)."""
    out = dict(grads)
    out["B1/conv_W"], out["B1/conv_B"] = np.ldexp(grads["B1/conv_W"], k), np.ldexp(grads["B1/conv_B"], k)
    out["B2/conv_W"] = np.ldexp(grads["B2/conv_W"], -k)
    return out


OUTLIER = 64.0      # times the tensor's largest magnitude: with the scale the rest sets it lands at 2^19 or above, past the f16 maximum


def filter_outlier(weights, layer, index):
    """``weights`` with the element at flat ``index`` of the layer's filter set to OUTLIER times the filter's largest magnitude."""
    out = dict(weights)
    w = weights[layer + "/conv_W"].copy()
    w.reshape(-1)[index] = np.float32(OUTLIER) * np.max(np.abs(w))
    out[layer + "/conv_W"] = w
    return out


def filter_positions(count):
    """The flat indices at which the reduction over a filter can lose its maximum: the ends and both sides of the first chunk boundary."""
    blocks, chunk = texp_partition(count)
    assert blocks > 1
    return {"first": 0, "last": count - 1, "chunk-end": chunk - 1, "chunk-start": chunk}


def pixel_outlier(x, x2, y, where):
    """(x, x2, y) with one LR pixel of x set to OUTLIER * 255 ("x-first", "x-last") or one HR pixel of y moved by as much ("y-first",
    "y-last"): the first or the last pixel of the batch."""
    x, y = x.copy(), y.copy()
    a = x if where[0] == "x" else y
    i = (0, 0, 0, 0) if where.endswith("first") else (-1, -1, -1, 0)
    a[i] = (0.0 if a is x else a[i]) + np.float32(OUTLIER * 255.0)
    return x, x2, y


def blocks_of_the_maxima(cfg, weights, x, x2, y, keep, key, layer="A1"):
    """Where launch_texp's partition finds the largest magnitudes of ``layer``'s input slice and of its dz, from the float64 activations:
    ((block of the argmax, blocks) of the input slice, the same of dz).  ``layer`` reads the concat of the feature layers."""
    feats = [op["var"] for op in O.build_topology(cfg) if op["op"] == "conv" and op["var"].startswith("CNN")]
    taps = {k: None for k in feats + [layer]}
    R.loss_and_grads(cfg, weights, x, x2, y, keep=keep, key=key, l2_decay=L2_DECAY, taps=taps)
    out = []
    for a in (np.concatenate([taps[k]["out"] for k in feats], axis=-1), taps[layer]["dz"]):
        blocks, chunk = texp_partition(a.size)
        out.append((int(np.argmax(np.abs(a))) // chunk, blocks))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def edge_inputs(name, act="prelu"):
    """(cfg, weights, x, x2, y) of an edge shape: synthetic weights seed 0, the batch of test_train_hip._batch seed 1."""
    over, (n, h, w) = EDGE_SHAPES[name]
    cfg = O.make_config(**dict(over, activator=act))
    return (cfg, O.synthetic_weights(cfg, seed=0)) + tuple(_batch(cfg, n, h, w, 1))


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
