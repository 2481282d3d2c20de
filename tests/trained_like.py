"""Weights with the value statistics of the trained checkpoints, on nets that have no checkpoint (test helper, not a test); shared
by tests/test_trained_like_host.py, tests/test_trained_like_hip.py and tests/test_train_trained_like_hip.py.

``oracle.synthetic_weights`` draws PReLU slopes from U(0.05, 0.3), biases from N(0, 0.1) and He filters of one magnitude per layer.
On slopes in (0, 1) the forms ``v > 0 ? v : a v``, ``max(v, a v)``, ``v + (a - 1) min(v, 0)`` and PReLU with the slope clamped to
[0, 1] are the same function, so an epilogue rewritten as one of them passes every test that uses those weights.  The three trained
L7 checkpoints under tests/golden/ have 513 slopes in -5.84 .. 1.61 (59 negative, 5 above 1) and 658 biases in -35.3 .. 23.9;
``trained_like_weights`` resamples the slopes and biases of any net from these pools and, with ``spread``, gives the output channels
of a layer magnitudes up to 2^spread apart (the trained nets show up to 9.5 within one layer) and one constant channel per layer.

The two mutant activators are what the host file proves the weights can see; the case tables are what the three files share."""
import contextlib
import os

import numpy as np

from conftest import CONFIGS, GOLDEN
import dcscn_oracle as O
import train_split16_cases as C

POOL_FILES = ("weights_L7_x2.npz", "weights_L7_x3.npz", "weights_L7_x4.npz")
SPREAD = 3                              # channel magnitudes up to 2^3 = 8 apart; 9.5 is the largest ratio in the pooled checkpoints
SPREADS = (0, SPREAD)
# The second word of the generator's seed.  It is the first of 1, 2, ... with which both mutants move every inference case by
# 1000 x BAR (tests/test_trained_like_host.py).  Only the separable x4 net with spread 3 depends on it: its branch is 10 against
# intermediates of 1400 and biases of std 8.5, and about half the words leave the max form at 240 .. 950 x BAR there (1 .. 4: 410, 408,
# 718, 244); with each of those four words it was the weakest case of the table for both mutants.
STREAM = 5


def pools():
    """(slopes, biases) of POOL_FILES as float32 vectors: files in that order, keys sorted, arrays flattened."""
    slopes, biases = [], []
    for f in POOL_FILES:
        with np.load(os.path.join(GOLDEN, f)) as z:
            for k in sorted(z.files):
                if "/prelu/" in k:
                    slopes.append(z[k].astype(np.float32).ravel())
                elif k.endswith("/conv_B"):
                    biases.append(z[k].astype(np.float32).ravel())
    return np.concatenate(slopes), np.concatenate(biases)


def trained_like_weights(cfg, seed, spread=0):
    """``oracle.synthetic_weights(cfg, seed)`` with, from one generator seeded by ``seed``:

    slopes    every /prelu/ tensor drawn with replacement from the slope pool; a tensor of 4 or more channels starts with the pool's
              minimum, its maximum, 0.0 and 1.0;
    biases    every conv_B drawn with replacement from the bias pool;
    spread    (``spread`` > 0) every conv_W / pointwise_W but the last reconstruction conv's has output channel c multiplied by
              2^-k_c, k_c an integer of [0, spread] (exact in float32), and where it has 8 or more output channels one of them set to
              zero: that channel is its bias everywhere.  depthwise_W and Tconv_W have no output channels of their own and stay."""
    slopes, biases = pools()
    weights = O.synthetic_weights(cfg, seed=seed)
    rng = np.random.default_rng([seed, STREAM])
    last = "R-CNN%d/" % cfg["reconstruct_layers"]
    for name in sorted(weights):                    # slopes and biases first: they do not depend on ``spread``
        w = weights[name]
        if "/prelu/" in name:
            a = rng.choice(slopes, size=w.shape)
            if a.size >= 4:
                a[:4] = (slopes.min(), slopes.max(), 0.0, 1.0)
            weights[name] = a.astype(np.float32)
        elif name.endswith("/conv_B"):
            weights[name] = rng.choice(biases, size=w.shape).astype(np.float32)
    for name in sorted(weights):
        w = weights[name]
        if spread > 0 and name.endswith(("/conv_W", "/pointwise_W")) and not name.startswith(last):
            cout = w.shape[3]
            w = np.ldexp(w, -rng.integers(0, spread + 1, cout).astype(np.int32))
            if cout >= 8:
                w[..., int(rng.integers(0, cout))] = 0.0
            weights[name] = w.astype(np.float32)
    return weights


# ---- mutant activators: what a "simplified" epilogue would compute ---------------------------------------------------------------
def _numpy_max(orig):
    return lambda x, kind, alpha=None: np.maximum(x, alpha * x) if kind == "prelu" else orig(x, kind, alpha)


def _numpy_clamp(orig):
    return lambda x, kind, alpha=None: orig(x, kind, np.clip(alpha, 0.0, 1.0) if kind == "prelu" else alpha)


def _torch_max(orig):
    import torch
    return lambda z, kind, alpha: torch.maximum(z, alpha.view(1, -1, 1, 1) * z) if kind == "prelu" else orig(z, kind, alpha)


def _torch_clamp(orig):
    return lambda z, kind, alpha: orig(z, kind, alpha.clamp(0.0, 1.0) if kind == "prelu" else alpha)


MUTANTS = {"max": (_numpy_max, _torch_max), "clamp": (_numpy_clamp, _torch_clamp)}


@contextlib.contextmanager
def mutant(name, oracle=None, train_ref=None):
    """Within the block ``oracle.activate`` and / or ``train_ref._act`` compute PReLU as max(v, a v) ("max") or with the slope
    clamped to [0, 1] ("clamp"); every other activator is untouched."""
    saved = []
    for module, attr, make in ((oracle, "activate", MUTANTS[name][0]), (train_ref, "_act", MUTANTS[name][1])):
        if module is not None:
            saved.append((module, attr, getattr(module, attr)))
            setattr(module, attr, make(getattr(module, attr)))
    try:
        yield
    finally:
        for module, attr, orig in saved:
            setattr(module, attr, orig)


# ---- inference cases --------------------------------------------------------------------------------------------------------------
BARE_SEED = 0                           # trained_like_weights(cfg, 0, spread); the batch is bare_branch.bare_batch(..., seed 1)
NAMED_SHAPE = (17, 33)                  # the smallest that straddles the 16-pixel tiles in both directions
FLAG_SHAPE = (20, 28)                   # test_flag_surface's
_S16 = ("split16", 0)
WIDE = ("conv3_h", "conv_nin_h", "conv5_h")

# (net, flags, n, (h, w), [(plan, options set before load_weights, kernels the launch list must hold)])
NAMED_CASES = [
    ("L8_F96to48_x2", CONFIGS["L8_F96to48_x2"], 2, NAMED_SHAPE, [
        ("default", (), WIDE),
        ("split16 0", (_S16,), ("conv_wino2", "conv_nin")),
        ("split16 0 winograd 0", (_S16, ("winograd", 0)), ("conv_igemm", "conv_nin")),
        ("fold_linear_tail 0", (("fold_linear_tail", 0),), ("conv3_h", "conv_nin_h", "conv_cout1")),
        ("p16 0", (("p16", 0),), WIDE)]),
    ("L12_F196to48_x2", CONFIGS["L12_F196to48_x2"], 1, NAMED_SHAPE, [
        ("default", (), ("conv3_h8",) + WIDE),
        ("conv3_h8 0", (("conv3_h8", 0),), WIDE),
        ("nin_h8 0", (("nin_h8", 0),), ("conv3_h8",) + WIDE),
        ("split16 0", (_S16,), ("conv_wino2", "conv_nin"))]),
    ("L12_F196to48_x4", CONFIGS["L12_F196to48_x4"], 1, NAMED_SHAPE, [
        ("default", (), ("conv3_h8",) + WIDE),
        ("fold_whole_tail 0", (("fold_whole_tail", 0),), ("conv3_h8",) + WIDE),
        ("split16 0", (_S16,), ("conv_wino2", "conv_nin"))]),
    ("L7_F32to8_x3", CONFIGS["L7_F32to8_x3"], 2, NAMED_SHAPE, [
        ("stream_nin 0", (("stream_nin", 0),), ("feat3_stream", "conv_nin_h", "conv5_h")),
        ("stream_dense 0", (("stream_dense", 0),), ("conv_cin1", "conv3_h", "conv_igemm", "conv_nin_h")),
        ("split16 0", (_S16,), ("layer by layer",))]),
    ("L7_F32to8_x4_DS", CONFIGS["L7_F32to8_x4_DS"], 2, NAMED_SHAPE, [
        ("default", (), ("feat_stream", "conv5_h")),
        ("stream_tail 0", (("stream_tail", 0),), ("feat_stream",)),       # (the folded whole tail wins: the default's launch list)
        ("fold_whole_tail 0", (("fold_whole_tail", 0),), ("feat_stream", "tail_stream")),
        ("stream_features 0", (("stream_features", 0),), ("depthwise", "conv_igemm", "conv_nin_h")),
        ("split16 0", (_S16,), ("feat_stream", "tail_stream"))]),
]
# the dicts of test_hip_parity.test_flag_surface that change the kernel size, the reconstruction and the upsampler, each with the
# kernels both of its plans must hold
FLAG_VARIANTS = [
    ("k5", dict(layers=3, filters=20, min_filters=8, cnn_size=5), ("conv_cin1", "conv_igemm", "conv_cout1")),
    ("k7", dict(layers=2, filters=40, min_filters=24, cnn_size=7, nin_filters=20, nin_filters2=12), ("conv_cin1", "conv_igemm")),
    ("no-nin", dict(use_nin=False, layers=3, filters=20, min_filters=8), ()),
    ("reconstruct3", dict(layers=3, filters=24, min_filters=8, reconstruct_layers=3, reconstruct_filters=12), ("conv_cout1",)),
    ("transposed", dict(layers=3, filters=16, min_filters=8, pixel_shuffler=False), ("conv_igemm", "conv_cout1")),
    ("x3-ps1", dict(layers=3, filters=16, min_filters=8, scale=3, pixel_shuffler_filters=1), ()),
    ("separable-k5", dict(layers=2, filters=12, min_filters=8, cnn_size=5, depthwise_separable=True), ("depthwise", "conv_igemm")),
]
FLAG_CASES = [(name, flags, 2, FLAG_SHAPE, [("default", (), want), ("split16 0", (_S16,), want)]) for name, flags, want in FLAG_VARIANTS]
INFER_CASES = NAMED_CASES + FLAG_CASES
FULL_NETS = [c[:4] for c in NAMED_CASES]          # with the bicubic term and the attenuated last conv, at test_hip_parity.MAX_ABS_TOL
REBALANCE_NET, REBALANCE_K = "L8_F96to48_x2", (-4, 4)


def bare_case(flags, n, hw, spread):
    """(cfg, bare trained-like weights, x, x2 = 0) of an inference case."""
    import bare_branch as B
    cfg = O.make_config(**flags)
    weights = B.bare_weights(cfg, trained_like_weights(cfg, BARE_SEED, spread))
    x, x2 = B.bare_batch(n, hw[0], hw[1], cfg["scale"], BARE_SEED + 1)
    return cfg, weights, x, x2


# ---- training cases ---------------------------------------------------------------------------------------------------------------
TOL = C.TOL
L2_DECAY = C.L2_DECAY
KEEPS = (1.0, 0.8)
TRAIN_KEY = 0x7e57
# (net, flags, (n, h, w)): all PReLU, trained_like_weights(cfg, 0, spread), the batch of test_train_hip._batch seed 1
TRAIN_CASES = [
    ("odd", C.ODD, (2, 7, 9)),
    ("mixed", C.MIXED, (2, 8, 8)),
    ("k5", C.K5, (1, 6, 5)),
    ("x4r", C.X4R, (1, 5, 4)),
    ("L8_F96to48_x2", CONFIGS["L8_F96to48_x2"], (1, 13, 11)),
]
TRAIN_OPTIONS = [(s, g) for s in (0, 1) for g in (0, 1)]      # ("train_split16", "train_split16_wgrad")


def train_case(flags, nhw, spread, act="prelu"):
    """(cfg, weights, x, x2, y) of a training case."""
    cfg = O.make_config(**dict(flags, activator=act))
    return (cfg, trained_like_weights(cfg, 0, spread)) + tuple(C._batch(cfg, *nhw, 1))


# ---- exact zeros --------------------------------------------------------------------------------------------------------------------
# K5 without NIN (train_split16_cases.K5 has use_nin = False already) and ODD; image 0 of x is black and every bias is zero, so every
# pre-activation of that image is exactly 0 and its gradient is what the reference's graph gives AT the tie:
#   prelu       relu(z) + a (z - |z|) / 2:  ReluGrad passes features > 0, Abs has the gradient sign(z) = 0          -> dh/dz = a / 2
#   leaky_relu  tf.maximum(z, 0.1 z):       MaximumGrad sends x >= y to the first argument                        -> 1
#   selu        SeluGrad: outputs < 0 ? g (outputs + scale alpha) : scale g                                       -> 1.0507009873554805
#   relu        ReluGrad                                                                                            -> 0
# read from helper/tf_graph.py:82-96 and TensorFlow 1.x's registered gradients; TensorFlow itself was not run.
ZERO_NETS = [("k5", C.K5), ("odd", C.ODD)]
ZERO_ACTS = ("prelu", "leaky_relu", "selu", "relu")
ZERO_SHAPE = (2, 7, 9)


def zero_case(flags, act):
    """(cfg, weights, x, x2, y): trained_like_weights(cfg, 0) with every bias zero, the batch of test_train_hip._batch seed 1 with image 0
    of x black (x2 and y stay: the loss gradient of that image is not zero); selu takes x / 255 as everywhere."""
    cfg = O.make_config(**dict(flags, activator=act))
    weights = trained_like_weights(cfg, 0)
    for k in weights:
        if k.endswith("/conv_B"):
            weights[k] = np.zeros_like(weights[k])
    x, x2, y = C._batch(cfg, *ZERO_SHAPE, 1)
    x = x.copy()
    if act == "selu":
        x = x / np.float32(255.0)
    x[0] = 0.0
    return cfg, weights, x, x2, y
