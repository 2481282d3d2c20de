"""The cases of tests/test_train_variants_surface_host.py and tests/test_train_variants_surface_hip.py (test helper, not a test): training
of the separable nets (option "train_separable") and of the transposed-conv nets (option "train_transposed") over the flag surface, the
weight-gradient splits of Up-TCNN, moved weights, re-carved arenas and uneven data-parallel shards.

The float64 reference of every case is tests/train_ref_transposed.py, whose ``forward`` restates ``ds`` convs, ``conv_transpose`` and
``depth_to_space``, that is all three kinds of net below; its l2 term sums ``conv_W`` and ``Tconv_W``, never ``depthwise_W`` or
``pointwise_W``.  Nothing here needs a GPU: the host file checks the generator's coverage and the margin that torch float32 autograd of
the same graph leaves under the GPU file's bar."""
import functools

import numpy as np
import torch

import dcscn_oracle as O
import train_ref_separable as S
import train_ref_transposed as T
from test_train_surface_hip import L2_DECAY, TRANSCENDENTAL, _draw, _ratios
from train_ref_separable import dw_splits, wgrad_splits  # noqa: F401 (re-exported)

FLAGS = dict(optimizer="adam", beta1=0.9, beta2=0.999, epsilon=1e-8, momentum=0.9, l2_decay=1e-4, clipping_norm=5.0,
             dropout_rate=1.0, use_l1_loss=False)
BAR = 1e-4                      # of max|g64|: the gradient bar of DESIGN.md section 8
F32_BAR = 2.5e-5                # the quarter of it that torch float32 has to meet on the host for a case to be used on the GPU

# ---------------------------------------------------------------------------------------------
# 1. the random walk: test_train_surface_hip._draw, then one more draw for the kind of net
# ---------------------------------------------------------------------------------------------
WALK_DRAWS = 200
WALK_RNG_BASE = 7000
KINDS = {0: dict(pixel_shuffler=True, depthwise_separable=True),       # separable, with the pixel shuffler
         1: dict(pixel_shuffler=False, depthwise_separable=False),     # transposed, dense convs
         2: dict(pixel_shuffler=False, depthwise_separable=True)}      # separable and transposed
# Draws that plain float32 does not carry: {draw: torch float32's worst max|g32 - g64| / max|g64| (tensor)}, measured on the host.  The host
# file asserts that each of them really exceeds F32_BAR and that every other draw meets it; at most 4 of the 200 may stand here.
WALK_EXCLUDED = {
    151: 2.5e-4,                # transposed x4, k 3, prelu, 3x16x14: Up-TCNN/Tconv_W
    185: 7.0e-5,                # separable x2, k 1, relu, 1x17x15: Up-PS/Up-PS_CNN/depthwise_W
}
WALK_KEPT = [seed for seed in range(WALK_DRAWS) if seed not in WALK_EXCLUDED]


def walk_draw(seed):
    """(kind, flags, n, h, w, l1, keep) of draw ``seed``."""
    rng = np.random.default_rng(WALK_RNG_BASE + seed)
    flags, n, h, w, l1, keep = _draw(rng)
    kind = int(rng.choice([0, 1, 2]))
    return kind, dict(flags, **KINDS[kind]), n, h, w, l1, keep


def walk_inputs(seed):
    """(cfg, weights, x, x2, y) of draw ``seed``: synthetic_weights(cfg, seed), batch(seed + 1), x / 255 for the transcendental activators."""
    _, flags, n, h, w, _, _ = walk_draw(seed)
    cfg = O.make_config(**flags)
    x, x2, y = S.batch(cfg, n, h, w, seed + 1)
    if cfg["activator"] in TRANSCENDENTAL:
        x = x / np.float32(255.0)
    return cfg, O.synthetic_weights(cfg, seed=seed), x, x2, y


def walk_context(seed):
    return "kind %d flags %r n %d h %d w %d l1 %r keep %r" % walk_draw(seed)


def float32_ratios(cfg, weights, x, x2, y, keep, key, l1, l2_decay):
    """({name: max|g32 - g64| / max|g64|} of torch float32 autograd against float64, the names whose float64 gradient is identically zero)."""
    _, g64 = T.loss_and_grads(cfg, weights, x, x2, y, keep=keep, key=key, l1=l1, l2_decay=l2_decay)
    _, g32 = T.loss_and_grads(cfg, {k: v.astype(np.float32) for k, v in weights.items()}, x, x2, y, keep=keep, key=key, l1=l1,
                              l2_decay=l2_decay, dtype=torch.float32)
    return _ratios(g32, g64), sorted(k for k, g in g64.items() if not np.any(g))


@functools.lru_cache(maxsize=None)
def walk_float32(seed):
    """float32_ratios of draw ``seed`` with the walk's settings (l2_decay 1e-3, dropout_key = seed): computed once."""
    _, _, _, _, _, l1, keep = walk_draw(seed)
    return float32_ratios(*walk_inputs(seed), keep=keep, key=seed, l1=l1, l2_decay=L2_DECAY)


def worst_nonzero(ratios, zeros):
    """(ratio, name) of the worst tensor whose float64 gradient is not identically zero."""
    name = max((k for k in ratios if k not in zeros), key=lambda k: ratios[k])
    return ratios[name], name


def depthwise_cins(cfg):
    return [op["cin"] for op in O.build_topology(cfg) if op["op"] == "conv" and op["ds"]]


def tconv_channels(cfg):
    """C of Up-TCNN, or None for a pixel-shuffler net."""
    for op in O.build_topology(cfg):
        if op["op"] == "conv_transpose":
            return op["channels"]
    return None


# ---------------------------------------------------------------------------------------------
# 2 - 5. directed cases on the nets of train_ref_transposed.NETS and net c of train_ref_separable, (net, n, h, w, seed, keep, l1)
# ---------------------------------------------------------------------------------------------
# more than one split of tup_wgrad: {case: (k, C, LR pixels, splits, chunk, pixels of the last split)}
SPLIT_CASES = {
    ("t3", 3, 19, 23, 1, 1.0, False): (5, 12, 1311, 2, 656, 655),      # the split boundary lies inside image 1
    ("t4", 2, 24, 27, 1, 1.0, False): (8, 76, 1296, 2, 656, 640),      # three column tiles
    ("t2", 3, 37, 40, 1, 1.0, False): (4, 14, 4440, 5, 896, 856),
    ("tds", 3, 19, 23, 1, 0.8, False): (4, 32, 1311, 2, 656, 655),     # separable, dropout
}
# shards (3, 2) and (2, 2, 1) of a 5 x 8 x 8 batch
SHARD_CASES = [("tds", 5, 8, 8, 0, 0.8, False), ("t2r", 5, 8, 8, 0, 0.8, False), ("t3", 5, 8, 8, 0, 0.8, True)]
SHARDS = [(3, 2), (2, 2, 1)]
# gradients after the weights have moved, and a new batch shape on one handle
MOVED_NETS = ["tds", "t3", "c"]
MOVED_STEP_SHAPE, MOVED_SHAPE, MOVED_SEED, MOVED_KEEP = (3, 20, 24), (2, 18, 22), 5, 0.8
RESHAPE_NETS = ["tds", "c"]
RESHAPE_SHAPES = [(4, 24, 24), (2, 40, 28), (3, 8, 8)]

case_id = T.case_id
reference = T.reference          # (stats, float64 gradients) of a case at T.L2_DECAY and T.KEY: computed once, shared, never changed
case_inputs = T.case_inputs


def net(name):
    """The config of a net of train_ref_transposed.NETS, or of net c of train_ref_separable (separable, x3, pixel shuffler)."""
    return T.net(name) if name in T.NETS else S.net(name)


@functools.lru_cache(maxsize=None)
def case_float32(case):
    """float32_ratios of a directed case at T.L2_DECAY and T.KEY: computed once."""
    return float32_ratios(*case_inputs(case), keep=case[5], key=T.KEY, l1=case[6], l2_decay=T.L2_DECAY)


def up_tcnn_splits(case):
    """(k, C, LR pixels, splits, chunk, pixels of the last split) of Up-TCNN's weight gradient on a case."""
    name, n, h, w = case[:4]
    cfg = net(name)
    s, c, pixels = cfg["scale"], tconv_channels(cfg), n * h * w
    k = 2 * s - s % 2
    splits, chunk = wgrad_splits(k, c, c, pixels)
    return k, c, pixels, splits, chunk, pixels - (splits - 1) * chunk


def moved_inputs(name):
    """(cfg, the weights set_train_tensor installs, x, x2, y) of the second comparison of the moved-weights test."""
    cfg = net(name)
    return (cfg, O.synthetic_weights(cfg, seed=MOVED_SEED)) + S.batch(cfg, *MOVED_SHAPE, 3)


def engine(cfg, weights, **flags):
    """A handle in training with the options its net needs: "train_transposed" without the pixel shuffler, "train_separable" for a
    separable net."""
    from dcscn_amd import engine as E
    eng = E.Engine(cfg, device=0)
    eng.load_weights(weights)
    if not cfg["pixel_shuffler"]:
        eng.set_option("train_transposed", 1)
    if cfg["depthwise_separable"]:
        eng.set_option("train_separable", 1)
    eng.train_begin(dict(FLAGS, **flags))
    return eng
