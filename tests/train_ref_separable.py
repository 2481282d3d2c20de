"""float64 restatement of the training graph of the depthwise-separable nets (test helper, not a test): tests/train_ref.py's graph with the
``ds`` ops of ``dcscn_oracle.build_topology`` understood -- tf.nn.separable_conv2d (tf_graph.py:155-177) is a grouped k x k conv2d (one
filter per input channel, SAME) followed by a 1x1 conv, then bias, activator and dropout as for a plain conv, with ONE dropout layer
number per separable layer.  The extra reconstruction layers are plain convs even in a separable net.  The l2 term sums ``conv_W`` leaves
only: the reference's l2_loss covers a separable layer's unused conv_W, never depthwise_W or pointwise_W, and the library does not hold
those unused tensors (include/dcscn.h, known departure).  Activators, masks, depth_to_space and the update rules are train_ref's."""

import numpy as np
import torch
import torch.nn.functional as F

import dcscn_oracle as O
from conftest import CONFIGS, synthetic_batch
from train_ref import _act, _tf_to_torch_d2s, dropout_mask

L2_DECAY = 1e-3          # large enough that a decay wrongly applied to pointwise_W or depthwise_W misses the gradient bar

# the three nets of tests/test_train_separable_hip.py
NETS = {
    "a": CONFIGS["L7_F32to8_x4_DS"],
    "b": dict(CONFIGS["L7_F32to8_x4_DS"], scale=2),
    # 5x5 depthwise, no NIN, a plain R-CNN1 inside a separable net
    "c": dict(scale=3, layers=3, filters=12, min_filters=6, cnn_size=5, activator="relu", use_nin=False, reconstruct_layers=2,
              reconstruct_filters=6, depthwise_separable=True),
}
# (net, n, h, w, seed, keep, l1) of every gradient comparison the GPU file makes; the host file checks for each of them that torch float32
# is within 2e-5 of the largest float64 value of every tensor's gradient, so that the GPU's 1e-4 bar does not sit next to plain float32
# rounding on a cancellation-prone scalar (R-CNN1/pointwise_W is a single number: net a, seed 0, keep 0.8 is 5.6e-5 off in torch float32
# and is not used).
MAIN_CASES = [("a", 2, 12, 16, 0, 1.0, False), ("b", 3, 24, 28, 0, 1.0, False), ("c", 2, 13, 17, 0, 1.0, False),
              ("a", 2, 12, 16, 0, 1.0, True), ("a", 2, 12, 16, 1, 0.8, False)]
# 1x1, 2x3 and 5x4 patches with n = 1, and one batch whose pixel count no depthwise split divides (dw_splits below)
EDGE_CASES = [(net, 1, h, w, 1, 1.0, False) for net in ("b", "c") for h, w in ((1, 1), (2, 3), (5, 4))] + [("b", 1, 23, 29, 1, 1.0, False)]
KEY = 0x1234567


def net(name):
    cfg = O.make_config(**NETS[name])
    return cfg


def batch(cfg, n, h, w, seed):
    """synthetic_batch(seed) with a target the net does not already produce: x2 + N(0, 8)."""
    x, x2 = synthetic_batch(n, h, w, cfg["scale"], seed=seed)
    y = (x2 + np.random.default_rng(seed + 100).normal(0, 8, x2.shape)).astype(np.float32)
    return x, x2, y


def case_inputs(case):
    """(cfg, weights, x, x2, y) of a case: synthetic_weights(seed), batch(seed + 1)."""
    name, n, h, w, seed, keep, l1 = case
    cfg = net(name)
    return (cfg, O.synthetic_weights(cfg, seed=seed)) + batch(cfg, n, h, w, seed + 1)


def dw_splits(cin, pixels):
    """(splits, pixels per split) of the depthwise weight gradient (train_dw.hpp: dw_splits), fixed by the shape alone."""
    cw = 1
    while cw < cin and cw < 64:
        cw *= 2
    per = (256 // cw) * 32
    s = max(1, min(128, (pixels + per - 1) // per))
    chunk = (pixels + s - 1) // s
    return (pixels + chunk - 1) // chunk, chunk


def wgrad_splits(ks, cin, cout, pixels, ds=False):
    """(splits, pixels per split) of a GEMM layer's weight gradient (train.hip: wgrad_splits), fixed by the shape alone.  ``ks`` is the
    kernel size of the GEMM: 1 for a separable layer's pointwise filter (``ds``), k = 2 s - s % 2 with cin = cout = C for Up-TCNN, whose
    pixels are the LR ones."""
    tiles = ((ks * ks * cin + 31) // 32) * ((cout + 31) // 32)
    by_tiles = (2048 + tiles - 1) // tiles
    if ds:
        s = max(1, min(by_tiles, 256, (pixels + 511) // 512))
    else:
        s = max(1, min(by_tiles, (pixels + 1023) // 1024))
    chunk = ((pixels + s - 1) // s + 15) // 16 * 16
    return (pixels + chunk - 1) // chunk, chunk


def forward(cfg, leaves, x, x2, keep=1.0, key=0, dtype=torch.float64):
    """y_ of the training graph (torch, NCHW) from ``leaves`` {name: tensor}; x, x2 numpy NHWC."""
    t = {"x": torch.from_numpy(np.asarray(x, np.float64)).to(dtype).permute(0, 3, 1, 2),
         "x2": torch.from_numpy(np.asarray(x2, np.float64)).to(dtype).permute(0, 3, 1, 2)}
    layer = 0
    for op in O.build_topology(cfg):
        kind = op["op"]
        if kind == "conv":
            v, k = op["var"], op["k"]
            if op["ds"]:
                dw = leaves[v + "/depthwise_W"].permute(2, 3, 0, 1).contiguous()          # [k, k, cin, 1] -> [cin, 1, k, k]
                d = F.conv2d(t[op["src"]], dw, padding=k // 2, groups=op["cin"])
                h = F.conv2d(d, leaves[v + "/pointwise_W"].permute(3, 2, 0, 1).contiguous())
            else:
                h = F.conv2d(t[op["src"]], leaves[v + "/conv_W"].permute(3, 2, 0, 1).contiguous(), padding=k // 2)
            if op["bias"]:
                h = h + leaves[v + "/conv_B"].view(1, -1, 1, 1)
            if op["act"]:
                h = _act(h, op["act"], leaves.get(v + "/prelu/" + op["name"] + "_prelu"))
                if keep < 1.0:
                    n, c, hh, ww = h.shape
                    m = dropout_mask(key, layer, (n, hh, ww, c), keep)
                    h = (h / keep) * torch.from_numpy(m.astype(np.float64)).to(dtype).permute(0, 3, 1, 2)
            t[op["dst"]] = h
            layer += 1                                                                    # one number per layer, separable or not
        elif kind == "concat":
            t[op["dst"]] = torch.cat([t[s] for s in op["srcs"]], dim=1)
        elif kind == "depth_to_space":
            t[op["dst"]] = F.pixel_shuffle(_tf_to_torch_d2s(t[op["src"]], op["block"]), op["block"])
        elif kind == "add":
            t[op["dst"]] = t[op["srcs"][0]] + t[op["srcs"][1]]
        else:
            raise ValueError(kind)
    return t["y_"]


def loss(cfg, leaves, x, x2, y_true, keep=1.0, key=0, l1=False, l2_decay=0.0, dtype=torch.float64):
    """(total loss, image loss, mse) as torch scalars."""
    y = forward(cfg, leaves, x, x2, keep, key, dtype)
    diff = y - torch.from_numpy(np.asarray(y_true, np.float64)).to(dtype).permute(0, 3, 1, 2)
    mse = torch.mean(diff * diff)
    image = torch.mean(torch.abs(diff)) if l1 else mse
    l2 = sum(0.5 * torch.sum(v * v) for k, v in leaves.items() if k.endswith("/conv_W"))
    return image + l2_decay * l2, image, mse


def loss_and_grads(cfg, weights, x, x2, y_true, keep=1.0, key=0, l1=False, l2_decay=0.0, dtype=torch.float64):
    """(stats dict, {name: gradient as float64}) of loss = image_loss + l2_decay * sum over conv_W of 0.5 ||conv_W||^2."""
    leaves = {k: torch.tensor(np.asarray(v, np.float64), dtype=dtype, requires_grad=True) for k, v in weights.items()}
    total, image, mse = loss(cfg, leaves, x, x2, y_true, keep, key, l1, l2_decay, dtype)
    total.backward()
    grads = {k: v.grad.numpy().astype(np.float64) for k, v in leaves.items()}
    return dict(image_loss=image.item(), mse=mse.item(), loss=total.item()), grads


_REF = {}


def reference(case):
    """(stats, float64 gradients) of a case at L2_DECAY and KEY: computed once, shared by the tests that need it, never changed."""
    if case not in _REF:
        cfg, weights, x, x2, y = case_inputs(case)
        _REF[case] = loss_and_grads(cfg, weights, x, x2, y, keep=case[5], key=KEY, l1=case[6], l2_decay=L2_DECAY)
    return _REF[case]
