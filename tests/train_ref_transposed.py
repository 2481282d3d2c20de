"""float64 restatement of the training graph of the transposed-conv nets (test helper, not a test): tests/train_ref_separable.py's graph
with the ``conv_transpose`` op of ``dcscn_oracle.build_topology`` understood -- build_transposed_conv (tf_graph.py:219-236) is
``F.conv_transpose2d(src, W.permute(3, 2, 0, 1), stride=s, padding=(k - s) // 2)`` on the filter ``Tconv_W`` [k, k, out, in], with no bias,
no activator and no dropout of its own.  The op still advances the dropout layer number: a layer's number is its position in
``dcscn_layer_info`` order, and Up-TCNN is a layer there.  The l2 term sums the leaves ending in ``/conv_W`` or ``/Tconv_W``: the
reference appends Tconv_W to ``self.Weights`` (tf_graph.py:235), which DCSCN.py:350 sums.  Everything else is train_ref_separable's."""

import numpy as np
import torch
import torch.nn.functional as F

import dcscn_oracle as O
from conftest import CONFIGS
from train_ref import _act, _tf_to_torch_d2s, dropout_mask
from train_ref_separable import batch

L2_DECAY = 1e-3          # large enough that a decay missing from Tconv_W misses the gradient bar (tests/test_train_transposed_host.py)
KEY = 0x1234567

NETS = {
    # x2, C = 14: a ragged k-step of 4
    "t2": dict(layers=3, filters=16, min_filters=8, nin_filters=9, nin_filters2=5),
    # x3, k = 5, the one-tap phase, an activated R-CNN1 behind the layer
    "t3": dict(scale=3, layers=3, filters=12, min_filters=6, cnn_size=5, activator="relu", use_nin=False, reconstruct_layers=2,
               reconstruct_filters=6),
    # x4, k = 8, C = 76: three column tiles; layers eligible for split16
    "t4": dict(scale=4, layers=2, filters=40, min_filters=36, use_nin=False, legacy_no_c=True),
    # a separable net, C = 32: both options
    "tds": dict(CONFIGS["L7_F32to8_x4_DS"], scale=2),
    # dropout on a layer numbered after Up-TCNN
    "t2r": dict(layers=2, filters=12, min_filters=8, nin_filters=8, nin_filters2=4, reconstruct_layers=2, reconstruct_filters=8),
}
# (net, n, h, w, seed, keep, l1) of every gradient comparison the GPU file makes; the host file checks the float32 margin of each
MAIN_CASES = [("t2", 2, 12, 16, 0, 1.0, False), ("t3", 2, 13, 17, 0, 1.0, False), ("t4", 2, 9, 11, 0, 1.0, False),
              ("tds", 2, 12, 16, 0, 1.0, False), ("t2r", 2, 12, 16, 1, 0.8, False), ("t2", 2, 12, 16, 0, 1.0, True)]
# 1 x 1 (every off-centre tap is outside), thin and small patches, and 23 x 29 = 667 pixels, which no tile or split divides
EDGE_CASES = [(net, 1, 1, 1, 1, 1.0, False) for net in ("t2", "t3", "t4")] + \
             [("t3", 1, 2, 3, 1, 1.0, False), ("t3", 1, 1, 7, 1, 1.0, False), ("t4", 1, 5, 4, 1, 1.0, False), ("t2", 1, 23, 29, 1, 1.0, False)]


def case_id(c):
    return "%s-n%d-%dx%d-s%d-k%g-l1%d" % c


def net(name):
    return O.make_config(**dict(NETS[name], pixel_shuffler=False))


def case_inputs(case):
    """(cfg, weights, x, x2, y) of a case: synthetic_weights(seed), batch(seed + 1)."""
    name, n, h, w, seed, keep, l1 = case
    cfg = net(name)
    return (cfg, O.synthetic_weights(cfg, seed=seed)) + batch(cfg, n, h, w, seed + 1)


def is_l2_leaf(name):
    return name.endswith("/conv_W") or name.endswith("/Tconv_W")


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
            layer += 1
        elif kind == "conv_transpose":
            w, s = leaves[op["var"] + "/Tconv_W"], op["scale"]                            # [k, k, out, in] -> torch's [in, out, k, k]
            t[op["dst"]] = F.conv_transpose2d(t[op["src"]], w.permute(3, 2, 0, 1).contiguous(), stride=s, padding=(w.shape[0] - s) // 2)
            layer += 1                                                                    # Up-TCNN is a layer of dcscn_layer_info: it takes a number
        elif kind == "concat":
            t[op["dst"]] = torch.cat([t[s] for s in op["srcs"]], dim=1)
        elif kind == "depth_to_space":
            t[op["dst"]] = F.pixel_shuffle(_tf_to_torch_d2s(t[op["src"]], op["block"]), op["block"])
        elif kind == "add":
            t[op["dst"]] = t[op["srcs"][0]] + t[op["srcs"][1]]
        else:
            raise ValueError(kind)
    return t["y_"]


def loss(cfg, leaves, x, x2, y_true, keep=1.0, key=0, l1=False, l2_decay=0.0, dtype=torch.float64, l2_leaf=is_l2_leaf):
    """(total loss, image loss, mse) as torch scalars."""
    y = forward(cfg, leaves, x, x2, keep, key, dtype)
    diff = y - torch.from_numpy(np.asarray(y_true, np.float64)).to(dtype).permute(0, 3, 1, 2)
    mse = torch.mean(diff * diff)
    image = torch.mean(torch.abs(diff)) if l1 else mse
    l2 = sum(0.5 * torch.sum(v * v) for k, v in leaves.items() if l2_leaf(k))
    return image + l2_decay * l2, image, mse


def loss_and_grads(cfg, weights, x, x2, y_true, keep=1.0, key=0, l1=False, l2_decay=0.0, dtype=torch.float64, l2_leaf=is_l2_leaf):
    """(stats dict, {name: gradient as float64}) of loss = image_loss + l2_decay * sum over the l2 leaves of 0.5 ||W||^2."""
    leaves = {k: torch.tensor(np.asarray(v, np.float64), dtype=dtype, requires_grad=True) for k, v in weights.items()}
    total, image, mse = loss(cfg, leaves, x, x2, y_true, keep, key, l1, l2_decay, dtype, l2_leaf)
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
