"""float64 restatement of the training graph (test helper, not a test): the loss of DCSCN.py:334-365 built from
``dcscn_oracle.build_topology`` with torch autograd for the gradients, the dropout masks of the hash documented in
include/dcscn.h, and TF's clipping and update rules (DCSCN.py:379-413) in numpy float64."""

import numpy as np
import torch
import torch.nn.functional as F

import dcscn_oracle as O

def splitmix64(z):
    """splitmix64 on uint64 numpy values (wrapping arithmetic), as include/dcscn.h states it."""
    with np.errstate(over="ignore"):
        z = np.asarray(z, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def layer_key(key, layer):
    with np.errstate(over="ignore"):
        return splitmix64(np.uint64(key) + np.uint64(0x9E3779B97F4A7C15) * np.uint64(layer + 1))


def dropout_mask(key, layer, shape, keep):
    """Kept units (bool, NHWC ``shape``) of conv layer ``layer`` (dcscn_layer_info order)."""
    thresh = np.uint64(int(np.floor(keep * 2 ** 24)))
    idx = np.arange(int(np.prod(shape)), dtype=np.uint64).reshape(shape)
    return (splitmix64(layer_key(key, layer) ^ idx) >> np.uint64(40)) < thresh


def _act(z, kind, alpha):
    if kind is None or kind == "":
        return z
    if kind == "prelu":
        return torch.where(z > 0, z, alpha.view(1, -1, 1, 1) * z)
    if kind == "relu":
        return torch.where(z > 0, z, torch.zeros_like(z))
    if kind == "leaky_relu":
        return torch.where(z > 0, z, 0.1 * z)
    if kind == "sigmoid":
        return torch.sigmoid(z)
    if kind == "tanh":
        return torch.tanh(z)
    if kind == "selu":
        return 1.0507009873554805 * torch.where(z > 0, z, 1.6732632423543772 * (torch.exp(torch.clamp(z, max=0)) - 1.0))
    raise NameError(kind)


def forward(cfg, leaves, x, x2, keep=1.0, key=0, dtype=torch.float64):
    """y_ of the training graph (torch, NCHW) from ``leaves`` {name: tensor}; x, x2 numpy NHWC."""
    t = {"x": torch.from_numpy(np.asarray(x, np.float64)).to(dtype).permute(0, 3, 1, 2),
         "x2": torch.from_numpy(np.asarray(x2, np.float64)).to(dtype).permute(0, 3, 1, 2)}
    layer = 0
    for op in O.build_topology(cfg):
        kind = op["op"]
        if kind == "conv":
            v, k = op["var"], op["k"]
            w = leaves[v + "/conv_W"].permute(3, 2, 0, 1).contiguous()     # (slow_conv2d's backward refuses some permuted views)
            h = F.conv2d(t[op["src"]], w, padding=k // 2)
            if op["bias"]:
                h = h + leaves[v + "/conv_B"].view(1, -1, 1, 1)
            if op["act"]:
                alpha = leaves.get(v + "/prelu/" + op["name"] + "_prelu")
                h = _act(h, op["act"], alpha)
                if keep < 1.0:
                    n, c, hh, ww = h.shape
                    m = dropout_mask(key, layer, (n, hh, ww, c), keep)
                    h = (h / keep) * torch.from_numpy(m.astype(np.float64)).to(dtype).permute(0, 3, 1, 2)
            t[op["dst"]] = h
            layer += 1
        elif kind == "concat":
            t[op["dst"]] = torch.cat([t[s] for s in op["srcs"]], dim=1)
        elif kind == "depth_to_space":
            t[op["dst"]] = F.pixel_shuffle(_tf_to_torch_d2s(t[op["src"]], op["block"]), op["block"])
        elif kind == "add":
            t[op["dst"]] = t[op["srcs"][0]] + t[op["srcs"][1]]
        else:
            raise ValueError(kind)
    return t["y_"]


def _tf_to_torch_d2s(h, b):
    """TF depth_to_space takes channel (i*b + j)*C + c; torch pixel_shuffle takes c*b*b + i*b + j: reorder."""
    n, cc, hh, ww = h.shape
    c = cc // (b * b)
    return h.view(n, b * b, c, hh, ww).transpose(1, 2).reshape(n, cc, hh, ww)


def loss_and_grads(cfg, weights, x, x2, y_true, keep=1.0, key=0, l1=False, l2_decay=0.0, dtype=torch.float64):
    """(stats dict, {name: gradient as float64}) of loss = image_loss + l2_decay * sum 0.5 ||conv_W||^2; ``dtype`` float32
    gives the same graph in torch float32 (the yardstick a failing parity test prints)."""
    leaves = {k: torch.tensor(np.asarray(v, np.float64), dtype=dtype, requires_grad=True) for k, v in weights.items()}
    y = forward(cfg, leaves, x, x2, keep, key, dtype)
    diff = y - torch.from_numpy(np.asarray(y_true, np.float64)).to(dtype).permute(0, 3, 1, 2)
    mse = torch.mean(diff * diff)
    image = torch.mean(torch.abs(diff)) if l1 else mse
    l2 = sum(0.5 * torch.sum(v * v) for k, v in leaves.items() if k.endswith("/conv_W"))
    loss = image + l2_decay * l2
    loss.backward()
    grads = {k: v.grad.numpy().astype(np.float64) for k, v in leaves.items()}
    return dict(image_loss=image.item(), mse=mse.item(), loss=loss.item()), grads


def clip_factor(grads, clipping_norm):
    norm = np.sqrt(sum(float(np.sum(np.asarray(g, np.float64) ** 2)) for g in grads.values()))
    return (clipping_norm / max(norm, clipping_norm) if clipping_norm > 0 else 1.0), norm


def adam(w, g, m, v, b1p, b2p, lr, b1=0.9, b2=0.999, eps=1e-8):
    """TF ApplyAdam with epsilon hat; b1p, b2p = beta powers of this step. Returns (w, m, v)."""
    lr_t = lr * np.sqrt(1.0 - b2p) / (1.0 - b1p)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    return w - lr_t * m / (np.sqrt(v) + eps), m, v


def momentum(w, g, a, lr, mu):
    a = mu * a + g
    return w - lr * a, a


def gd(w, g, lr):
    return w - lr * g
