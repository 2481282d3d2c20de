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
    """The activators as the reference writes them (helper/tf_graph.py:82-96), so that autograd takes at z == 0 the gradient the
    reference's graph takes under TensorFlow 1.x's registered gradients (ReluGrad: features > 0; Abs: sign(z); MaximumGrad: x >= y
    goes to the first argument; SeluGrad: outputs < 0, else scale): a / 2 for prelu, 1 for leaky_relu, the scale for selu, 0 for relu.
    This convention is derived from those registrations; it has not been run against TensorFlow.  For z != 0 the values and the
    gradients are those of ``where(z > 0, z, a z)``: 2 z, its product with a and the halving are exact."""
    if kind is None or kind == "":
        return z
    if kind == "prelu":
        return torch.relu(z) + alpha.view(1, -1, 1, 1) * (z - z.abs()) * 0.5
    if kind == "relu":
        return torch.relu(z)
    if kind == "leaky_relu":
        return torch.where(z >= 0.1 * z, z, 0.1 * z)
    if kind == "sigmoid":
        return torch.sigmoid(z)
    if kind == "tanh":
        return torch.tanh(z)
    if kind == "selu":
        return 1.0507009873554805 * torch.where(z < 0, 1.6732632423543772 * (torch.exp(torch.clamp(z, max=0)) - 1.0), z)
    raise NameError(kind)


def forward(cfg, leaves, x, x2, keep=1.0, key=0, dtype=torch.float64, taps=None):
    """y_ of the training graph (torch, NCHW) from ``leaves`` {name: tensor}; x, x2 numpy NHWC.  ``taps`` {conv variable prefix: anything}
    asks for those layers' tensors: the entry becomes (pre-activation, output after activator and dropout), torch NCHW, the first
    with its gradient retained."""
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
            z = h
            if taps is not None and v in taps and z.requires_grad:
                z.retain_grad()
            if op["act"]:
                alpha = leaves.get(v + "/prelu/" + op["name"] + "_prelu")
                h = _act(h, op["act"], alpha)
                if keep < 1.0:
                    n, c, hh, ww = h.shape
                    m = dropout_mask(key, layer, (n, hh, ww, c), keep)
                    h = (h / keep) * torch.from_numpy(m.astype(np.float64)).to(dtype).permute(0, 3, 1, 2)
            t[op["dst"]] = h
            if taps is not None and v in taps:
                taps[v] = (z, h)
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


def loss_and_grads(cfg, weights, x, x2, y_true, keep=1.0, key=0, l1=False, l2_decay=0.0, dtype=torch.float64, taps=None):
    """(stats dict, {name: gradient as float64}) of loss = image_loss + l2_decay * sum 0.5 ||conv_W||^2; ``dtype`` float32
    gives the same graph in torch float32 (the yardstick a failing parity test prints).  ``taps`` {conv variable prefix: anything},
    when given, is filled with dict(z=pre-activation, out=the layer's output, dz=the loss gradient of z) per named layer, float64
    numpy NHWC -- the tensors whose magnitudes option "train_split16" scales by."""
    leaves = {k: torch.tensor(np.asarray(v, np.float64), dtype=dtype, requires_grad=True) for k, v in weights.items()}
    y = forward(cfg, leaves, x, x2, keep, key, dtype, taps)
    diff = y - torch.from_numpy(np.asarray(y_true, np.float64)).to(dtype).permute(0, 3, 1, 2)
    mse = torch.mean(diff * diff)
    image = torch.mean(torch.abs(diff)) if l1 else mse
    l2 = sum(0.5 * torch.sum(v * v) for k, v in leaves.items() if k.endswith("/conv_W"))
    loss = image + l2_decay * l2
    loss.backward()
    grads = {k: v.grad.numpy().astype(np.float64) for k, v in leaves.items()}
    if taps is not None:
        nhwc = lambda a: a.detach().permute(0, 2, 3, 1).numpy().astype(np.float64)
        for k, (z, out) in taps.items():
            taps[k] = dict(z=nhwc(z), out=nhwc(out), dz=nhwc(z.grad))
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


# ---- dcscn_train_apply_records, restated operation by operation (include/dcscn.h "Data-parallel training") --------------------
# train.hip is compiled with fp contract(off): every multiply, add, divide and sqrt below is one IEEE operation with one rounding,
# in the order the kernels take them, so numpy float64 / float32 give the device's bits.

RECORD_TRAILER_FLOATS = 8
NORM_BLOCKS = 256                  # tsumsq's grid for the gradient norm (kNormBlocks)
# make_records seed per variable count, chosen so that reducing a world of 8 in reversed rank order changes at least one float32 bit
# of g (with and without the large values) and every one of the three float64 stats, and that summing its fractional counts from
# the last rank changes a weight: the float64 sum hides the order in g unless it lands next to a float32 rounding boundary
# (tests/test_train_parallel_host.py asserts all of it for each of them)
RECORD_SEEDS = {2604: 360, 27209: 18, 28654: 42, 1823: 1186}


def record_pad(count):
    return (count + 3) // 4 * 4


def make_records(count, world, seed, large=False, fractional=False, pad_value=12345.0):
    """[world, record_floats] float32 records filled on the host: gradients N(0,1) * 10^U(-6, 2) of mixed sign with a few planted
    elements (+-0, float32 subnormals, a pair that cancels across ranks 0 and 1, and with ``large`` values near the float32
    maximum whose weighted sum stays finite), uneven positive integer patch counts, random positive doubles in trailer slots
    0, 1 and 3, and ``pad_value`` (not zero) in the padding floats behind the gradient.  ``fractional`` scales every count by a
    random factor: integers this small add up exactly in any order, so only such counts show the order the counts are summed in."""
    rng = np.random.default_rng(seed)
    pad = record_pad(count)
    rec = np.full((world, pad + RECORD_TRAILER_FLOATS), pad_value, np.float32)
    g = (rng.standard_normal((world, count)) * 10.0 ** rng.uniform(-6.0, 2.0, (world, count))).astype(np.float32)
    sign = np.where(np.arange(world) % 2 == 0, 1.0, -1.0).astype(np.float32)
    e = np.sort(rng.choice(count, 8, replace=False))             # where the planted elements sit: anywhere in the record
    g[:, e[0]] = 0.0
    g[:, e[1]] = -0.0
    g[:, e[2]] = 0.0 * sign                                       # +0 and -0 mixed over the ranks
    g[:, e[3]] = np.float32(1e-45) * sign                         # the smallest float32 subnormal
    g[:, e[4]] = np.float32(3e-39)                                # subnormal on every rank
    g[:, e[5]] = 0.0
    g[0, e[5]] = 1.0
    if world > 1:
        g[1, e[5]] = np.float32(-1.0) + np.float32(2.0 ** -23)    # cancels against rank 0 down to the last bit, under unequal weights
    if large:
        g[:, e[6]] = np.float32(2.0e38)                           # a plain float32 sum overflows from world = 2 on; the weighted mean does not
        g[:, e[7]] = np.float32(1.5e38) * sign                    # (and the norm of both, 2.5e38, is still a float32)
    rec[:, :count] = g
    counts = np.array(([3, 2, 2, 1] + [int(v) for v in rng.integers(1, 6, max(world - 4, 0))])[:world], np.float64)
    tr = rng.uniform(0.5, 2000.0, (world, 4))
    if fractional:
        counts = counts * np.random.default_rng([seed, 1]).uniform(0.5, 1.5, world)
    tr[:, 2] = counts
    rec[:, pad:] = tr.view(np.float32)
    return rec


def record_parts(rec, count):
    """(gradients [world, count] float32, trailers [world, 4] float64) of records."""
    pad = record_pad(count)
    return rec[:, :count], np.ascontiguousarray(rec[:, pad:]).view(np.float64)


def rank_weights(counts, order=None):
    """w_r = n_r / sum n_r, the sum taken in rank order (trank_weights)."""
    counts = np.asarray(counts, np.float64)
    total = np.float64(0.0)
    for r in (range(len(counts)) if order is None else order):
        total = total + counts[r]
    return counts / total


def weighted_sum(values, w, order=None):
    """acc = w_0 * v_0, then acc = acc + w_r * v_r for r ascending, in float64 (treduce_ranks, tstats_ranks); ``order`` replaces
    the rank order (the host tests use it to show that the order is visible in the result)."""
    order = list(range(len(w))) if order is None else list(order)
    acc = w[order[0]] * np.asarray(values[order[0]], np.float64)
    for r in order[1:]:
        acc = acc + w[r] * np.asarray(values[r], np.float64)
    return acc


def _tree(r):
    """The LDS tree r[t] += r[t + o], o = 128 ... 1, over the last axis (256 wide); returns r[..., 0]."""
    r = np.array(r, np.float64)
    o = 128
    while o > 0:
        r[..., :o] = r[..., :o] + r[..., o:2 * o]
        o //= 2
    return r[..., 0]


def tree_sumsq(g):
    """Sum of squares of the float32 vector ``g`` in tsumsq's and tstats_ranks' order, as float64: NORM_BLOCKS blocks of
    chunk = ceil(count / NORM_BLOCKS) elements, thread t of a block adds the squares of elements t, t + 256, ... of its chunk
    in order, an LDS tree per block, then thread t of one block holds partial t and the same tree runs once more."""
    g = np.asarray(g, np.float32).ravel()
    count = g.size
    chunk = (count + NORM_BLOCKS - 1) // NORM_BLOCKS
    rows = (chunk + 255) // 256
    sq = g.astype(np.float64) * g.astype(np.float64)
    s = np.zeros((NORM_BLOCKS, 256), np.float64)
    base = np.arange(NORM_BLOCKS, dtype=np.int64)[:, None] * chunk
    for row in range(rows):
        inside = row * 256 + np.arange(256, dtype=np.int64)[None, :]
        idx = base + inside
        valid = (inside < chunk) & (idx < count)
        s = np.where(valid, s + sq[np.minimum(idx, count - 1)], s)
    return _tree(0.0 + _tree(s))


def reduce_records(rec, count, clipping_norm):
    """(g float32 [count], stats: [image_loss, mse, float32 norm, total loss], float32 clip factor) of dcscn_train_apply_records."""
    grads, tr = record_parts(rec, count)
    w = rank_weights(tr[:, 2])
    g = weighted_sum(grads, w).astype(np.float32)
    norm = np.float32(np.sqrt(tree_sumsq(g)))
    c = np.float32(clipping_norm)
    clip = c / max(norm, c) if clipping_norm > 0 else np.float32(1.0)
    stats = [weighted_sum(tr[:, 0], w), weighted_sum(tr[:, 1], w), norm, weighted_sum(tr[:, 3], w)]
    return g, stats, np.float32(clip)
