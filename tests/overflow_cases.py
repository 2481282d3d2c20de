"""Inputs whose FIRST value beyond the f16 range arises behind the input, shared by tests/test_overflow_host.py and
tests/test_overflow_hip.py.

The split16 path carries an activation as an f16 (hi, lo) pair, which works for |x| < 65520 (F16_EDGE: the first float32 whose f16
rounding is infinite); beyond it the launch that meets or produces the value raises the image's redo flag and the float32 plan
recomputes the image ("split16" in include/dcscn.h, csrc/split16.hpp).  The three tests older than this file multiply an input image by
4000, so the first split16 launch of the pass decides everything.  Here ONE conv of the net (the target) has its filter and bias
multiplied by 2^e, so that the hot image of the batch stays inside the range in every tensor in front of the target's output and
leaves it there; the other images stay inside everywhere.

The margins LIM_LO and LIM_HI keep the device's float32 values on the same side of the edge as the float64 oracle's: the worst per-layer
relative error on record is about 1e-6, so 1 % above and 10 % below are ample.  They are conditions of the construction, not measurements.

x2 is zero throughout and the last conv is not attenuated (tests/bare_branch.py): the output is the bare network branch, and the
bar, the error measure and the float32-restatement rule are that file's."""
import math

import numpy as np

from bare_branch import BAR, RESTATEMENT_FACTOR, bare_batch, bare_weights, rel_error, restatement_error, walk_draw  # noqa: F401 (re-exported)

F16_MAX = 65504.0
F16_EDGE = 65520.0
LIM_LO = 0.9 * F16_MAX
LIM_HI = 1.01 * F16_EDGE
HOT_FACTOR = 8.0                        # a hot IMAGE is the clean one times 8: its input stays below 2100
HOT_PIXEL = 0.85 * F16_MAX              # a hot PIXEL: inside the range itself, with nothing to spare behind a filter tap of 1.06

DIRECTED_EXPONENTS = range(-6, 14)
WALK_EXPONENTS = range(-8, 20)


def convs(oracle, cfg):
    """The conv ops of the topology, in graph order."""
    return [op for op in oracle.build_topology(cfg) if op["op"] == "conv"]


def conv_names(oracle, cfg):
    return [op["name"] for op in convs(oracle, cfg)]


def tensors_before(oracle, cfg, target):
    """Names of the tensors the graph holds before ``target``'s output exists: x and every op's output in front of it."""
    names = ["x"]
    for op in oracle.build_topology(cfg):
        if op["op"] == "conv" and op["name"] == target:
            return names
        names.append(op["dst"])
    raise KeyError(target)


def hot_input(x, hot):
    """``x`` with image ``hot`` times 8, or, for a triple (image, row, col), with that one LR pixel set to 0.85 * 65504."""
    xb = np.array(x, np.float32, copy=True)
    if isinstance(hot, tuple):
        i, r, c = hot
        xb[i, r, c, 0] = np.float32(HOT_PIXEL)
    else:
        xb[hot] *= np.float32(HOT_FACTOR)
    return xb


def hot_index(hot):
    return hot[0] if isinstance(hot, tuple) else hot


def scaled_weights(oracle, cfg, weights, target, e):
    """``weights`` with the target conv's conv_W (pointwise_W of a separable conv) and conv_B times 2^e: exact in float32."""
    op = [o for o in convs(oracle, cfg) if o["name"] == target][0]
    out = dict(weights)
    f = np.float32(math.ldexp(1.0, e))
    w = op["var"] + ("/pointwise_W" if op["ds"] else "/conv_W")
    out[w] = weights[w] * f
    assert np.array_equal(out[w].astype(np.float64), weights[w].astype(np.float64) * math.ldexp(1.0, e)), (target, e)
    if op["bias"]:
        out[op["var"] + "/conv_B"] = weights[op["var"] + "/conv_B"] * f
    return out


def _amax(t, image=None):
    a = np.abs(t if image is None else t[image])
    return float(a.max()) if a.size else 0.0


def conditions(oracle, cfg, tensors, hot, target):
    """None when the three conditions hold on ``tensors`` (oracle.forward(..., return_intermediates=True)[1]), else which one fails."""
    i = hot_index(hot)
    before = tensors_before(oracle, cfg, target)
    for name in before:
        if _amax(tensors[name], i) >= LIM_LO:
            return "hot image reaches %.6g in %s, in front of %s" % (_amax(tensors[name], i), name, target)
    if _amax(tensors[target], i) < LIM_HI:
        return "hot image reaches only %.6g in %s" % (_amax(tensors[target], i), target)
    n = tensors["x"].shape[0]
    for name, t in tensors.items():
        if name in ("y_", "x2"):
            continue
        for j in range(n):
            if j != i and _amax(t, j) >= LIM_LO:
                return "bystander %d reaches %.6g in %s" % (j, _amax(t, j), name)
    return None


def base_tensors(oracle, cfg, weights, x, hot):
    """The tensors of the hot batch with the weights as they are (e = 0): what every target's guess is read from."""
    xb = hot_input(x, hot)
    x2 = np.zeros((x.shape[0], x.shape[1] * cfg["scale"], x.shape[2] * cfg["scale"], 1), np.float32)
    return oracle.forward(cfg, weights, xb, x2, dtype=np.float64, return_intermediates=True)[1]


def _find(oracle, cfg, weights, x, hot, target, exponents, base=None):
    """(weights', e, float64 y_ of the hot batch, its tensors) by the rule of first_overflow_at, or None."""
    t0 = base if base is not None else base_tensors(oracle, cfg, weights, x, hot)
    m = _amax(t0[target], hot_index(hot))
    if not (m > 0.0 and math.isfinite(m)):
        return None
    # filter, bias and every activator the nets use (prelu, relu, leaky_relu) are positively homogeneous in the target's (W, B): its output at
    # 2^e is 2^e times this one, so the smallest e that reaches LIM_HI is known from one forward; a second one confirms it with the rest
    assert cfg["activator"] in ("prelu", "relu", "leaky_relu")
    e = int(math.ceil(math.log2(LIM_HI / m)))
    if e not in exponents:
        return None
    w = scaled_weights(oracle, cfg, weights, target, e)
    y, t = oracle.forward(cfg, w, t0["x"], t0["x2"], dtype=np.float64, return_intermediates=True)
    if conditions(oracle, cfg, t, hot, target) is not None:
        return None
    assert e == min(exponents) or m * math.ldexp(1.0, e - 1) < LIM_HI
    return w, e, y, t


def first_overflow_at(oracle, cfg, weights, x, hot, target, exponents=DIRECTED_EXPONENTS, base=None):
    """``(weights', e)`` with the smallest e of ``exponents`` for which, with the target conv's filter and bias times 2^e, the hot image
    stays below LIM_LO in every tensor before the target's output, reaches LIM_HI in it, and every other image of ``x`` stays below
    LIM_LO in every tensor except y_; None when no exponent does.  ``hot``: an image index (that image times 8) or (image, row, col)
    (that LR pixel set to 0.85 * 65504).  x2 = 0."""
    found = _find(oracle, cfg, weights, x, hot, target, exponents, base)
    return None if found is None else found[:2]


class HotCase:
    """One hot batch with its float64 reference; the conditions are asserted on the tensors of the forward that yields ``ref``."""

    def __init__(self, oracle, cfg, weights, x, hot, target, exponents=DIRECTED_EXPONENTS, base=None):
        found = _find(oracle, cfg, weights, x, hot, target, exponents, base)
        assert found is not None, "no exponent in %r puts the first overflow of %r at %s" % (exponents, hot, target)
        self.cfg, self.hot, self.target, self.i = cfg, hot, target, hot_index(hot)
        self.weights, self.e, ref, tensors = found
        assert conditions(oracle, cfg, tensors, hot, target) is None
        self.x = np.array(x, np.float32, copy=True)
        self.xb = hot_input(x, hot)
        self.x2 = np.zeros(ref.shape, np.float32)
        self.ref = ref
        self.peak = _amax(tensors[target], self.i)
        for a in (self.x, self.xb, self.x2, self.ref):
            a.flags.writeable = False


# ---------------------------------------------------------------------------------------------
# relay nets: a float32 value of the input reaches the operands of CNN2 and of A1 || B1 with its exact bits
# ---------------------------------------------------------------------------------------------
RELAY_SHIFT = 12                        # the relayed channel's filter rows times 2^-12: 65520 * 2^-12 * |w| < 16 |w|


def relay_weights(cfg, weights, channel, shift=RELAY_SHIFT):
    """A copy of ``weights`` in which output channel ``channel`` of CNN1 is the input itself (centre tap 1, other taps 0, bias 0, PReLU
    slope 1: exact for either sign), CNN1's other filters are halved, and every consumer's filter rows for that channel -- CNN2's input channel, A1's and B1's row of the
    concat, which CNN1 leads -- are multiplied by 2^-shift, so that the relayed value moves no other tensor far."""
    assert cfg["channels"] == 1 and not cfg["depthwise_separable"] and cfg["use_nin"] and cfg["activator"] == "prelu" and cfg["layers"] >= 2
    out = dict(weights)
    k = cfg["cnn_size"]
    w = np.array(weights["CNN1/conv_W"], np.float32, copy=True)
    assert 0 <= channel < w.shape[3]
    w *= np.float32(0.5)                # the other channels see the value through a tap of up to 0.94: halved, they stay below LIM_LO
    w[:, :, 0, channel] = 0.0
    w[k // 2, k // 2, 0, channel] = 1.0
    out["CNN1/conv_W"] = w
    b = np.array(weights["CNN1/conv_B"], np.float32, copy=True)
    b[channel] = 0.0
    out["CNN1/conv_B"] = b
    a = np.array(weights["CNN1/prelu/CNN1_prelu"], np.float32, copy=True)
    a[channel] = 1.0
    out["CNN1/prelu/CNN1_prelu"] = a
    f = np.float32(math.ldexp(1.0, -shift))
    for name in ("CNN2/conv_W", "A1/conv_W", "B1/conv_W"):
        w = np.array(weights[name], np.float32, copy=True)
        w[:, :, channel, :] *= f
        out[name] = w
    return out


def edge_values():
    """The eight float32 values around the edge, and whether each is beyond it: +-65504, +-nextafter(65520, 0), +-65520, +-nextafter(65520, inf)."""
    edge = np.float32(F16_EDGE)
    mags = [np.float32(F16_MAX), np.nextafter(edge, np.float32(0.0)), edge, np.nextafter(edge, np.float32(np.inf))]
    assert [float(m) >= F16_EDGE for m in mags] == [False, False, True, True] and float(mags[1]) > 65519.99
    return [(np.float32(s) * m, bool(float(m) >= F16_EDGE)) for m in mags for s in (1.0, -1.0)]


def relay_input(x, image, row, col, v):
    xb = np.array(x, np.float32, copy=True)
    xb[image, row, col, 0] = np.float32(v)
    return xb


def relay_conditions(tensors, image, row, col, channel, v):
    """None when CNN1's relay channel holds x bit for bit and only the relayed value is >= 65504 in any operand (tensors: float32
    restatement with intermediates); else what fails."""
    x, c1 = tensors["x"], tensors["CNN1"]
    if x.dtype != np.float32 or not np.array_equal(c1[..., channel].view(np.uint32), x[..., 0].view(np.uint32)):
        return "CNN1[..., %d] is not x bit for bit" % channel
    if c1[image, row, col, channel] != np.float32(v):
        return "the relay channel holds %r at the hot pixel, not %r" % (c1[image, row, col, channel], v)
    for name, t in tensors.items():
        if name in ("y_", "x2"):
            continue
        a = np.abs(t.astype(np.float64))
        big = np.argwhere(a >= F16_MAX)
        for idx in big:
            relayed = tuple(idx[:3]) == (image, row, col) and (name == "x" or (name in ("CNN1", "H_concat") and idx[3] == channel))
            if not relayed:
                return "%s%r = %.6g" % (name, tuple(idx), a[tuple(idx)])
        if name == "x":
            a[image, row, col, 0] = 0.0
        elif name in ("CNN1", "H_concat"):
            a[image, row, col, channel] = 0.0
        if a.max() >= LIM_LO:
            return "%s reaches %.6g beside the relayed value" % (name, a.max())
    return None


# ---------------------------------------------------------------------------------------------
# which launches of eng.ops() write and read a tensor of the topology
# ---------------------------------------------------------------------------------------------
SPLIT16_KERNELS = ("conv_nin_h", "conv5_h", "conv3_h8", "conv3_h", "feat3_stream")
STREAM_KERNELS = ("feat_stream", "tail_stream")             # one name for the float32 and the F16 instantiation: split16 where the option's bit 0 is on


def _covered(op_name, names, vars_):
    """The convs of the topology (by name) that the launch called ``op_name`` computes (graph.hip's launch names)."""
    base = op_name.replace(" (folded)", "").replace(" (streamed)", "")
    if base.endswith("/depthwise"):
        base = base[: -len("/depthwise")]

    def one(part):
        part = part.strip()
        for n, v in zip(names, vars_):
            if part in (n, v) or v.split("/")[0] == part:
                return n
        if part == "R-CNN":
            return names[-1]
        return None                                         # (the transposed-conv upsampler: no conv of the topology)
    if ".." in base:
        first, last = base.split("..")
        a, b = names.index(one(first)), names.index(one(last))
        return names[a:b + 1]
    return [n for n in (one(p) for p in base.split("+")) if n is not None]


def _around(oracle, cfg, ops, target):
    """(launches that compute ``target``, [(launch, the convs it computes that read ``target``)])."""
    topo = oracle.build_topology(cfg)
    cv = [o for o in topo if o["op"] == "conv"]
    names, vars_ = [o["name"] for o in cv], [o["var"] for o in cv]
    holds = {}                                              # tensor -> conv outputs it is made of
    for o in topo:
        if o["op"] == "conv":
            holds[o["dst"]] = {o["name"]}
        elif o["op"] in ("concat", "add"):
            holds[o["dst"]] = set().union(*[holds.get(s, set()) for s in o["srcs"]])
        else:
            holds[o["dst"]] = set(holds.get(o["src"], set()))
    readers = {o["name"]: o for o in cv if target in holds.get(o["src"], set())}
    writes, reads = [], []
    for op in ops:
        got = _covered(op["name"], names, vars_)
        if target in got:
            writes.append(op)
        if set(readers) & set(got):
            reads.append((op, [readers[n] for n in got if n in readers]))
    assert writes, (target, [o["name"] for o in ops])
    return writes, reads


def launches_around(oracle, cfg, ops, target):
    """(launches that compute ``target``, launches that compute a conv reading it) as lists of eng.ops() entries."""
    writes, reads = _around(oracle, cfg, ops, target)
    return writes, [op for op, _ in reads]


def on_split16(op, split16=1):
    """Whether the launch runs a split16 kernel under option split16 = 1 / 2 (3x3 and streamed only) / 3 (1x1 only)."""
    return op["kernel"] in SPLIT16_KERNELS or (op["kernel"] in STREAM_KERNELS and split16 in (1, 2))


def flag_expected(oracle, cfg, ops, target, split16=1):
    """Whether the plan of ``ops`` must raise the flag of an image that leaves the range in ``target``: a split16 launch READS the tensor
    as an operand of its contraction.  It then meets the value (a non-finite accumulator), or, the tensor being P16, its writer has
    produced it -- a P16 tensor has split16 readers only.  Not such a read:
    - a split16 launch that only WRITES a float32 tensor;
    - a folded launch that computes the target and its reader as one affine map: it never holds the tensor (a streamed one holds it as
      (hi, lo) pairs in LDS);
    - a separable k x k conv: its depthwise stage reads the tensor in float32 -- the "/depthwise" launch, or VALU code inside
      feat_stream / tail_stream -- and the contraction reads that stage's output.  (A folded launch composes both stages into one filter.)
    None where the list cannot tell: the reader is a "layer by layer" launch, whose layers' kernels dcscn_op_info does not name."""
    writes, reads = _around(oracle, cfg, ops, target)
    unknown = False
    for op, convs_read in reads:
        folded = "(folded)" in op["name"]
        if folded and any(op is w for w in writes):
            continue
        for c in convs_read:
            if c["ds"] and c["k"] > 1 and not folded:
                continue
            if op["kernel"] == "layer by layer":
                unknown = True
            elif on_split16(op, split16):
                return True
    return None if unknown else False


# ---------------------------------------------------------------------------------------------
# the self-ensemble: one image that leaves the range at the target in EVERY flip
# ---------------------------------------------------------------------------------------------
class EnsembleCase:
    """An image times 8 and the smallest e for which each of the first ``n_ensemble`` flips (oracle.flip) meets the conditions of
    first_overflow_at as a batch of one; ``ref`` is oracle.do's float64 mean, formed here from the forwards the conditions are
    asserted on.  None of the flips may stay inside the range: its bits would be split16 bits, not the float32 plan's."""

    def __init__(self, oracle, cfg, weights, image, target, n_ensemble, exponents=DIRECTED_EXPONENTS):
        s = cfg["scale"]
        h, w = image.shape[:2]
        self.cfg = cfg
        self.x = np.array(image, np.float32, copy=True).reshape(h, w, 1)
        self.xb = hot_input(self.x[None], 0)[0]
        self.x2 = np.zeros((h * s, w * s, 1), np.float32)
        flips = [np.ascontiguousarray(oracle.flip(self.xb, i)) for i in range(n_ensemble)]
        peaks = [_amax(base_tensors(oracle, cfg, weights, f[None] / np.float32(HOT_FACTOR), 0)[target]) for f in flips]
        e = int(math.ceil(math.log2(LIM_HI / min(peaks))))
        assert e in exponents, (target, e)
        self.e, self.target, self.n = e, target, n_ensemble
        self.weights = scaled_weights(oracle, cfg, weights, target, e)
        out = np.zeros([s * h, s * w, 1])
        for i, f in enumerate(flips):
            y, t = oracle.forward(cfg, self.weights, f[None], oracle.flip(self.x2, i)[None], dtype=np.float64, return_intermediates=True)
            why = conditions(oracle, cfg, t, 0, target)
            assert why is None, (i, why)
            out += oracle.flip(y[0], i, invert=True)
        out /= n_ensemble
        self.ref = out


# ---------------------------------------------------------------------------------------------
# the directed cases both files parametrize: shipped nets, weights seed 9, batch seed 10
# ---------------------------------------------------------------------------------------------
WEIGHT_SEED, BATCH_SEED = 9, 10
NETS = ("L7_F32to8_x2", "L7_F32to8_x3", "L7_F32to8_x4", "L7_F32to8_x4_DS", "L8_F96to48_x2", "L12_F196to48_x2", "L12_F196to48_x4")
SHAPE_A = (3, 17, 19, 1)                # (n, h, w, hot image): no multiple of any tile; 323 pixels, so 128- and 256-pixel blocks straddle images
SHAPE_A_L12 = (3, 20, 15, 2)            # the L12 nets once more with the hot image last
# convs of a topology for which no exponent of DIRECTED_EXPONENTS meets the conditions on SHAPE_A (tests/test_overflow_host.py asserts
# that these, and no others, are the ones): the separable net's last feature layers are too small where their predecessors are in range
LEFT_OUT_A = {"L7_F32to8_x4_DS": ("CNN6", "CNN7", "Up-PS2_CNN")}


def flagged_by_hand(net, target):
    """Shipped nets, default options: every target up to B2 is read by a split16 launch; Up-PS*, R-CNN* are inside the folded tail or
    float32 tensors of the tail (only a float32 value overflows), and nothing is asserted about the flag there.  On the separable net
    B1's only reader is B2's depthwise stage, float32 code inside feat_stream."""
    return not target.startswith(("Up-", "R-CNN")) and not (net == "L7_F32to8_x4_DS" and target == "B1")


def cases_a(oracle, configs):
    """[(net, shape, target, flagged)] of leg A."""
    out = []
    for net in NETS:
        cfg = oracle.make_config(**configs[net])
        for shape in (SHAPE_A,) + ((SHAPE_A_L12,) if net.startswith("L12") else ()):
            for t in conv_names(oracle, cfg):
                if shape == SHAPE_A and t in LEFT_OUT_A.get(net, ()):
                    continue
                out.append((net, shape, t, flagged_by_hand(net, t)))
    return out


# leg B: one hot pixel in image 1 of 3, on the streamed kernels' shapes with a last strip of one column (exec.hip: stream_geometry)
NETS_B = (("L8_F96to48_x2", 17, 33), ("L7_F32to8_x2", 17, 33), ("L7_F32to8_x4_DS", 33, 49))
# 0.85 * 65504 behind the separable CNN1 (depthwise tap x pointwise weight up to 2.6) leaves LIM_LO before any later target: on the separable net
# the pixel cases take CNN1 itself as the target -- in front of it there is only x -- and the four later targets are left out
TARGETS_B = {"L8_F96to48_x2": ("CNN2", "CNN8", "A1", "B2"), "L7_F32to8_x2": ("CNN2", "CNN7", "A1", "B2"), "L7_F32to8_x4_DS": ("CNN1",)}
LEFT_OUT_B = {"L7_F32to8_x4_DS": ("CNN2", "CNN7", "A1", "B2")}


def pixels_b(h, w):
    return ((0, 0), (h - 1, w - 1), (h // 2, w // 2))


def cases_b():
    """[(net, (3, h, w, (1, row, col)), target, flagged)] of leg B."""
    return [(net, (3, h, w, (1,) + px), t, True) for net, h, w in NETS_B for px in pixels_b(h, w) for t in TARGETS_B[net]]


_NET, _BASE, _CASE = {}, {}, {}


def shipped_net(oracle, configs, net):
    if net not in _NET:
        cfg = oracle.make_config(**configs[net])
        _NET[net] = (cfg, bare_weights(cfg, oracle.synthetic_weights(cfg, seed=WEIGHT_SEED)))
    return _NET[net]


def directed_base(oracle, configs, net, shape):
    """(cfg, weights, clean x, e = 0 tensors of the hot batch) of a directed case's net and shape, computed once."""
    key = (net, shape)
    if key not in _BASE:
        cfg, weights = shipped_net(oracle, configs, net)
        n, h, w, hot = shape
        x, _ = bare_batch(n, h, w, cfg["scale"], BATCH_SEED)
        x.flags.writeable = False
        _BASE[key] = (cfg, weights, x, base_tensors(oracle, cfg, weights, x, hot))
    return _BASE[key]


def directed_case(oracle, configs, net, shape, target):
    """The HotCase of (net, shape = (n, h, w, hot), target), computed once and shared by the tests that need it; left unchanged."""
    key = (net, shape, target)
    if key not in _CASE:
        cfg, weights, x, base = directed_base(oracle, configs, net, shape)
        _CASE[key] = HotCase(oracle, cfg, weights, x, shape[3], target, base=base)
    return _CASE[key]


# ---------------------------------------------------------------------------------------------
# the walk: the 200 draws of test_random_configs._draw, first image and its 8-fold copy, target by seed
# ---------------------------------------------------------------------------------------------
# draws for which no exponent of WALK_EXPONENTS meets the conditions (asserted by tests/test_overflow_host.py to be exactly these)
WALK_LEFT_OUT = (20,)                   # target CNN3


def walk_target(oracle, cfg, seed):
    names = conv_names(oracle, cfg)
    return names[seed % len(names)]


def walk_setup(oracle, seed):
    """(flags, cfg, bare weights, x = [first image, first image], target, engine options) of draw ``seed``; image 1 is the hot one."""
    flags, cfg, weights, x, _, opts = walk_draw(oracle, seed)
    x = np.ascontiguousarray(np.concatenate([x[:1], x[:1]]))
    return flags, cfg, weights, x, walk_target(oracle, cfg, seed), opts


def walk_case(oracle, seed):
    flags, cfg, weights, x, target, opts = walk_setup(oracle, seed)
    return flags, opts, HotCase(oracle, cfg, weights, x, 1, target, exponents=WALK_EXPONENTS)
