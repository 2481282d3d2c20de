"""CPU restatement, nets and one-product sets of the engine option "fast16_separable" (include/dcscn.h), shared by
tests/test_fast16_separable_host.py and tests/test_fast16_separable_hip.py.  Built on tests/fast16_model.py (f16_round, weight_scale, rms,
max_abs), which stays as it is.

With fast16_separable = 1 (and split16 = 1) every matrix contraction of a feat_stream or tail_stream launch (csrc/feat_stream.hpp,
csrc/tail_stream.hpp: NP = 1) is the single product wh * xh accumulated in float32.  The one-product set of a launch is every conv it
computes except CNN1 (feat_stream) and R-CNN1 (tail_stream), which are float32 VALU work.  The device's rounding points, restated here:

* k x k separable layers (CNN2 .., B2, Up-PS, Up-PS2): the depthwise stage is the oracle's (float32 on the device), its output is rounded
  to f16; the pointwise filter is multiplied by the power of two that puts THAT tensor's largest magnitude in [2^13, 2^14)
  (csrc/split16_pack.hpp: split16_scale_exp over the pointwise tensor) and rounded to f16; products are accumulated in float64.  This is
  what fast16_model.restate does for a selected separable conv.
* A1 and B1 (1 x 1 separable): the device folds the 1 x 1 depthwise scale d_c into the filter (csrc/pack.hip: nin_column), so the operands
  are f16(x_c) and f16(float32(d_c * p[c][co]) * 2^e) with ONE e over all A1 || B1 columns.  fast16_model.restate would round f16(x_c d_c)
  and f16(p 2^e_layer) instead; restate() below takes the device's form.

A conv selected because a LAYER kernel computes it on one product (option "fast16": the folded tail on conv5_h, modelled as the layers it
replaces) is restated as fast16_model.restate does it.

restate() substitutes dcscn_oracle.conv2d_same and depthwise_conv2d_same while it runs and restores them in ``finally``.  The oracle calls
conv2d_same once per conv op, in topology order, and for a separable conv depthwise_conv2d_same right in front of it.

Every error band of the device tests runs on the BARE BRANCH (x2 = 0, the last conv's conv_W / pointwise_W times 100, errors relative to
max |ref|) or on trained weights: oracle.synthetic_weights attenuates the last conv by 0.01, which puts the mode's error below the float32
floor of the rest of the net, where no band can be met or mean anything."""
import os

import numpy as np

import fast16_model as M
import overflow_cases as C
from conftest import CONFIGS, GOLDEN, synthetic_batch

STREAM_KERNELS = ("feat_stream", "tail_stream")
NOT_ON_THE_MATRIX_PIPE = {"feat_stream": "CNN1", "tail_stream": "R-CNN1"}
C5 = "L7_F32to8_x4_DS"
# (n, h, w): one ragged strip; images shorter than the 2L+1-step pipeline, jobs back to back behind separator rows; two 48-pixel column strips
# with halos; one tall single image that the plan cuts into row blocks
SHAPES = [(2, 19, 35), (3, 7, 9), (1, 50, 51), (1, 300, 70)]
VARIANT_SHAPE = (2, 19, 35)
TAIL_SHAPES = [(2, 19, 35), (1, 50, 51)]
C5_SEED = 11


# ---------------------------------------------------------------------------------------------
# nets
# ---------------------------------------------------------------------------------------------
def bare_weights(cfg, weights):
    """The last conv NOT attenuated (tests/test_hip_parity.py: test_streamed_separable_net_matches_layer_by_layer)."""
    weights = dict(weights)
    last = "R-CNN%d" % cfg["reconstruct_layers"]
    hit = [k for k in weights if k.startswith(last + "/") and k.endswith(("conv_W", "pointwise_W"))]
    assert hit, last
    for k in hit:
        weights[k] = weights[k] * 100.0
    return weights


def bare_input(n, h, w, scale, seed):
    x, x2 = synthetic_batch(n, h, w, scale, seed=seed)
    return x, np.zeros_like(x2)


_NETS = {}


def c5(oracle):
    """(cfg, bare-branch weights) of BASELINE configs[4]."""
    if "c5" not in _NETS:
        cfg = oracle.make_config(**CONFIGS[C5])
        _NETS["c5"] = (cfg, bare_weights(cfg, oracle.synthetic_weights(cfg, seed=C5_SEED)))
    return _NETS["c5"]


def variant(oracle, v):
    """(cfg, bare-branch weights) of an entry of test_hip_parity.STREAM_VARIANTS, built as test_feat_stream_variants builds it."""
    if v not in _NETS:
        layers, filters, min_filters, gamma, na, nb, scale, act = v
        cfg = oracle.make_config(layers=layers, filters=filters, min_filters=min_filters, filters_decay_gamma=gamma, nin_filters=na,
                                 nin_filters2=nb, scale=scale, activator=act, depthwise_separable=True, reconstruct_layers=0,
                                 pixel_shuffler_filters=1)
        _NETS[v] = (cfg, bare_weights(cfg, oracle.synthetic_weights(cfg, seed=layers * 10 + scale)))
    return _NETS[v]


def conv_pairs(oracle, v):
    """[(input quads, output tiles)] of CNN2 .. CNNL and B2: the template arguments of stream_conv_role."""
    layers, filters, min_filters, gamma, na, nb = v[:6]
    sched = oracle.filter_schedule(layers, filters, min_filters, gamma)
    quads = lambda c: (c + 3) // 4
    return [(quads(sched[i]), (sched[i + 1] + 15) // 16) for i in range(layers - 1)] + [(quads(nb), (nb + 15) // 16)]


# the instantiations feat_stream's dispatch has (csrc/feat_stream.hpp: the switch in feat_stream), which are the pairs the plan streams
# (graph.hip: stream_conv_supported -- up to 5 input quads one output tile, 6 and 7 two, 8 either)
INSTANTIATED = frozenset([(1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (6, 2), (7, 2), (8, 2), (8, 1)])
# test_hip_parity.STREAM_VARIANTS holds no 8-quad layer with at most 16 outputs, so its streaming entries leave <8, 1> out: 32 -> 12 reaches it
EXTRA_VARIANTS = [(2, 32, 12, 1.0, 8, 8, 2, "prelu")]


def streams(oracle, v):
    """The plan takes feat_stream for this net (tests/test_hip_parity.py: test_feat_stream_variants asserts the same rule on the device)."""
    return all(p in INSTANTIATED for p in conv_pairs(oracle, v))


def streaming(oracle, variants):
    return [v for v in variants if streams(oracle, v)]


def last_chunk_quads(oracle, v):
    """Valid channel quads (1 .. 4) of the last 16-channel chunk of every A1 || B1 source ring (StreamNinSrc::last_ql)."""
    layers, filters, min_filters, gamma = v[:4]
    return [((c + 3) // 4 - 1) % 4 + 1 for c in oracle.filter_schedule(layers, filters, min_filters, gamma)]


def chunk_parities(oracle, v):
    """{chunks odd?} over the pointwise GEMMs and the A1 || B1 sources: odd = the K = 16 MFMA form is taken, more than one = the K = 32 form."""
    layers, filters, min_filters, gamma, na, nb = v[:6]
    chunks = [(c + 15) // 16 for c in oracle.filter_schedule(layers, filters, min_filters, gamma)] + [(nb + 15) // 16]
    return {"k16": any(c & 1 for c in chunks), "k32": any(c >= 2 for c in chunks)}


# ---------------------------------------------------------------------------------------------
# one-product sets
# ---------------------------------------------------------------------------------------------
def _names(oracle, cfg):
    convs = C.convs(oracle, cfg)
    return [o["name"] for o in convs], [o["var"] for o in convs]


def streamed_set_of(oracle, cfg, kernel, launch_name):
    """The convs a feat_stream / tail_stream launch of that name takes on one product: all it computes but CNN1 / R-CNN1."""
    names, vars_ = _names(oracle, cfg)
    return frozenset(C._covered(launch_name, names, vars_)) - {NOT_ON_THE_MATRIX_PIPE[kernel]}


def streamed_set(oracle, cfg, ops):
    """The same from Engine.ops(): empty where the plan has neither launch."""
    out = set()
    for op in ops:
        if op["kernel"] in STREAM_KERNELS:
            assert op["name"].endswith(" (streamed)"), op
            out |= streamed_set_of(oracle, cfg, op["kernel"], op["name"])
    return frozenset(out)


def one_product_set(oracle, cfg, ops, fast16, fast16_separable):
    """(convs on one product under the two options, those among them in the device's feat_stream / tail_stream form)."""
    sep = streamed_set(oracle, cfg, ops) if fast16_separable else frozenset()
    lay = M.selected_by_ops(oracle, cfg, ops) if fast16 else frozenset()
    assert not (sep & lay), (sep, lay)
    return frozenset(sep | lay), sep


FEAT_SET_C5 = frozenset(["CNN%d" % i for i in range(2, 8)] + ["A1", "B1", "B2"])
TAIL_SET_C5 = frozenset(["Up-PS_CNN", "Up-PS2_CNN"])
FOLD_SET_C5 = frozenset(["Up-PS_CNN", "Up-PS2_CNN", "R-CNN1"])


# ---------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------
def nin_scale(weights, vars_):
    """The ONE power of two of the A1 || B1 image: over float32(d_c * p[c][co]) of both layers (csrc/pack.hip: pack_feat_stream)."""
    folded = [folded_nin(weights, v) for v in vars_]
    return M.weight_scale(np.concatenate([f.ravel() for f in folded]))


def folded_nin(weights, var):
    """float32(d_c * p[c][co]) of a 1 x 1 separable conv, as [cin, cout] (csrc/pack.hip: nin_column)."""
    d = np.asarray(weights[var + "/depthwise_W"], np.float32)
    p = np.asarray(weights[var + "/pointwise_W"], np.float32)
    assert d.shape[:2] == (1, 1) and p.shape[:2] == (1, 1) and d.shape[3] == 1, (d.shape, p.shape)
    return (d[0, 0, :, 0][:, None] * p[0, 0]).astype(np.float32)


def restate(oracle, cfg, weights, x, x2, selected, separable=None):
    """float64 y_ with the convs in ``selected`` on one f16 product; those also in ``separable`` (default: all of them) take the form
    of the streamed kernels, which differs from fast16_model.restate for A1 and B1 only."""
    selected = frozenset(selected)
    separable = selected if separable is None else frozenset(separable)
    assert separable <= selected
    convs = C.convs(oracle, cfg)
    names = [o["name"] for o in convs]
    by_name = {o["name"]: o for o in convs}
    folded = {n for n in separable if by_name[n]["k"] == 1 and by_name[n]["ds"]}
    assert folded in (set(), {"A1", "B1"}), folded                # one image, one scale: both or neither
    s_nin = nin_scale(weights, [by_name[n]["var"] for n in ("A1", "B1")]) if folded else None
    real_conv, real_dw = oracle.conv2d_same, oracle.depthwise_conv2d_same
    calls, held = [], []

    def depthwise(xin, w):
        name = names[len(calls)]                                   # the conv whose pointwise call comes next
        if name in folded:
            held.append(xin)                                       # the ring value: the depthwise scale is part of the filter
        return real_dw(xin, w)

    def conv(xin, w):
        name = names[len(calls)]
        calls.append(name)
        if name not in selected:
            return real_conv(xin, w)
        if name in folded:
            xr = held.pop()
            f = folded_nin(weights, by_name[name]["var"]).astype(np.float64)
            wf = M.f16_round(f * s_nin) / s_nin
            return real_conv(M.f16_round(xr), wf[None, None])
        return real_conv(M.f16_round(xin), M.f16_weights(w))

    oracle.conv2d_same, oracle.depthwise_conv2d_same = conv, depthwise
    try:
        y = oracle.forward(cfg, weights, x, x2, dtype=np.float64)
    finally:
        oracle.conv2d_same, oracle.depthwise_conv2d_same = real_conv, real_dw
    assert calls == names and not held, (calls, names)
    return y


_MODEL = {}


def model_error(oracle, key, cfg, weights, x, x2, selected, separable=None):
    """(float64 oracle output, restatement output, E_model = rms of their difference), computed once per key and selection and left
    unchanged."""
    selected = frozenset(selected)
    separable = selected if separable is None else frozenset(separable)
    k = (key, selected, separable)
    if k not in _MODEL:
        ref = reference(oracle, key, cfg, weights, x, x2)
        mod = restate(oracle, cfg, weights, x, x2, selected, separable)
        mod.flags.writeable = False
        _MODEL[k] = (ref, mod, M.rms(mod, ref))
    return _MODEL[k]


_REF = {}


def reference(oracle, key, cfg, weights, x, x2):
    if key not in _REF:
        ref = oracle.forward(cfg, weights, x, x2, dtype=np.float64)
        ref.flags.writeable = False
        _REF[key] = ref
    return _REF[key]


# ---------------------------------------------------------------------------------------------
# trained weights
# ---------------------------------------------------------------------------------------------
def golden_crop_ds(oracle):
    """(cfg, trained weights, lr [1, 48, 48, 1], bicubic [1, 192, 192, 1], HR ground truth [192, 192, 1]): the 48 x 48 LR crop at rows
    10 .. 57, columns 8 .. 55 of the third Set5 image at x4 with its bicubic x2, on tests/golden/weights_L7_x4_DS.npz."""
    if "crop" not in _NETS:
        import json
        from PIL import Image
        with open(os.path.join(GOLDEN, "goldens.json")) as f:
            g = json.load(f)
        cfg = oracle.make_config(**CONFIGS[C5])
        weights = dict(np.load(os.path.join(GOLDEN, "weights_L7_x4_DS.npz")))
        img = np.atleast_3d(np.array(Image.open(os.path.join(GOLDEN, "set5", g["files"][2]))))
        true_y = oracle.rgb_to_y(oracle.align(img, 4))
        lr_full = oracle.pil_bicubic(true_y, 0.25)
        r0, c0 = 10, 8
        assert lr_full.shape[0] >= r0 + 48 and lr_full.shape[1] >= c0 + 48, lr_full.shape
        lr = np.ascontiguousarray(lr_full[r0:r0 + 48, c0:c0 + 48]).astype(np.float32)
        bic = oracle.pil_bicubic(lr, 4).astype(np.float32)
        truth = np.ascontiguousarray(true_y[4 * r0:4 * r0 + 192, 4 * c0:4 * c0 + 192]).reshape(192, 192, 1)
        _NETS["crop"] = (cfg, weights, lr.reshape(1, 48, 48, 1), bic.reshape(1, 192, 192, 1), truth)
    return _NETS["crop"]
