"""CPU restatement of the engine option "fast16" (include/dcscn.h), shared by tests/test_fast16_host.py and tests/test_fast16_hip.py.

With fast16 = 1 every launch on conv3_h, conv3_h8, conv_nin_h or conv5_h takes a contraction as the single f16 product wh * xh:
xh = f16(x) of the float32 activation, wh = f16(w * 2^e) with 2^e the power of two that puts the layer's largest |w| in [2^13, 2^14)
(csrc/split16_pack.hpp), products exact in float32, accumulated in float32 per 32-deep block.  Here the convs of the topology that such a
launch computes (``selected``) have their activations and weights rounded the same way and are then accumulated in float64; every other
layer, and bias / activators / adds everywhere, is the oracle's.  A folded tail is modelled as the layers it replaces.

restate() substitutes dcscn_oracle.conv2d_same while it runs, as tools/f16x3_numerics.py does, and restores it in ``finally``.  The oracle
calls conv2d_same once per conv op, in topology order (a separable conv: for its pointwise stage), which is how a call learns its layer."""
import math

import numpy as np

import overflow_cases as C

FAST16_KERNELS = ("conv3_h", "conv3_h8", "conv_nin_h", "conv5_h")


def f16_round(x):
    """f16(float32(x)) as float64: what the hi piece of a P16 record, or of a value split in registers, holds."""
    return np.asarray(x).astype(np.float32).astype(np.float16).astype(np.float64)


def weight_scale(w):
    """The power of two s with max|w| * s in [2^13, 2^14)."""
    m = float(np.max(np.abs(w)))
    if m == 0.0:
        return 1.0
    s = math.ldexp(1.0, 13 - int(math.floor(math.log2(m))))
    assert 2.0 ** 13 <= m * s < 2.0 ** 14, (m, s)
    return s


def f16_weights(w):
    s = weight_scale(w)
    return f16_round(np.asarray(w, np.float64) * s) / s


def numerics_rule(name, w):
    """The eligibility rule of tools/f16x3_numerics.py: 3x3 with >= 24 input channels and more than one output tile, 1x1 with >= 32 inputs."""
    kh, kw, cin, cout = w.shape
    if kh == 3:
        return cin >= 24 and cout > 16
    return kh == 1 and cin >= 32


def selected_by_ops(oracle, cfg, ops):
    """Names of the convs of the topology computed by a launch of ``ops`` (Engine.ops()) whose kernel is one of FAST16_KERNELS."""
    convs = C.convs(oracle, cfg)
    names, vars_ = [o["name"] for o in convs], [o["var"] for o in convs]
    out = set()
    for op in ops:
        if op["kernel"] in FAST16_KERNELS:
            out.update(C._covered(op["name"], names, vars_))
    return frozenset(out)


def restate(oracle, cfg, weights, x, x2, selected):
    """float64 y_ of the net with the convs in ``selected`` -- a set of conv names, or a rule(name, w) -> bool -- on one f16 product."""
    names = C.conv_names(oracle, cfg)
    rule = selected if callable(selected) else (lambda name, w: name in selected)
    real = oracle.conv2d_same
    calls = []

    def conv(xin, w):
        name = names[len(calls)]
        calls.append(name)
        if not rule(name, w):
            return real(xin, w)
        return real(f16_round(xin), f16_weights(w))

    oracle.conv2d_same = conv
    try:
        y = oracle.forward(cfg, weights, x, x2, dtype=np.float64)
    finally:
        oracle.conv2d_same = real
    assert calls == names, (calls, names)
    return y


def rms(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return float(np.sqrt(np.mean(d * d)))


def max_abs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


_MODEL = {}


def model_error(oracle, key, cfg, weights, x, x2, selected):
    """(float64 oracle output, restatement output, E_model = rms of their difference), computed once per ``key`` + selection."""
    k = (key, selected if not callable(selected) else selected.__name__)
    if k not in _MODEL:
        ref = oracle.forward(cfg, weights, x, x2, dtype=np.float64)
        mod = restate(oracle, cfg, weights, x, x2, selected)
        for a in (ref, mod):
            a.flags.writeable = False
        _MODEL[k] = (ref, mod, rms(mod, ref))
    return _MODEL[k]
