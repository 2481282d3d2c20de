"""numpy restatement of the three update rules behind option "train_optimizers" (test helper, not a test; it extends
tests/train_ref.py, which stays as it is): TF 1.x's ApplyAdagrad, ApplyAdadelta and ApplyRMSProp as include/dcscn.h states them, with
the defaults TF gives the optimizers the reference constructs (DCSCN.py:383-392).  The arrays' dtype decides the arithmetic: float64
arrays give the yardstick, and nothing here rounds to float32.  Written from knowledge of TF 1.x, never run against TensorFlow."""
import numpy as np

ADADELTA_RHO, ADADELTA_EPS = 0.95, 1e-8
ADAGRAD_INITIAL_ACCUMULATOR = 0.1
RMSPROP_DECAY, RMSPROP_EPS, RMSPROP_INITIAL_MS = 0.9, 1e-10, 1.0

OPTIMIZERS = ("adagrad", "adadelta", "rmsprop")
# optimizer -> (suffix of the slot in the library's m buffer, suffix of the one in v or None): TF's slot names
SLOTS = {"adagrad": ("/Adagrad", None), "adadelta": ("/Adadelta", "/Adadelta_1"), "rmsprop": ("/RMSProp", "/RMSProp_1")}
INITIAL = {"adagrad": (ADAGRAD_INITIAL_ACCUMULATOR, None), "adadelta": (0.0, 0.0), "rmsprop": (RMSPROP_INITIAL_MS, 0.0)}


def f32(v):
    """The float32 nearest to v, as a Python float: the library holds lr, the momentum and the constants above as float32."""
    return float(np.float32(v))


def adagrad(w, g, acc, lr):
    """-> (w, acc)"""
    a = acc + g * g
    return w - lr * g * (1.0 / np.sqrt(a)), a


def adadelta(w, g, acc, upd, lr, rho=f32(ADADELTA_RHO), eps=f32(ADADELTA_EPS)):
    """-> (w, acc, upd); acc = <var>/Adadelta, upd = <var>/Adadelta_1"""
    a = acc * rho + g * g * (1.0 - rho)
    u = np.sqrt(upd + eps) * (1.0 / np.sqrt(a + eps)) * g
    return w - u * lr, a, upd * rho + u * u * (1.0 - rho)


def rmsprop(w, g, ms, mom, lr, mu, decay=f32(RMSPROP_DECAY), eps=f32(RMSPROP_EPS)):
    """-> (w, ms, mom); ms = <var>/RMSProp, mom = <var>/RMSProp_1; not centred"""
    s = ms + (g * g - ms) * (1.0 - decay)
    q = mom * mu + (g * lr) / np.sqrt(s + eps)
    return w - q, s, q


def step(opt, w, g, m, v, lr, mu):
    """One step of ``opt`` on (w, slot m, slot v) with the clipped gradient g -> (w, m, v); v passes through where the rule has none."""
    if opt == "adagrad":
        w, m = adagrad(w, g, m, lr)
    elif opt == "adadelta":
        w, m, v = adadelta(w, g, m, v, lr)
    elif opt == "rmsprop":
        w, m, v = rmsprop(w, g, m, v, lr, mu)
    else:
        raise NameError(opt)
    return w, m, v
