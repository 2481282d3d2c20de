"""The bare network branch and its bar, shared by tests/test_bare_branch_host.py and tests/test_bare_branch_surface_hip.py.

"Bare" (test_residual_branch_relative_error, test_streamed_separable_net_matches_layer_by_layer): the last reconstruction conv,
which oracle.synthetic_weights attenuates by 0.01, is multiplied by 100 again, and the bicubic input x2 is zero, so that the
output is the network branch alone and an upstream error cannot hide behind the bicubic term.  The error of an output is
``max|y - ref| / max|ref|`` against ``oracle.forward(..., float64)``.

The bar is the project's 5e-6.  A float32 restatement of the same graph (``oracle.forward(dtype=np.float32)``) stays within
1.02e-6 of float64 on the 200 draws of test_random_configs._draw, so the bar has a margin of 4.9 over a correct float32
implementation.  A case beyond 5e-6 still passes when it is within 4 times (4.9 rounded down) its OWN float32 restatement's
error; the restatement is computed only for such a case, and the GPU file asserts that at most 2 % of its cases needed it.
No bar is derived from the kernels' output."""
import numpy as np

from conftest import synthetic_batch
from test_random_configs import _draw

BAR = 5e-6
RESTATEMENT_FACTOR = 4.0
WALK_RNG_BASE = 1000                # test_random_configs._run_draw: default_rng(1000 + seed)


def bare_weights(cfg, weights):
    """A copy of ``weights`` with every conv_W / pointwise_W of R-CNN<reconstruct_layers> multiplied by 100."""
    last = "R-CNN%d/" % cfg["reconstruct_layers"]
    out = dict(weights)
    hit = 0
    for k in weights:
        if k.startswith(last) and k.endswith(("conv_W", "pointwise_W")):
            out[k] = weights[k] * np.float32(100.0)
            hit += 1
    assert hit == 1, (last, sorted(weights))
    return out


def bare_batch(n, h, w, scale, seed):
    """synthetic_batch's x with x2 = 0."""
    x, x2 = synthetic_batch(n, h, w, scale, seed=seed)
    return x, np.zeros_like(x2)


def rel_error(y, ref):
    return float(np.max(np.abs(np.asarray(y, np.float64) - ref)) / np.max(np.abs(ref)))


def worst_pixel(y, ref):
    """'image i, pixel (r, c) of HxW: top r, bottom b, left c, right d' of the largest error of an [n, H, W, 1] output."""
    err = np.abs(np.asarray(y, np.float64) - ref)[..., 0]
    i, r, c = np.unravel_index(int(np.argmax(err)), err.shape)
    hh, ww = err.shape[1:]
    return "image %d, HR pixel (%d, %d) of %dx%d: %d from the top, %d from the bottom, %d from the left, %d from the right" % (
        i, r, c, hh, ww, r, hh - 1 - r, c, ww - 1 - c)


def walk_draw(oracle, seed):
    """Draw ``seed`` of test_random_configs on the bare branch: (flags, cfg, bare weights, x, x2 = 0, engine options)."""
    flags, n, h, w, opts = _draw(np.random.default_rng(WALK_RNG_BASE + seed))
    cfg = oracle.make_config(**flags)
    weights = bare_weights(cfg, oracle.synthetic_weights(cfg, seed=seed))
    x, x2 = bare_batch(n, h, w, cfg["scale"], seed + 1)
    return flags, cfg, weights, x, x2, opts


def restatement_error(oracle, cfg, weights, x, x2, ref):
    """Relative error of the float32 restatement of the graph against the float64 reference."""
    return rel_error(oracle.forward(cfg, weights, x, x2, dtype=np.float32), ref)
