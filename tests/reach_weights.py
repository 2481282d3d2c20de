"""Weights whose output reaches exactly as far as the graph's receptive field, shared by tests/test_tiling_host.py and
tests/test_tiling_hip.py.

A forward through haloed windows (exec.hip: run_tiled) is right when every owned pixel lies at least the receptive-field radius
away from a cut.  He-initialised synthetic weights hardly tell a halo that is one pixel short: on the shipped nets of seven
layers or more a cut one pixel too near moves the outermost owned pixels by 4e-8 .. 2e-4 of the branch, 0.01 .. 42 times the
5e-6 bar, and a cut three pixels too near can still pass (tests/test_tiling_host.py prints the figure per net).  Here every k x k filter is zero except at ONE corner tap, all weights and biases are positive (every
activation is positive, PReLU is the identity) and each output channel's weights sum to 1 (magnitudes stay near the input's).
The output pixel then depends on one diagonal chain of input pixels that ends exactly at the true radius, and the pixel at its
end moves the output by O(1): a cut one pixel too near changes the outermost owned pixels by 7e-3 .. 0.5 of the branch.

Nothing is attenuated: the last conv keeps its full size and the tests use x2 = 0, so the output is the bare branch of
tests/bare_branch.py, judged by its ``rel_error`` at its ``BAR``."""
import numpy as np

from bare_branch import BAR, rel_error, worst_pixel  # noqa: F401  (re-exported: the two tiling files import them from here)

DIAGONALS = ((1, 1), (-1, -1), (1, -1), (-1, 1))      # (sy, sx): +1 = the tap at the bottom / right corner of the filter


def reach_weights(cfg, sy, sx, seed):
    """``{variable name: float32 array}`` for every name of ``oracle.variable_shapes(cfg)``.

    conv_W, depthwise_W and Tconv_W are zero except at the corner tap (bottom for sy > 0, right for sx > 0; a conv's output
    pixel then reads the input pixel floor(k / 2) below / right of it; Tconv_W takes the opposite corner, which is the tap
    through which an output pixel of the transposed conv reads below / right).  The tap holds U(0.5, 1.5) values, normalised so that
    each output channel's weights sum to 1 (conv_W [k, k, cin, cout]: over cin; Tconv_W [k, k, out, in]: over in; a depthwise
    channel has one weight, which stays as drawn: the pointwise filter behind it is normalised).  pointwise_W is positive and
    normalised over cin.  conv_B ~ U(0, 1); PReLU slopes ~ U(0.05, 0.3) as in ``oracle.synthetic_weights``."""
    import dcscn_oracle as oracle
    rng = np.random.default_rng(seed)
    diagonal = (sy, sx)
    weights = {}
    for name, shape in sorted(oracle.variable_shapes(cfg).items()):
        sy, sx = diagonal
        leaf = name.rsplit("/", 1)[-1]
        if leaf in ("conv_W", "depthwise_W", "Tconv_W"):
            k = shape[0]
            tap = rng.uniform(0.5, 1.5, shape[2:])
            if leaf == "conv_W":
                tap /= tap.sum(axis=0, keepdims=True)
            elif leaf == "Tconv_W":
                tap /= tap.sum(axis=1, keepdims=True)
            w = np.zeros(shape)
            if leaf == "Tconv_W":                     # a transposed conv scatters: tap 0 is the one whose output reads downwards
                sy, sx = -sy, -sx
            w[k - 1 if sy > 0 else 0, k - 1 if sx > 0 else 0] = tap
        elif leaf == "pointwise_W":
            w = rng.uniform(0.5, 1.5, shape)
            w /= w.sum(axis=2, keepdims=True)
        elif leaf == "conv_B":
            w = rng.uniform(0.0, 1.0, shape)
        else:
            w = rng.uniform(0.05, 0.3, shape)
        weights[name] = w.astype(np.float32)
    return weights


def reach_batch(n, h, w, scale, seed):
    """x ~ U(0, 255) [n, h, w, 1] and x2 = 0."""
    x = np.random.default_rng(seed).uniform(0, 255, (n, h, w, 1)).astype(np.float32)
    return x, np.zeros((n, h * scale, w * scale, 1), np.float32)


def implied_radius(oracle, cfg):
    """The receptive-field radius of y_ in LR pixels that ``oracle.build_topology(cfg)`` implies, as an exact fraction
    (numerator, denominator = scale): a k x k conv at resolution r widens it by floor(k / 2) / r LR pixels; the transposed
    conv of scale s (k = 2 s - s % 2, padding (k - s) // 2) scatters an LR pixel over HR offsets -(k - s) // 2 .. k - 1 -
    (k - s) // 2, which is at most one LR pixel to either side."""
    s = cfg["scale"]
    res, num = 1, 0                                   # num / s LR pixels
    for op in oracle.build_topology(cfg):
        if op["op"] == "conv":
            num += (op["k"] // 2) * (s // res)
        elif op["op"] == "depth_to_space":
            res *= op["block"]
        elif op["op"] == "conv_transpose":
            num += s
            res *= op["scale"]
    return num, s


def true_reach(oracle, cfg, weights, sy, sx, margin=3):
    """(rows, columns): the farthest LR row and column at which a perturbed input pixel still moves the float64 oracle's output.

    One pixel of a U(0, 255) image, ``margin`` pixels inside the corner the diagonal (sy, sx) points to, is raised by 100 grey
    levels; an output pixel has moved when it differs by more than 1e-9 of max|branch|.  The image is sized so that the
    implied radius plus two more pixels fit between the pixel and the far borders: a reach beyond the implied radius is seen,
    not clipped."""
    s = cfg["scale"]
    num, den = implied_radius(oracle, cfg)
    side = -(-num // den) + 2 + 2 * margin
    h, w = side, side + 1
    x, x2 = reach_batch(1, h, w, s, seed=11)
    cy = h - 1 - margin if sy > 0 else margin
    cx = w - 1 - margin if sx > 0 else margin
    ref = oracle.forward(cfg, weights, x, x2, dtype=np.float64)
    xp = x.copy()
    xp[0, cy, cx, 0] += 100.0
    moved = np.abs(oracle.forward(cfg, weights, xp, x2, dtype=np.float64) - ref)[0, :, :, 0] > 1e-9 * np.max(np.abs(ref))
    rows, cols = np.nonzero(moved)
    assert rows.size, "the perturbed pixel moves nothing"
    rows, cols = rows // s - cy, cols // s - cx
    reach = (int(np.max(np.abs(rows))), int(np.max(np.abs(cols))))
    # the far side of the image is at least two pixels beyond what moved
    assert reach[0] + 2 <= (cy if sy > 0 else h - 1 - cy) and reach[1] + 2 <= (cx if sx > 0 else w - 1 - cx), (reach, h, w)
    return reach


def crop_change(oracle, cfg, weights, sy, sx, distance):
    """What a window edge ``distance`` LR pixels away does to the outermost pixels that window owns.

    LR row ``ky`` and column ``kx`` lie two pixels inside the image corner the diagonal (sy, sx) points AWAY from; the image is
    cropped ``distance`` rows and columns beyond them on the side the diagonal reads from, as a window with a halo of
    ``distance`` pixels would cut it, and the oracle runs on the crop.  Returns (rows, columns): the largest change of the
    outputs of LR row ``ky`` (over the columns up to ``kx``, the ones such a window owns) and of LR column ``kx`` (over the rows
    up to ``ky``), as a fraction of max|branch| of the whole image.  Zero when ``distance`` is the true reach or more."""
    s = cfg["scale"]
    h, w = distance + 6, distance + 8                # three resp. five rows / columns are cut off
    x, x2 = reach_batch(1, h, w, s, seed=12)
    ref = oracle.forward(cfg, weights, x, x2, dtype=np.float64)[0, :, :, 0]
    ys = slice(0, distance + 3) if sy > 0 else slice(h - distance - 3, h)
    xs = slice(0, distance + 3) if sx > 0 else slice(w - distance - 3, w)
    ky = 2 if sy > 0 else distance                   # in the crop's coordinates
    kx = 2 if sx > 0 else distance
    xc = np.ascontiguousarray(x[:, ys, xs])
    got = oracle.forward(cfg, weights, xc, np.zeros((1, xc.shape[1] * s, xc.shape[2] * s, 1), np.float32), dtype=np.float64)[0, :, :, 0]
    whole = ref[ys.start * s:ys.stop * s, xs.start * s:xs.stop * s]
    d = np.abs(got - whole) / np.max(np.abs(ref))
    own_y = slice(0, (ky + 1) * s) if sy > 0 else slice(ky * s, None)
    own_x = slice(0, (kx + 1) * s) if sx > 0 else slice(kx * s, None)
    return float(d[ky * s:(ky + 1) * s, own_x].max()), float(d[own_y, kx * s:(kx + 1) * s].max())
