"""Forwards through haloed windows (exec.hip: run_tiled) on every kernel, with weights that reach the halo.

Every case runs a net under the weights of tests/reach_weights.py (one corner tap per filter, all positive: the output depends
on the input pixel exactly the receptive-field radius away with O(1) weight; tests/test_tiling_host.py measures that a window
edge one pixel too near moves an owned pixel by 1400 .. 99000 x BAR) and checks the stitched output against the float64 oracle
of the WHOLE image at the plain 5e-6 bar of tests/bare_branch.py.  No float32-restatement clause: the restatement is within
BAR / 4 on these weights (asserted on the CPU).

* The library's R is read from the message of the EngineError that a budget of one byte raises -- the one place the library
  states it -- and must be at least the true reach that tests/test_tiling_host.py measures on the oracle.
* Evidence that a forward was tiled: engine A runs the whole image; engine B is fresh, has its budget set before its first
  forward and runs only the tiled one.  The arena only grows (plan.h: grow), so B's workspace is what windows need, and it must
  be smaller than A's.
* The bytes the library charges per LR pixel (exec.hip: pass_pixels) are read off refused forwards: the message states the
  pixels of a pass, and the smallest budget with a pass of one pixel is that figure.  With it ``_windows`` restates the window
  shapes and starts of run_tiled for a budget, which is how the cases are chosen and their geometry is asserted (three windows
  or more per axis, an irregular last one; stride 1; one-axis tiling) -- never how an expected VALUE is computed.

A failure names the case, the kernel list of ``eng.ops()``, R, the windows, the output pixel of the worst error with its
distance to the four image borders, and the error of the untiled forward of the same engine options."""
import re

import numpy as np
import pytest

import reach_weights as RW
import test_bare_branch_surface_hip as S
import test_tiling_host as H
from conftest import CONFIGS

pytestmark = pytest.mark.gpu

KERNEL_NAMES = S.KERNEL_NAMES                   # exec.hip: kernel_name
TRUE_REACH = {name: reach for name, _, reach in H.NETS}
NET_FLAGS = {name: flags for name, flags, _ in H.NETS}
NO_BUDGET = 1 << 40

_RAN = set()                                    # node ids of this file's tests that started
_CASES = []                                     # (leg, label, relative error)
_REACH = {k: 0 for k in KERNEL_NAMES}           # tiled cases whose launch list holds the kernel
_RADII = {}                                     # case label -> (library R, true reach)
_REFS = {}


def _engine(cfg, weights, load=None, options=()):
    from dcscn_amd import engine
    eng = engine.Engine(cfg, device=0)
    try:
        for key, value in options:
            eng.set_option(key, value)
        eng.load_weights(weights, **(load or {}))
    except Exception:
        eng.close()
        raise
    return eng


def _forward_under(eng, budget, x, x2):
    """``forward(x, x2)`` under ``budget``: (None, y), or (the message of the EngineError it raises, None); the status is NOMEM."""
    from dcscn_amd import engine
    eng.set_option("workspace_budget_bytes", budget)
    try:
        return None, eng.forward(x, x2)
    except engine.EngineError as exc:
        assert engine.STATUS_NAMES.get(exc.status) == "NOMEM", exc
        return str(exc), None


def _refusal(eng, budget, x, x2):
    return _forward_under(eng, budget, x, x2)[0]


def _probe(scale):
    return np.full((1, 4, 4, 1), 7.0, np.float32), np.zeros((1, 4 * scale, 4 * scale, 1), np.float32)


def _library_radius(eng, scale):
    """R of exec.hip: halo_lr_pixels, from '... with a %d-pixel halo' of the refusal of a one-byte budget."""
    msg = _refusal(eng, 1, *_probe(scale))
    assert msg is not None, "a budget of one byte was not refused"
    found = re.search(r"with a (\d+)-pixel halo", msg)
    assert found, msg
    return int(found.group(1))


def _bytes_per_pixel(eng, scale, guess):
    """exec.hip: pass_pixels' workspace bytes per LR pixel = the smallest budget whose refusal states a pass of one pixel."""
    x, x2 = _probe(scale)

    def pixels(budget):
        msg = _refusal(eng, budget, x, x2)
        if msg is None:
            return x.size                       # ran: a pass of at least the probe image
        found = re.search(r"a pass of (\d+) LR pixels", msg)
        assert found, msg
        return int(found.group(1))

    hi = max(int(guess), 1)
    while pixels(hi) < 1:
        hi *= 2
    lo = 0                                      # pixels(lo) < 1 <= pixels(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pixels(mid) < 1:
            lo = mid
        else:
            hi = mid
    assert pixels(hi) == 1 and pixels(2 * hi) == 2 and pixels(2 * hi - 1) == 1, hi
    return hi


def _windows(pass_px, h, w, r):
    """run_tiled's window shape and starts for a pass of ``pass_px`` LR pixels: (Ht, Wt, ys, xs), or None where it refuses."""
    ht = min(h, max(1, int(np.floor(np.sqrt(float(pass_px))))))
    wt = min(w, max(1, pass_px // ht))
    if wt == w:
        ht = min(h, pass_px // wt)
    if (ht < h and ht <= 2 * r) or (wt < w and wt <= 2 * r):
        return None

    def starts(full, win):
        if win >= full:
            return [0]
        out = list(range(0, full - win, win - 2 * r))
        return out + [full - win]

    return ht, wt, starts(h, ht), starts(w, wt)


def _describe(geometry):
    ht, wt, ys, xs = geometry
    return "windows %d x %d, rows at %s, columns at %s" % (ht, wt, ys, xs)


def _reference(oracle, key, cfg, weights, x, x2):
    if key not in _REFS:
        ref = oracle.forward(cfg, weights, x, x2, dtype=np.float64)
        ref.flags.writeable = False
        assert float(np.max(np.abs(ref))) > 0.0
        _REFS[key] = ref
    return _REFS[key]


def _judge(leg, label, y, ref, kernels, detail):
    """Tally the tiled case; None or the failure message."""
    assert y.shape == ref.shape, (label, y.shape, ref.shape)
    for k in set(kernels):
        _REACH[k] += 1
    if not np.isfinite(y).all():
        _CASES.append((leg, label, float("inf")))
        return "%s [%s]: output not finite; kernels %s; %s" % (label, leg, kernels, detail)
    rel = RW.rel_error(y, ref)
    _CASES.append((leg, label, rel))
    print("TILED %s | %s | rel %.3g | max|branch| %.3g | %s | %s" % (leg, label, rel, float(np.max(np.abs(ref))), detail, ",".join(kernels)))
    if rel <= RW.BAR:
        return None
    return "%s [%s]: relative error %.3g > %.1g\n  kernels: %s\n  %s\n  worst at %s" % (
        label, leg, rel, RW.BAR, kernels, detail, RW.worst_pixel(y, ref))


def _finish(failures):
    failures = [f for f in failures if f]
    if failures:
        pytest.fail("\n".join(failures))


# ---------------------------------------------------------------------------------------------
# 1. the shipped nets and the flag variants
# ---------------------------------------------------------------------------------------------
_F32 = dict(split16=False)
# (net of test_tiling_host.NETS, images, plan name, load_weights keywords, options, kernels the plan must hold)
PLANS = [
    ("L12_F196to48_x2", 1, "default", {}, (), ()),
    ("L12_F196to48_x4", 1, "default", {}, (), ("conv5_h",)),
    ("L8_F96to48_x2", 1, "default", {}, (), ()),
    ("L8_F96to48_x2", 1, "split16 0", _F32, (), ()),
    ("L2_F4to4_x2", 1, "default", {}, (), ()),
]
for _scale in (2, 3, 4):
    PLANS += [("L7_F32to8_x%d" % _scale, 2, "default", {}, (), ("feat3_stream",) + (("conv5_h",) if _scale > 2 else ())),
              ("L7_F32to8_x%d" % _scale, 2, "split16 0", _F32, (), ("layer by layer",)),
              ("L7_F32to8_x%d" % _scale, 2, "fold_tail False", dict(fold_tail=False), (), ("feat3_stream",))]
PLANS += [("L7_F32to8_x4_DS", 2, "default", {}, (), ("feat_stream", "conv5_h")),
          ("L7_F32to8_x4_DS", 2, "split16 0", _F32, (), ()),
          ("L7_F32to8_x4_DS", 2, "fold_whole_tail 0", {}, (("fold_whole_tail", 0),), ("feat_stream", "tail_stream"))]
# the flag variants, on layers = 3, filters = 16, min_filters = 8
PLANS += [(name, 1, "default", {}, (), ()) for name in
          ("cnn_size5", "cnn_size7", "reconstruct2", "no_nin", "transposed_x2", "transposed_x3", "transposed_x4", "separable5")]
PLANS += [("small", 1, "winograd False", dict(winograd=False), (), ())]
NET_CASES = [plan + (diagonal,) for plan in PLANS for diagonal in RW.DIAGONALS[:2]]


def _tiled_forward(oracle, name, n, plan, load, options, want, diagonal):
    """Engine A: R, the whole image, bytes per pixel.  Engine B, fresh: the budget, then the tiled forward alone.  Returns what the
    judgement needs; asserts R, the workspace evidence and the geometry."""
    sy, sx = diagonal
    cfg = oracle.make_config(**NET_FLAGS[name])
    scale = cfg["scale"]
    weights = RW.reach_weights(cfg, sy, sx, seed=3)
    label = "%s (%+d, %+d) %s" % (name, sy, sx, plan)
    with _engine(cfg, weights, load, options) as a:
        kernels = [op["kernel"] for op in a.ops()]
        for k in want:
            assert k in kernels, (label, kernels)
        r = _library_radius(a, scale)
        _RADII[label] = (r, TRUE_REACH[name])
        h, w = 2 * r + 13, 2 * r + 19           # at most 2 R + 24
        x, x2 = RW.reach_batch(n, h, w, scale, seed=21)
        a.set_option("workspace_budget_bytes", NO_BUDGET)
        whole = a.forward(x, x2)
        a_bytes = a.workspace_bytes()
        per_px = a_bytes // (n * h * w) + 1
        budget = per_px * (2 * r + 4) * (2 * r + 7)
        charged = _bytes_per_pixel(a, scale, per_px)
    geometry = _windows(budget // charged, h, w, r)
    assert geometry is not None, (label, budget, charged)
    ht, wt, ys, xs = geometry
    detail = "R %d (true reach %d), image %d x %d x %d, %s" % (r, TRUE_REACH[name], n, h, w, _describe(geometry))
    assert len(ys) >= 3 and len(xs) >= 3, (label, detail)
    assert ys[-1] - ys[-2] != ht - 2 * r and xs[-1] - xs[-2] != wt - 2 * r, (label, detail)     # an irregular last window
    with _engine(cfg, weights, load, options) as b:
        b.set_option("workspace_budget_bytes", budget)
        y = b.forward(x, x2)
        b_bytes = b.workspace_bytes()
    assert 0 < b_bytes < a_bytes, "%s: the tiled engine's workspace is %d bytes, the whole image's %d; %s" % (label, b_bytes, a_bytes, detail)
    # judged behind the stitched values, so that a halo that is too short shows in both
    short = None if r >= TRUE_REACH[name] else "%s: the library's halo is %d pixels, the graph reaches %d" % (label, r, TRUE_REACH[name])
    return cfg, weights, x, x2, whole, y, kernels, label, detail, short


@pytest.mark.parametrize("name,n,plan,load,options,want,diagonal", NET_CASES,
                         ids=["%s-%s-%s" % (c[0], c[2].replace(" ", "_"), "pp" if c[6][0] > 0 else "mm") for c in NET_CASES])
def test_tiled_forward_on_reach_weights(oracle, request, name, n, plan, load, options, want, diagonal):
    _RAN.add(request.node.nodeid)
    leg = "shipped nets" if name in CONFIGS else "flag variants"
    cfg, weights, x, x2, whole, y, kernels, label, detail, short = _tiled_forward(oracle, name, n, plan, load, options, want, diagonal)
    ref = _reference(oracle, (name, diagonal, x.shape), cfg, weights, x, x2)
    detail += "; untiled forward of the same options: %.3g" % RW.rel_error(whole, ref)
    _finish([_judge(leg, label, y, ref, kernels, detail), short])


# ---------------------------------------------------------------------------------------------
# 2. window geometry
# ---------------------------------------------------------------------------------------------
GEOMETRY_SHAPES = [(23, 31), (31, 23)]          # wider than tall: one-axis tiling cuts columns; taller than wide: rows


def _sweep(h, w, r):
    """Passes (LR pixels) from below (2 R + 1)^2 to the image area whose windows grow by one pixel on one side at a time."""
    out = []
    for t in range(2 * r - 1, max(h, w) + 1):
        out += [t * t, t * (t + 1)]
    out = [p for p in out if p < h * w]
    if h > w:                                   # windows as wide as the image and t rows tall
        out += [w * t for t in range(w, h)]
    return sorted(set(out + [h * w - 1]))


@pytest.mark.parametrize("shape", GEOMETRY_SHAPES, ids=["23x31", "31x23"])
@pytest.mark.parametrize("diagonal", RW.DIAGONALS, ids=["pp", "mm", "pm", "mp"])
def test_window_geometry(oracle, request, diagonal, shape):
    """Every budget of the sweep is refused with NOMEM or meets the bar, as ``_windows`` says; a forward behind a refusal is right."""
    _RAN.add(request.node.nodeid)
    sy, sx = diagonal
    h, w = shape
    cfg = oracle.make_config(**NET_FLAGS["tiny"])
    weights = RW.reach_weights(cfg, sy, sx, seed=3)
    x, x2 = RW.reach_batch(2, h, w, 2, seed=22)
    ref = _reference(oracle, ("tiny", diagonal, x.shape), cfg, weights, x, x2)
    failures = []
    seen = dict(refused=0, stride1=0, one_axis=0, last_gap1=0, after_refusal=0)
    with _engine(cfg, weights) as eng:
        kernels = [op["kernel"] for op in eng.ops()]
        r = _library_radius(eng, 2)
        if r < TRUE_REACH["tiny"]:
            failures.append("tiny: the library's halo is %d pixels, the graph reaches %d" % (r, TRUE_REACH["tiny"]))
        _RADII["tiny (%+d, %+d) %dx%d" % (sy, sx, h, w)] = (r, TRUE_REACH["tiny"])
        charged = _bytes_per_pixel(eng, 2, 4096)
        passes = _sweep(h, w, r)
        assert passes[0] < (2 * r + 1) ** 2 <= passes[-1]
        refused_before = False
        for px in passes + [passes[0], (2 * r + 3) * (2 * r + 4)]:      # at the end: a refusal, then an accepted budget once more
            geometry = _windows(px, h, w, r)
            label = "tiny (%+d, %+d) 2x%dx%d, pass of %d pixels" % (sy, sx, h, w, px)
            msg, y = _forward_under(eng, px * charged, x, x2)
            if geometry is None:
                assert msg is not None and "a pass of %d LR pixels" % px in msg, (label, msg)
                seen["refused"] += 1
                refused_before = True
                continue
            assert msg is None, (label, msg, _describe(geometry))
            ht, wt, ys, xs = geometry
            seen["stride1"] += ht == 2 * r + 1 and wt == 2 * r + 1
            seen["one_axis"] += (ht == h and wt < w) if h < w else (wt == w and ht < h)     # columns cut on 23 x 31, rows on 31 x 23
            seen["last_gap1"] += (len(ys) > 1 and ys[-1] - ys[-2] == 1) or (len(xs) > 1 and xs[-1] - xs[-2] == 1)
            seen["after_refusal"] += refused_before
            refused_before = False
            failures.append(_judge("window geometry", label, y, ref, kernels, "R %d, %s" % (r, _describe(geometry))))
        # sub_batch_pixels below one window: the window batch runs as passes of one window
        px = (2 * r + 3) * (2 * r + 4)
        eng.set_option("workspace_budget_bytes", px * charged)
        eng.set_option("sub_batch_pixels", px - 1)
        failures.append(_judge("window geometry", "tiny (%+d, %+d) 2x%dx%d, sub_batch_pixels %d" % (sy, sx, h, w, px - 1),
                               eng.forward(x, x2), ref, kernels, "R %d, %s" % (r, _describe(_windows(px, h, w, r)))))
    print("GEOMETRY %dx%d (%+d, %+d): %d budgets, %r" % (h, w, sy, sx, len(passes) + 2, seen))
    assert seen["refused"] >= 2 and seen["stride1"] >= 1 and seen["one_axis"] >= 1 and seen["last_gap1"] >= 1 and seen["after_refusal"] >= 2, seen
    _finish(failures)


# ---------------------------------------------------------------------------------------------
# 3. the other entry points on windows
# ---------------------------------------------------------------------------------------------
def test_self_ensemble_on_windows(oracle, request):
    """forward_ensemble(8) of a 34 x 52 image under a budget that tiles the [h, w] group and the [w, h] group."""
    _RAN.add(request.node.nodeid)
    cfg = oracle.make_config(**NET_FLAGS["small"])
    weights = RW.reach_weights(cfg, 1, 1, seed=3)
    h, w = 34, 52
    x, x2 = RW.reach_batch(1, h, w, 2, seed=23)
    with _engine(cfg, weights) as a:
        kernels = [op["kernel"] for op in a.ops()]
        r = _library_radius(a, 2)
        a.set_option("workspace_budget_bytes", NO_BUDGET)
        a.forward_ensemble(x[0], x2[0], 8)
        a_bytes = a.workspace_bytes()
        charged = _bytes_per_pixel(a, 2, a_bytes // (4 * h * w) + 1)
    px = (2 * r + 4) * (2 * r + 7)
    geometries = [_windows(px, h, w, r), _windows(px, w, h, r)]
    for g in geometries:
        assert g is not None and len(g[2]) >= 2 and len(g[3]) >= 2, geometries
    with _engine(cfg, weights) as b:
        b.set_option("workspace_budget_bytes", px * charged)
        y = b.forward_ensemble(x[0], x2[0], 8)
        b_bytes = b.workspace_bytes()
    assert 0 < b_bytes < a_bytes, (b_bytes, a_bytes)
    ref = oracle.do(cfg, weights, x[0], x2[0], self_ensemble=8)
    assert y.dtype == np.float64
    _finish([_judge("self-ensemble", "small (+1, +1) forward_ensemble 8, 34x52", y[None], ref[None], kernels,
                    "R %d, %s; turned: %s" % (r, _describe(geometries[0]), _describe(geometries[1]))),
             None if r >= TRUE_REACH["small"] else "the library's halo is %d pixels, the graph reaches %d" % (r, TRUE_REACH["small"])])


def test_forward_lr_on_windows_equals_forward_with_the_pillow_bicubic(oracle, request):
    """The bicubic image computed on the device and the one of Pillow give the same bits through windows."""
    _RAN.add(request.node.nodeid)
    cfg = oracle.make_config(**NET_FLAGS["small"])
    weights = RW.reach_weights(cfg, -1, -1, seed=3)
    n, h, w = 2, 29, 41
    x, _ = RW.reach_batch(n, h, w, 2, seed=24)
    x2 = np.stack([oracle.pil_bicubic(x[i], 2) for i in range(n)]).astype(np.float32)
    ref = oracle.forward(cfg, weights, x, x2, dtype=np.float64)
    with _engine(cfg, weights) as a:
        kernels = [op["kernel"] for op in a.ops()]
        r = _library_radius(a, 2)
        a.set_option("workspace_budget_bytes", NO_BUDGET)
        a.forward_lr(x)
        a_bytes = a.workspace_bytes()
        charged = _bytes_per_pixel(a, 2, a_bytes // (n * h * w) + 1)
    px = (2 * r + 4) * (2 * r + 7)
    geometry = _windows(px, h, w, r)
    assert geometry is not None and len(geometry[2]) >= 2 and len(geometry[3]) >= 2, geometry
    with _engine(cfg, weights) as b:
        b.set_option("workspace_budget_bytes", px * charged)
        y_lr = b.forward_lr(x)
        b_bytes = b.workspace_bytes()
        y = b.forward(x, x2)
    assert 0 < b_bytes < a_bytes, (b_bytes, a_bytes)
    assert np.array_equal(y_lr, y), "forward_lr and forward differ in %d values" % int((y_lr != y).sum())
    _finish([_judge("forward_lr", "small (-1, -1) forward_lr 2x29x41", y_lr, ref, kernels, "R %d, %s" % (r, _describe(geometry)))])


# ---------------------------------------------------------------------------------------------
# 4. what the file reached
# ---------------------------------------------------------------------------------------------
N_TESTS = len(NET_CASES) + len(GEOMETRY_SHAPES) * len(RW.DIAGONALS) + 2


def _whole_file_ran():
    if len(_RAN) != N_TESTS:
        pytest.skip("%d of this file's %d tiled tests ran before this one: it speaks about the whole file" % (len(_RAN), N_TESTS))


def test_every_kernel_name_was_reached_by_a_tiled_case():
    """Every name of exec.hip: kernel_name is in the launch list of at least one tiled case of this file."""
    _whole_file_ran()
    print("REACH tiled cases per kernel (of %d)" % len(_CASES))
    for k in KERNEL_NAMES:
        print("REACH %-16s %d" % (k, _REACH[k]))
    legs = {}
    for leg, label, rel in _CASES:
        if leg not in legs or rel > legs[leg][0]:
            legs[leg] = (rel, label)
    for leg in sorted(legs):
        print("WORST %s: %.3g on %s" % (leg, legs[leg][0], legs[leg][1]))
    for label in sorted(_RADII):
        print("RADIUS %s: library %d, true reach %d, difference %d" % ((label,) + _RADII[label] + (_RADII[label][0] - _RADII[label][1],)))
    assert set(_REACH) == set(KERNEL_NAMES), sorted(set(_REACH) - set(KERNEL_NAMES))
    assert not [k for k in KERNEL_NAMES if _REACH[k] == 0], _REACH
