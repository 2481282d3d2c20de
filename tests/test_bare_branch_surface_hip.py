"""The inference kernels on the BARE network branch over the random flag surface, the strip and row-block edges of the streamed
kernels and the hand-picked flag surface.

The attenuated 1e-4 check (last conv x 0.01, bicubic term added) that test_random_configs.py, test_flag_surface,
test_ragged_sizes and test_streamed_dense_feature_extractor apply is worth between 5.4e-6 and 0.25 relative on the branch (median
3.2e-5); filters that lost their f16 ``lo`` piece pass it (tests/test_bare_branch_host.py).  Here the same nets, sizes and engine
options meet the 5e-6 relative bar of test_residual_branch_relative_error against ``oracle.forward(..., float64)``, with the rule
of tests/bare_branch.py for a case beyond it: within 4 x its own float32 restatement's error, for at most 2 % of the cases.

A failure names the case, the kernel list of ``eng.ops()``, the output pixel of the worst error with its distance to the four
image borders, and the error of a ``split16 = 0`` run of the same case.

Measured on an MI355X (557 cases, none beyond 5e-6): walk 3.22e-6 (draw 155), walk with split16 off 2.06e-6 (draw 35), forced
tiling 1.14e-6 (draw 19), feat3_stream 8.33e-7, feat_stream 7.74e-7, tail_stream 3.79e-7, flag surface 2.21e-6; the tables are
in DESIGN.md section 4."""
import numpy as np
import pytest

import bare_branch as B
import test_hip_parity as P
from conftest import CONFIGS

pytestmark = pytest.mark.gpu

# exec.hip: kernel_name
KERNEL_NAMES = ("conv_igemm", "conv_wino2", "conv_nin", "conv_nin_h", "conv5_h", "conv3_h8", "conv3_h", "conv_cin1", "conv_cout1",
                "depthwise", "feat_stream", "tail_stream", "feat3_stream", "layer by layer")

_RAN = set()                                    # node ids of this file's tests that started
_CASES = []                                     # (leg, label, relative error, used the float32-restatement clause)
_REACH = {k: 0 for k in KERNEL_NAMES}           # bare-branch cases whose launch list holds the kernel


def _forward(cfg, weights, x, x2, load=None, options=()):
    """(y, kernel list) of one engine: ``options`` before load_weights, ``load`` = load_weights' keywords."""
    from dcscn_amd import engine
    with engine.Engine(cfg, device=0) as eng:
        for key, value in options:
            eng.set_option(key, value)
        eng.load_weights(weights, **(load or {}))
        kernels = [op["kernel"] for op in eng.ops()]
        y = eng.forward(x, x2)
    return y, kernels


def _judge(oracle, leg, label, y, kernels, ref, cfg, weights, x, x2, load=None, options=()):
    """Tally the case and return None, or the failure message."""
    assert y.shape == ref.shape and y.dtype == np.float32, (label, y.shape, ref.shape)
    for k in set(kernels):
        _REACH[k] += 1
    if not np.isfinite(y).all():
        _CASES.append((leg, label, float("inf"), True))
        return "%s [%s]: output not finite; kernels %s" % (label, leg, kernels)
    rel = B.rel_error(y, ref)
    print("BARE %s | %s | rel %.3g | max|branch| %.3g | %s" % (leg, label, rel, float(np.max(np.abs(ref))), ",".join(kernels)))
    if rel <= B.BAR:
        _CASES.append((leg, label, rel, False))
        return None
    _CASES.append((leg, label, rel, True))
    r32 = B.restatement_error(oracle, cfg, weights, x, x2, ref)
    print("BARE %s | %s | beyond %.1g: float32 restatement %.3g, bound %.3g" % (leg, label, B.BAR, r32, B.RESTATEMENT_FACTOR * r32))
    if rel <= B.RESTATEMENT_FACTOR * r32:
        return None
    y0, k0 = _forward(cfg, weights, x, x2, dict(load or {}, split16=False), options)
    return ("%s [%s]: relative error %.3g > %.1g and > %g x the float32 restatement's %.3g\n  kernels: %s\n  worst at %s\n"
            "  split16 = 0 run (untiled) of the same case: %.3g, worst at %s\n  its kernels: %s"
            % (label, leg, rel, B.BAR, B.RESTATEMENT_FACTOR, r32, kernels, B.worst_pixel(y, ref), B.rel_error(y0, ref),
               B.worst_pixel(y0, ref), k0))


def _finish(failures):
    failures = [f for f in failures if f]
    if failures:
        pytest.fail("\n".join(failures))


def _reference(oracle, cfg, weights, x, x2):
    ref = oracle.forward(cfg, weights, x, x2, dtype=np.float64)
    ref.flags.writeable = False
    assert float(np.max(np.abs(ref))) > 0.0
    return ref


# ---------------------------------------------------------------------------------------------
# 1. the random walk of test_random_configs.py on the bare branch
# ---------------------------------------------------------------------------------------------
_WALK = {}                                      # seed -> case with its float64 reference, for the draws both legs run


def _walk_case(oracle, seed):
    if seed not in _WALK:
        flags, cfg, weights, x, x2, opts = B.walk_draw(oracle, seed)
        case = (flags, cfg, weights, x, x2, opts, _reference(oracle, cfg, weights, x, x2))
        if seed >= 60:
            return case
        _WALK[seed] = case
    return _WALK[seed]


def _walk(oracle, seed, split16, leg):
    """test_random_configs._run_draw with bare weights and x2 = 0: the drawn winograd and fold, and the forced tiling leg."""
    from dcscn_amd import engine
    flags, cfg, weights, x, x2, opts, ref = _walk_case(oracle, seed)
    n, h, w = x.shape[:3]
    load = dict(winograd=opts["winograd"], fold_tail=opts["fold"], split16=split16)
    label = "walk draw %d: %r n %d h %d w %d %r" % (seed, flags, n, h, w, opts)
    yt = None
    with engine.Engine(cfg, device=0) as eng:
        eng.load_weights(weights, **load)
        kernels = [op["kernel"] for op in eng.ops()]
        y = eng.forward(x, x2)
        if opts["tile"] and h * w >= 600:
            per_px = eng.workspace_bytes() // (n * h * w) + 1
            eng.set_option("workspace_budget_bytes", per_px * (h * w // 2))
            try:
                yt = eng.forward(x, x2)
            except engine.EngineError:
                yt = None                       # windows smaller than the halo: a reported error, not a crash
    failures = [_judge(oracle, leg, label, y, kernels, ref, cfg, weights, x, x2, load)]
    if yt is not None:
        failures.append(_judge(oracle, "tiled", label + " (tiled)", yt, kernels, ref, cfg, weights, x, x2, load))
    _finish(failures)


@pytest.mark.parametrize("seed", range(200))
def test_random_flag_surface_bare_branch(oracle, request, seed):
    """The 200 draws of test_random_flag_surface; the tiled result meets the same bar against the oracle of the whole image."""
    _RAN.add(request.node.nodeid)
    _walk(oracle, seed, None, "walk default")   # library default: split16 on


@pytest.mark.parametrize("seed", range(60))
def test_random_flag_surface_bare_branch_f32_kernels(oracle, request, seed):
    """The first 60 draws with split16 off, against the reference the default leg computed."""
    _RAN.add(request.node.nodeid)
    _walk(oracle, seed, False, "walk f32")


# ---------------------------------------------------------------------------------------------
# 2. the streamed kernels where strips and row blocks end
# ---------------------------------------------------------------------------------------------
STREAM_PX = 48                                  # kernels.h: kStreamPX, computed columns per strip


def _geometry(n, h, w, halo):
    """exec.hip: stream_geometry -> (strips, columns the last strip stores, row blocks, rows the last block stores)."""
    if w <= STREAM_PX:
        strips, useful_w = 1, w
    else:
        useful_w = STREAM_PX - 2 * halo
        strips = -(-w // useful_w)
    cols = n * strips
    want = max(1, -(-512 // cols))
    useful_h = max(32, -(-h // want))
    blocks = -(-h // useful_h)
    return strips, w - (strips - 1) * useful_w, blocks, h - (blocks - 1) * useful_h


def _edge_shapes(halo, only_one_wide=False):
    """[(id, n, H, W)] for a streamed kernel of this halo.  Strips start at W = 49 and store 48 - 2 halo columns each; with one
    image and one strip a row block stores 32 rows, so blocks start at H = 33."""
    u = STREAM_PX - 2 * halo
    shapes = [("w48-one-strip", 1, 20, 48, (1, 48, 1, 20)),
              ("w49", 1, 20, 49, (2, 49 - u, 1, 20)),
              ("last-strip-one-column", 1, 9, 2 * u + 1, (3, 1, 1, 9)),
              ("h32-one-block", 1, 32, 20, (1, 20, 1, 32)),
              ("h33-last-block-one-row", 1, 33, 20, (1, 20, 2, 1)),
              ("h65-last-block-one-row", 1, 65, 20, (1, 20, 3, 1)),
              ("strips-and-blocks", 1, 65, 2 * u + 1, (3, 1, 3, 1)),
              ("batch-of-3", 3, 33, 49, (2, 49 - u, 2, 1))]
    for name, n, h, w, want in shapes:
        assert _geometry(n, h, w, halo) == want, (name, halo, _geometry(n, h, w, halo), want)
        assert n <= 3 and h <= 70 and w <= 110
    if only_one_wide:
        shapes = [s for s in shapes if s[4][1] == 1 or s[4][3] == 1]
    return [s[:4] for s in shapes]


def _stream_case(oracle, flags, n, h, w, seed):
    cfg = oracle.make_config(**flags)
    weights = B.bare_weights(cfg, oracle.synthetic_weights(cfg, seed=seed))
    x, x2 = B.bare_batch(n, h, w, cfg["scale"], seed + 1)
    return cfg, weights, x, x2, _reference(oracle, cfg, weights, x, x2)


def _run_plans(oracle, leg, label, case, plans):
    """``plans``: [(plan name, options, kernels that must be in the list, kernels that must not)]; every plan meets the bar."""
    cfg, weights, x, x2, ref = case
    failures = []
    for name, options, present, absent in plans:
        y, kernels = _forward(cfg, weights, x, x2, options=options)
        for k in present:
            assert k in kernels, (label, name, kernels)
        for k in absent:
            assert k not in kernels, (label, name, kernels)
        failures.append(_judge(oracle, "%s (%s)" % (leg, name), "%s, plan %s" % (label, name), y, kernels, ref, cfg, weights, x, x2,
                               options=options))
    _finish(failures)


# feat3_stream (graph.hip: fuse_feat3_stream): any non-separable 3x3 net of 2 .. 8 feature layers of <= 32 channels.  Conv i of the
# launch runs on s3_conv_role<octets = ceil(cin / 8), tiles = ceil(cout / 16)> (feat3_stream.hpp); the roles of each net's schedule
# (oracle.filter_schedule) are listed behind it and checked by test_feat3_nets_reach_every_reachable_role.  <1, 2> and <2, 2> are
# instantiated but UNREACHABLE: two output tiles need cout >= 17, a schedule never grows, so cin >= 17 and octets >= 3.
# None of these is a shipped shape (32 .. 8 over 7 layers); depths 2, 5 and 8, scales 2, 3 and 4.
_S3_NIN = dict(nin_filters=24, nin_filters2=8)
S3_NETS = [
    ("L2-32to32-x2", dict(layers=2, filters=32, min_filters=32, scale=2, **_S3_NIN), {(4, 2)}),
    ("L2-32to16-x3", dict(layers=2, filters=32, min_filters=16, scale=3, pixel_shuffler_filters=1, **_S3_NIN), {(4, 1)}),
    ("L5-24to24-x3", dict(layers=5, filters=24, min_filters=24, scale=3, **_S3_NIN), {(3, 2)}),
    ("L5-24to12-x4", dict(layers=5, filters=24, min_filters=12, filters_decay_gamma=1.0, scale=4, pixel_shuffler_filters=1, **_S3_NIN),
     {(3, 2), (3, 1), (2, 1)}),
    ("L5-32to32-x2", dict(layers=5, filters=32, min_filters=32, scale=2, pixel_shuffler_filters=4, **_S3_NIN), {(4, 2)}),
    ("L8-16to16-x4", dict(layers=8, filters=16, min_filters=16, scale=4, pixel_shuffler_filters=4, **_S3_NIN), {(2, 1)}),
    ("L8-8to8-x2", dict(layers=8, filters=8, min_filters=8, scale=2, **_S3_NIN), {(1, 1)}),
    # 32, 23, 18, 14, 10, 7, 4, 1: a one-channel last layer
    ("L8-32to1-x3", dict(layers=8, filters=32, min_filters=1, filters_decay_gamma=1.5, scale=3, pixel_shuffler_filters=2, **_S3_NIN),
     {(4, 2), (3, 2), (3, 1), (2, 1), (1, 1)}),
]
S3_REACHABLE = {(o, t) for o in (1, 2, 3, 4) for t in (1, 2)} - {(1, 2), (2, 2)}
S3_CASES = [(name, flags, shape) for name, flags, _ in S3_NETS for shape in _edge_shapes(flags["layers"])]


def _roles(oracle, flags):
    sched = oracle.filter_schedule(flags["layers"], flags["filters"], flags["min_filters"], flags.get("filters_decay_gamma", 1.5))
    return sched, {((sched[i] + 7) // 8, (sched[i + 1] + 15) // 16) for i in range(len(sched) - 1)}


def test_feat3_nets_reach_every_reachable_role(oracle, request):
    _RAN.add(request.node.nodeid)
    reached = set()
    for name, flags, roles in S3_NETS:
        sched, got = _roles(oracle, flags)
        assert max(sched) <= 32 and sched == sorted(sched, reverse=True) and got == roles, (name, sched, got)
        reached |= got
    assert sched[-1] == 1
    assert reached == S3_REACHABLE
    assert {f["layers"] for _, f, _ in S3_NETS} == {2, 5, 8} and {f["scale"] for _, f, _ in S3_NETS} == {2, 3, 4}


@pytest.mark.parametrize("name,flags,shape", S3_CASES, ids=["%s-%s" % (c[0], c[2][0]) for c in S3_CASES])
def test_feat3_stream_edges_bare_branch(oracle, request, name, flags, shape):
    """Non-shipped nets on feat3_stream (halo = layers) and, stream_dense = 0, on their layers' own launches."""
    _RAN.add(request.node.nodeid)
    sid, n, h, w = shape
    case = _stream_case(oracle, flags, n, h, w, seed=50 + flags["layers"])
    _run_plans(oracle, "feat3_stream", "%s %s %dx%dx%d" % (name, sid, n, h, w), case,
               [("streamed", (), ("feat3_stream",), ()),
                ("stream_dense 0", (("stream_dense", 0),), (), ("feat3_stream",))])


# the shipped 32 .. 8 shape: with A1 || B1 and B2 in the launch (stream_nin, halo L + 1 = 8) and without (halo L = 7)
S3_SHIPPED_CASES = [(scale, nin, shape) for scale in (2, 4) for nin in (1, 0) for shape in _edge_shapes(8 if nin else 7)]


@pytest.mark.parametrize("scale,nin,shape", S3_SHIPPED_CASES, ids=["x%d-stream_nin%d-%s" % (c[0], c[1], c[2][0]) for c in S3_SHIPPED_CASES])
def test_feat3_stream_shipped_shape_edges_bare_branch(oracle, request, scale, nin, shape):
    _RAN.add(request.node.nodeid)
    sid, n, h, w = shape
    case = _stream_case(oracle, CONFIGS["L7_F32to8_x%d" % scale], n, h, w, seed=60 + scale)
    plans = [("streamed", (("stream_nin", nin),), ("feat3_stream",), ())]
    if nin:
        plans.append(("stream_dense 0", (("stream_dense", 0),), (), ("feat3_stream",)))
    _run_plans(oracle, "feat3_stream shipped, stream_nin %d" % nin, "L7_F32to8_x%d %s %dx%dx%d" % (scale, sid, n, h, w), case, plans)


def _ds_flags(variant):
    layers, filters, min_filters, gamma, na, nb, scale, act = variant
    return dict(layers=layers, filters=filters, min_filters=min_filters, filters_decay_gamma=gamma, nin_filters=na, nin_filters2=nb,
                scale=scale, activator=act, depthwise_separable=True, reconstruct_layers=0, pixel_shuffler_filters=1)


# feat_stream (halo L + 1) and tail_stream (halo 2) on the shapes whose last strip stores one column or whose last block stores
# one row, for each kernel's own halo: C5's net (feat_stream + the folded tail; fold_whole_tail = 0: feat_stream + tail_stream) and
# the two of test_hip_parity.STREAM_VARIANTS that take feat_stream with other widths than the shipped ones (3 layers 32, 21, 17 at x4,
# 2 layers 16, 13 at x3: halos 4 and 3)
DS_NETS = [("C5", CONFIGS["L7_F32to8_x4_DS"]), ("variant5", _ds_flags(P.STREAM_VARIANTS[5])), ("variant6", _ds_flags(P.STREAM_VARIANTS[6]))]
DS_CASES = []
for _name, _flags in DS_NETS:
    _shapes = _edge_shapes(_flags["layers"] + 1, only_one_wide=True)
    if _name == "C5":
        _shapes += [("tail-" + s[0],) + s[1:] for s in _edge_shapes(2, only_one_wide=True) if s not in _shapes and s[3] > STREAM_PX]
    DS_CASES += [(_name, _flags, s) for s in _shapes]


@pytest.mark.parametrize("name,flags,shape", DS_CASES, ids=["%s-%s" % (c[0], c[2][0]) for c in DS_CASES])
def test_feat_stream_and_tail_stream_edges_bare_branch(oracle, request, name, flags, shape):
    _RAN.add(request.node.nodeid)
    sid, n, h, w = shape
    case = _stream_case(oracle, flags, n, h, w, seed=70 + flags["layers"])
    plans = [("default", (), ("feat_stream",) + (("conv5_h",) if name == "C5" else ()), ("tail_stream",))]
    if name == "C5":
        plans.append(("fold_whole_tail 0", (("fold_whole_tail", 0),), ("feat_stream", "tail_stream"), ()))
    _run_plans(oracle, "feat_stream / tail_stream", "%s %s %dx%dx%d" % (name, sid, n, h, w), case, plans)


# ---------------------------------------------------------------------------------------------
# 3. the hand-picked flag surface of test_hip_parity.py
# ---------------------------------------------------------------------------------------------
def _params(test, arg):
    """The value list a test function of test_hip_parity.py is parametrised with for ``arg``."""
    for mark in test.pytestmark:
        if mark.name == "parametrize" and mark.args[0] == arg:
            return list(mark.args[1])
    raise KeyError(arg)


FLAG_VARIANTS = _params(P.test_flag_surface, "variant")
RAGGED_SIZES = _params(P.test_ragged_sizes, "hw")
# the three nets in the body of test_ragged_sizes, with their batch sizes
RAGGED_NETS = [("L7_F32to8_x2", CONFIGS["L7_F32to8_x2"], 2),
               ("odd-channels", dict(layers=4, filters=37, min_filters=13, nin_filters=21, nin_filters2=10), 1),
               ("wide-odd", dict(layers=3, filters=70, min_filters=45, nin_filters=40, nin_filters2=33), 1)]


_SURFACE = {}


def _surface(oracle, leg, label, flags, n, h, w, split16, want=()):
    """test_hip_parity._check's weights (seed 0) and batch (seed 1), bare."""
    if label not in _SURFACE:                   # one reference for the two split16 legs
        _SURFACE[label] = _stream_case(oracle, flags, n, h, w, seed=0)
    cfg, weights, x, x2, ref = _SURFACE[label]
    load = dict(split16=split16)
    y, kernels = _forward(cfg, weights, x, x2, load)
    for k in want:
        assert k in kernels, (label, kernels)
    _finish([_judge(oracle, leg, "%s split16 %r" % (label, split16), y, kernels, ref, cfg, weights, x, x2, load)])


@pytest.mark.parametrize("split16", P.SPLIT16)
@pytest.mark.parametrize("variant", FLAG_VARIANTS, ids=[str(i) for i in range(len(FLAG_VARIANTS))])
def test_flag_surface_bare_branch(oracle, request, variant, split16):
    _RAN.add(request.node.nodeid)
    _surface(oracle, "flag surface", "flag surface %r 2x20x28" % (variant,), variant, 2, 20, 28, split16)


@pytest.mark.parametrize("split16", P.SPLIT16)
@pytest.mark.parametrize("hw", RAGGED_SIZES)
@pytest.mark.parametrize("net", RAGGED_NETS, ids=[n[0] for n in RAGGED_NETS])
def test_ragged_sizes_bare_branch(oracle, request, net, hw, split16):
    _RAN.add(request.node.nodeid)
    name, flags, n = net
    _surface(oracle, "flag surface", "ragged %s %dx%dx%d" % (name, n, hw[0], hw[1]), flags, n, hw[0], hw[1], split16)


# ---------------------------------------------------------------------------------------------
# 4. reach, and the use of the second clause
# ---------------------------------------------------------------------------------------------
def test_two_channel_groups_bare_branch(oracle, request):
    """conv3_h8 takes 3x3 layers of two channel groups (test_conv3_h8_is_bit_identical_to_conv3_h's 176 .. 112 net); the widest
    draw of the walk has 148 filters.  A ragged size, so that image-edge tiles take its general epilogue."""
    _RAN.add(request.node.nodeid)
    flags = dict(layers=3, filters=176, min_filters=112, filters_decay_gamma=1.0, nin_filters=48, nin_filters2=24)
    _surface(oracle, "two channel groups", "wide-3 2x19x37", flags, 2, 19, 37, None, want=("conv3_h8",))


N_TESTS = 200 + 60 + 1 + len(S3_CASES) + len(S3_SHIPPED_CASES) + len(DS_CASES) + 2 * len(FLAG_VARIANTS) + 2 * len(RAGGED_NETS) * len(RAGGED_SIZES) + 1


def _whole_file_ran():
    if len(_RAN) != N_TESTS:
        pytest.skip("%d of this file's %d tests ran before this one: it speaks about the whole file" % (len(_RAN), N_TESTS))


def test_every_kernel_name_was_reached_on_the_bare_branch():
    """Every name of exec.hip: kernel_name is in the launch list of at least one bare-branch case of this file."""
    _whole_file_ran()
    print("REACH bare-branch cases per kernel (of %d)" % len(_CASES))
    for k in KERNEL_NAMES:
        print("REACH %-16s %d" % (k, _REACH[k]))
    assert set(_REACH) == set(KERNEL_NAMES), sorted(set(_REACH) - set(KERNEL_NAMES))
    assert not [k for k in KERNEL_NAMES if _REACH[k] == 0], _REACH


def test_the_float32_restatement_clause_is_the_exception():
    """At most 2 % of the cases were beyond 5e-6 and passed (or failed) on their float32 restatement; the float64 reference's own
    float32 restatement needs the clause on none of the 200 draws."""
    _whole_file_ran()
    legs = {}
    for leg, label, rel, clause in _CASES:
        if leg not in legs or rel > legs[leg][0]:
            legs[leg] = (rel, label)
    for leg in sorted(legs):
        print("WORST %s: %.3g on %s" % (leg, legs[leg][0], legs[leg][1]))
    used = [(leg, label, rel) for leg, label, rel, clause in _CASES if clause]
    print("CLAUSE %d of %d cases used the float32-restatement clause" % (len(used), len(_CASES)))
    for leg, label, rel in used:
        print("CLAUSE   %s | %s | %.3g" % (leg, label, rel))
    assert len(used) <= 0.02 * len(_CASES), used
