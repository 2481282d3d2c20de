"""The f16-range fallback of the split16 path where the first value beyond the range arises BEHIND the input.

test_split16_overflow_falls_back_to_f32, test_p16_overflow_recomputes_the_image_on_the_float32_plan and
test_whole_tail_fold_flagged_image_takes_the_float32_plan multiply an input image by 4000: the first split16 launch of the pass flags
the image in every workgroup, and no detection site behind it ever decides an outcome.  Here one conv's filter and bias are scaled by a
power of two (tests/overflow_cases.py) so that the hot image -- or ONE pixel of it -- leaves the range at a chosen tensor and nowhere
before, and every case asserts the contract of "split16" in include/dcscn.h, and only that:

1. bystanders: every other image of the batch has the bits of a forward of the same handle on the clean batch;
2. value: the hot image is finite and within 5e-6 of the float64 oracle relative to max|ref| of that image (or, beyond that, within
   4 x its own float32 restatement's error: tests/bare_branch.py; at most 2 % of the file's cases);
3. independence: the hot image alone (n = 1) gives the bits it has inside the batch;
4. float32 plan, where the case is marked ``flagged``: the hot image equals a split16 = 0 forward of the same handle bit for bit, and the
   next clean forward equals the first clean one.

``flagged`` is set by hand per case and checked against the plan (overflow_cases.flag_expected on eng.ops(): a split16 launch reads the
tensor).  Nothing asserts that an image was NOT flagged: a spurious flag costs time, not correctness.

Legs: A every conv of the shipped nets; B one hot pixel; C the edge values 65504 .. nextafter(65520, inf) themselves, relayed bit for
bit; D sub-batched passes, forced tiling, graph replay, the self-ensemble; E the engine options; F the random walk.

Found by this file: with split16 = 3 the narrow nets' streamed launch runs layer by layer with A1 || B1 on conv_nin_h, and the pass
neither cleared its flags nor ran its float32 plan -- a hot image came out NaN (exec.hip: op_any_split16 is the fix).  Worst relative
errors per leg, the reach counts and the mutants are in DESIGN.md section 4."""
import numpy as np
import pytest

import dcscn_oracle
import overflow_cases as C
import test_hip_parity as P
from conftest import CONFIGS
from test_bare_branch_surface_hip import KERNEL_NAMES, _geometry

pytestmark = pytest.mark.gpu

# the names of exec.hip: kernel_name that run a split16 kernel (feat_stream / tail_stream: their F16 instantiation, the default)
SPLIT16_NAMES = C.SPLIT16_KERNELS + C.STREAM_KERNELS

_RAN = set()
_CASES = []                                     # (leg, label, relative error of the hot image, used the float32-restatement clause)
_REACH = {k: 0 for k in KERNEL_NAMES}           # hot cases whose launch list holds the kernel


def _engine(cfg, weights, options=(), load=None):
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


def _value(oracle, leg, label, y, ref, kernels, restate):
    """Clause 2 for one image: None or the failure message.  ``restate()`` -> the float32 restatement's error of that image."""
    for k in set(kernels):
        _REACH[k] += 1
    if not np.isfinite(y).all():
        _CASES.append((leg, label, float("inf"), True))
        return "%s [%s]: hot image not finite (%d of %d values); kernels %s" % (label, leg, int((~np.isfinite(y)).sum()), y.size, kernels)
    rel = C.rel_error(y, ref)
    print("HOT %s | %s | rel %.3g | max|ref| %.3g | %s" % (leg, label, rel, float(np.max(np.abs(ref))), ",".join(kernels)))
    if rel <= C.BAR:
        _CASES.append((leg, label, rel, False))
        return None
    _CASES.append((leg, label, rel, True))
    r32 = restate()
    print("HOT %s | %s | beyond %.1g: float32 restatement %.3g, bound %.3g" % (leg, label, C.BAR, r32, C.RESTATEMENT_FACTOR * r32))
    if rel <= C.RESTATEMENT_FACTOR * r32:
        return None
    return "%s [%s]: relative error %.3g > %.1g and > %g x the float32 restatement's %.3g; kernels %s" % (
        label, leg, rel, C.BAR, C.RESTATEMENT_FACTOR, r32, kernels)


def _restate(oracle, case):
    return lambda: C.rel_error(oracle.forward(case.cfg, case.weights, case.xb, case.x2, dtype=np.float32)[case.i], case.ref[case.i])


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


def _contract(oracle, leg, label, eng, case, flagged, split16=1, independence=True, marking="exact"):
    """Clauses 1 .. 4 for a HotCase on a loaded engine; returns the failure messages."""
    ops = eng.ops()
    kernels = [o["kernel"] for o in ops]
    expected = C.flag_expected(oracle, case.cfg, ops, case.target, split16)
    writes, reads = C.launches_around(oracle, case.cfg, ops, case.target)
    sides = "written by %s, read by %s" % ([o["kernel"] for o in writes], [o["kernel"] for o in reads])
    if marking == "exact":                      # the hand marking against the plan
        assert expected is None or flagged == expected, "%s: marked flagged = %r, but %s is %s" % (label, flagged, case.target, sides)
    n, i = case.x.shape[0], case.i
    clean = eng.forward(case.x, case.x2)
    y = eng.forward(case.xb, case.x2)
    again = eng.forward(case.x, case.x2)
    fails = []
    for j in range(n):
        if j != i and not _same(y[j], clean[j]):
            fails.append("%s [%s]: bystander %d differs from the clean batch's in %d values (max %.3g)" % (
                label, leg, j, int((y[j] != clean[j]).sum()), float(np.nanmax(np.abs(y[j].astype(np.float64) - clean[j])))))
    fails.append(_value(oracle, leg, label, y[i], case.ref[i], kernels, _restate(oracle, case)))
    if independence:
        alone = eng.forward(case.xb[i:i + 1], case.x2[i:i + 1])
        if not _same(alone[0], y[i]):
            fails.append("%s [%s]: the hot image alone differs from the one in the batch in %d values" % (label, leg, int((alone[0] != y[i]).sum())))
    if flagged:
        if not _same(again, clean):
            fails.append("%s [%s]: the clean forward behind the hot one differs from the one before it in %d values" % (label, leg, int((again != clean).sum())))
        eng.set_option("split16", 0)
        y32 = eng.forward(case.xb, case.x2)
        eng.set_option("split16", split16)
        if not _same(y[i], y32[i]):
            fails.append("%s [%s]: the hot image is not the split16 = 0 forward's, %d values differ (max %.3g of %.3g); %s is %s" % (
                label, leg, int((y[i] != y32[i]).sum()), float(np.nanmax(np.abs(y[i].astype(np.float64) - y32[i]))), float(np.max(np.abs(case.ref[i]))),
                case.target, sides))
    return [f for f in fails if f]


def _finish(fails):
    if fails:
        pytest.fail("\n".join(fails))


def _label(net, shape, target, case):
    return "%s %dx%dx%d hot %r at %s (2^%d, peak %.4g)" % (net, shape[0], shape[1], shape[2], shape[3], target, case.e, case.peak)


# ---------------------------------------------------------------------------------------------
# A. every conv of the shipped nets
# ---------------------------------------------------------------------------------------------
CASES_A = C.cases_a(dcscn_oracle, CONFIGS)
# the separable net once more on feat_stream + tail_stream: Concat2 [B2 | A1] is then read by Up-PS's depthwise stage, float32 code inside
# tail_stream like the stages behind it, so only the feature layers (operands of the A1 || B1 GEMM in feat_stream) are marked
CASES_A_TAIL = [(net, shape, t, t.startswith("CNN")) for net, shape, t, _ in CASES_A if net == "L7_F32to8_x4_DS"]


def _ids(cases):
    return ["%s-%dx%d-%s" % (c[0], c[1][1], c[1][2], c[2]) for c in cases]


@pytest.mark.parametrize("net,shape,target,flagged", CASES_A, ids=_ids(CASES_A))
def test_first_overflow_at_every_layer(oracle, request, net, shape, target, flagged):
    """Batch of three, hot image in the middle (L12 on 20 x 15: last), first overflow at ``target``."""
    _RAN.add(request.node.nodeid)
    case = C.directed_case(oracle, CONFIGS, net, shape, target)
    with _engine(case.cfg, case.weights) as eng:
        _finish(_contract(oracle, "A layers", _label(net, shape, target, case), eng, case, flagged))


@pytest.mark.parametrize("net,shape,target,flagged", CASES_A_TAIL, ids=_ids(CASES_A_TAIL))
def test_first_overflow_at_every_layer_streamed_tail(oracle, request, net, shape, target, flagged):
    """fold_whole_tail = 0: the separable net's tail on tail_stream instead of the whole-tail fold."""
    _RAN.add(request.node.nodeid)
    case = C.directed_case(oracle, CONFIGS, net, shape, target)
    with _engine(case.cfg, case.weights, (("fold_whole_tail", 0),)) as eng:
        assert "tail_stream" in [o["kernel"] for o in eng.ops()], eng.ops()
        _finish(_contract(oracle, "A layers, tail_stream", _label(net, shape, target, case) + " fold_whole_tail 0", eng, case, flagged))


# ---------------------------------------------------------------------------------------------
# B. one hot pixel: only the workgroups whose receptive field holds it can see the overflow
# ---------------------------------------------------------------------------------------------
CASES_B = C.cases_b()


def test_hot_pixel_shapes_end_in_a_strip_of_one_column():
    """exec.hip: stream_geometry for the streamed kernels' halos: feat3_stream with A1 || B1 and B2 (8), feat_stream (8), tail_stream (2)."""
    _RAN.add("shapes")
    assert _geometry(3, 17, 33, 8)[:2] == (1, 33)           # one strip: W <= 48
    assert _geometry(3, 33, 49, 8)[:2] == (2, 49 - 32) and _geometry(3, 33, 49, 8)[2:] == (2, 1)      # two strips, two row blocks, the last of one row
    assert _geometry(3, 33, 49, 2)[:2] == (2, 5)


@pytest.mark.parametrize("net,shape,target,flagged", CASES_B, ids=["%s-%s-px%d.%d" % (c[0], c[2], c[1][3][1], c[1][3][2]) for c in CASES_B])
def test_one_hot_pixel(oracle, request, net, shape, target, flagged):
    _RAN.add(request.node.nodeid)
    case = C.directed_case(oracle, CONFIGS, net, shape, target)
    with _engine(case.cfg, case.weights) as eng:
        _finish(_contract(oracle, "B pixel", _label(net, shape, target, case), eng, case, flagged))


# ---------------------------------------------------------------------------------------------
# C. the edge itself: a float32 value relayed bit for bit to the operands of CNN2 and A1 || B1
# ---------------------------------------------------------------------------------------------
RELAY_NETS = ("L8_F96to48_x2", "L7_F32to8_x2")
CASES_C = [(net, last, px) for net in RELAY_NETS for last in (False, True) for px in ((0, 0), (8, 16))]


@pytest.mark.parametrize("net,last,px", CASES_C, ids=["%s-ch%s-px%d.%d" % (c[0], "last" if c[1] else "0", c[2][0], c[2][1]) for c in CASES_C])
def test_the_edge_values_relayed_bit_for_bit(oracle, request, net, last, px):
    """Batch of 2 on 17 x 33; the hot pixel of image 1 holds +-65504, +-nextafter(65520, 0) (both split to a finite hi), +-65520,
    +-nextafter(65520, inf) (neither does: flagged).  All eight meet clauses 1 .. 3; the four beyond the edge meet clause 4."""
    _RAN.add(request.node.nodeid)
    cfg, weights = C.shipped_net(oracle, CONFIGS, net)
    channel = weights["CNN1/conv_W"].shape[3] - 1 if last else 0
    relay = C.relay_weights(cfg, weights, channel)
    x, x2 = C.bare_batch(2, 17, 33, cfg["scale"], C.BATCH_SEED)
    fails = []
    with _engine(cfg, relay) as eng:
        ops = eng.ops()
        kernels = [o["kernel"] for o in ops]
        assert C.flag_expected(oracle, cfg, ops, "CNN1"), ops         # CNN1's output is read by split16 launches
        clean = eng.forward(x, x2)
        for v, beyond in C.edge_values():
            label = "%s relay channel %d, pixel %r = %r" % (net, channel, px, float(v))
            xb = C.relay_input(x, 1, px[0], px[1], v)
            ref, t = oracle.forward(cfg, relay, xb, x2, dtype=np.float64, return_intermediates=True)
            assert t["CNN1"][1, px[0], px[1], channel] == float(v)
            y = eng.forward(xb, x2)
            again = eng.forward(x, x2)
            alone = eng.forward(xb[1:], x2[1:])
            if not _same(y[0], clean[0]):
                fails.append("%s: the bystander differs in %d values" % (label, int((y[0] != clean[0]).sum())))
            fails.append(_value(oracle, "C edge", label, y[1], ref[1], kernels,
                                lambda: C.rel_error(oracle.forward(cfg, relay, xb, x2, dtype=np.float32)[1], ref[1])))
            if not _same(alone[0], y[1]):
                fails.append("%s: the hot image alone differs in %d values" % (label, int((alone[0] != y[1]).sum())))
            if beyond:
                if not _same(again, clean):
                    fails.append("%s: the next clean forward differs in %d values" % (label, int((again != clean).sum())))
                eng.set_option("split16", 0)
                y32 = eng.forward(xb, x2)
                eng.set_option("split16", 1)
                if not _same(y[1], y32[1]):
                    fails.append("%s: not the split16 = 0 forward's bits, %d values differ" % (label, int((y[1] != y32[1]).sum())))
    _finish([f for f in fails if f])


# ---------------------------------------------------------------------------------------------
# D. pass structure: the flags are pass-local and cleared by pass_begin
# ---------------------------------------------------------------------------------------------
NETS_D = ("L8_F96to48_x2", "L7_F32to8_x4")


@pytest.mark.parametrize("hot", [0, 2, 4])
@pytest.mark.parametrize("per_pass", [1, 2])
@pytest.mark.parametrize("net", NETS_D)
def test_hot_image_in_a_sub_batched_forward(oracle, request, net, per_pass, hot):
    """Five images as passes of 1, or of 2, 2 and 1: a hot image in a later pass is recomputed (the flag index is pass-local), bystanders
    in later passes keep their bits (pass_begin clears the flags)."""
    _RAN.add(request.node.nodeid)
    shape = (5, 17, 19, hot)
    case = C.directed_case(oracle, CONFIGS, net, shape, "B1")
    with _engine(case.cfg, case.weights, (("sub_batch_pixels", per_pass * 17 * 19),)) as eng:
        _finish(_contract(oracle, "D sub-batch", _label(net, shape, "B1", case) + " %d per pass" % per_pass, eng, case, True))


@pytest.mark.parametrize("px", C.pixels_b(40, 33), ids=lambda p: "px%d.%d" % p)
@pytest.mark.parametrize("net", NETS_D)
def test_hot_pixel_in_a_tiled_forward(oracle, request, net, px):
    """workspace_budget_bytes as in test_random_configs._run_draw: 40 x 33 runs as haloed windows.  The unit that is recomputed is a
    window, so clauses 1 and 2 only; the bystander is compared with its own tiled run."""
    from dcscn_amd import engine
    _RAN.add(request.node.nodeid)
    shape = (2, 40, 33, (1,) + px)
    case = C.directed_case(oracle, CONFIGS, net, shape, "B1")
    label = _label(net, shape, "B1", case) + " tiled"
    with _engine(case.cfg, case.weights) as eng:
        kernels = [o["kernel"] for o in eng.ops()]
        eng.forward(case.x, case.x2)            # (workspace_bytes speaks of the last forward)
        per_px = eng.workspace_bytes() // (2 * 40 * 33) + 1
        eng.set_option("workspace_budget_bytes", per_px * (40 * 33 // 2))
        try:
            clean = eng.forward(case.x, case.x2)
        except engine.EngineError as exc:
            pytest.fail("%s: the windows of this budget are smaller than the halo (%s): pick another shape" % (label, exc))
        y = eng.forward(case.xb, case.x2)
    fails = [] if _same(y[0], clean[0]) else ["%s: the bystander differs from its own tiled run in %d values" % (label, int((y[0] != clean[0]).sum()))]
    fails.append(_value(oracle, "D tiled", label, y[1], case.ref[1], kernels, _restate(oracle, case)))
    _finish([f for f in fails if f])


@pytest.mark.parametrize("net", NETS_D)
def test_hot_image_in_a_replayed_graph(oracle, request, net):
    """graph_replay = 1 through forward_device on fixed buffers: clean, clean (captured), hot (replayed), clean (replayed); each equals
    the same forward with graph_replay = 0 -- the captured graph carries pass_begin and the gated float32 plan."""
    _RAN.add(request.node.nodeid)
    shape = C.SHAPE_A
    case = C.directed_case(oracle, CONFIGS, net, shape, "B1")
    n, h, w = shape[:3]
    hip = P._Hip()
    try:
        with _engine(case.cfg, case.weights) as eng:
            kernels = [o["kernel"] for o in eng.ops()]
            assert C.flag_expected(oracle, case.cfg, eng.ops(), "B1")
            clean, hot = eng.forward(case.x, case.x2), eng.forward(case.xb, case.x2)
            dx, dx2, dy = hip.upload(case.x), hip.upload(case.x2), hip.alloc(clean.nbytes)
            st = hip.stream()
            eng.set_option("graph_replay", 1)
            got = []
            for x in (case.x, case.x, case.xb, case.x):
                hip.write(dx, x)
                eng.forward_device(dx, dx2, dy, n, h, w, stream=st)
                eng.synchronize()
                got.append(hip.download(dy, clean.shape))
            eng.set_option("graph_replay", 0)
    finally:
        hip.close()
    fails = ["%s: call %d through the graph differs from plain launches in %d values" % (net, k, int((g != e).sum()))
             for k, (g, e) in enumerate(zip(got, (clean, clean, hot, clean))) if not _same(g, e)]
    fails.append(_value(oracle, "D graph", _label(net, shape, "B1", case) + " replayed", got[2][1], case.ref[1], kernels, _restate(oracle, case)))
    _finish([f for f in fails if f])


@pytest.mark.parametrize("n_ensemble", [5, 8])
@pytest.mark.parametrize("net", NETS_D)
def test_hot_image_in_the_self_ensemble(oracle, request, net, n_ensemble):
    """13 x 18, every flip beyond the range at B1 -- the four plain flips as one batch, the transposed ones as another: the float64 mean
    against oracle.do at the bar of clause 2, and bit for bit the split16 = 0 ensemble."""
    _RAN.add(request.node.nodeid)
    cfg, weights = C.shipped_net(oracle, CONFIGS, net)
    x, _ = C.bare_batch(1, 13, 18, cfg["scale"], C.BATCH_SEED)
    case = C.EnsembleCase(oracle, cfg, weights, x[0], "B1", n_ensemble)
    with _engine(cfg, case.weights) as eng:
        kernels = [o["kernel"] for o in eng.ops()]
        assert C.flag_expected(oracle, cfg, eng.ops(), "B1")
        y = eng.forward_ensemble(case.xb, case.x2, n_ensemble)
        eng.set_option("split16", 0)
        y32 = eng.forward_ensemble(case.xb, case.x2, n_ensemble)
    label = "%s ensemble of %d on 13x18 at B1 (2^%d)" % (net, n_ensemble, case.e)
    fails = [] if _same(y, y32) else ["%s: not the split16 = 0 ensemble's bits, %d values differ" % (label, int((y != y32).sum()))]

    def restate():
        return C.rel_error(oracle.do(cfg, case.weights, case.xb, case.x2, self_ensemble=n_ensemble, dtype=np.float32), case.ref)
    fails.append(_value(oracle, "D ensemble", label, y, case.ref, kernels, restate))
    _finish([f for f in fails if f])


# ---------------------------------------------------------------------------------------------
# E. the engine options: another plan, the same contract
# ---------------------------------------------------------------------------------------------
OPTIONS_E = [("split16", 2), ("split16", 3), ("p16", 0), ("nin_h8", 0), ("stream_dense", 0), ("stream_nin", 0), ("fold_linear_tail", 0), ("winograd", 0)]
NETS_E = {"L8_F96to48_x2": ("CNN4", "B2"), "L7_F32to8_x2": ("CNN4", "B2")}
# split16 = 3 keeps only the 1x1 GEMMs on the f16 pipe (api.hip: mask bit 1; exec.hip: op_on_split16): B2 is then written and read by float32
# 3x3 launches.  The narrow net's streamed launch then runs layer by layer with A1 || B1 on conv_nin_h, which reads CNN4: flagged, though
# dcscn_op_info does not name the kernels of a "layer by layer" launch (flag_expected: None)
NOT_FLAGGED_E = {("L8_F96to48_x2", ("split16", 3), "B2"), ("L7_F32to8_x2", ("split16", 3), "B2")}
CASES_E = [(net, opt, t) for net, targets in NETS_E.items() for opt in OPTIONS_E for t in targets]
CASES_E += [("L12_F196to48_x2", opt, t) for opt in (("conv3_h8", 0), ("nin_h8", 0)) for t in ("CNN4", "B2")]


@pytest.mark.parametrize("net,option,target", CASES_E, ids=["%s-%s%d-%s" % (c[0], c[1][0], c[1][1], c[2]) for c in CASES_E])
def test_first_overflow_under_an_option(oracle, request, net, option, target):
    _RAN.add(request.node.nodeid)
    case = C.directed_case(oracle, CONFIGS, net, C.SHAPE_A, target)
    split16 = option[1] if option[0] == "split16" else 1
    with _engine(case.cfg, case.weights, (option,)) as eng:
        _finish(_contract(oracle, "E options", _label(net, C.SHAPE_A, target, case) + " %s = %d" % option, eng, case,
                          (net, option, target) not in NOT_FLAGGED_E, split16=split16))


# ---------------------------------------------------------------------------------------------
# F. the walk
# ---------------------------------------------------------------------------------------------
WALK = [s for s in range(200) if s not in C.WALK_LEFT_OUT]


@pytest.mark.parametrize("seed", WALK)
def test_random_flag_surface_first_overflow(oracle, request, seed):
    """Draw ``seed`` of test_random_configs with its own winograd and fold: its first image and the 8-fold copy, target
    convs[seed % len(convs)].  Clauses 1 .. 3; clause 4 where a split16 launch reads the target (overflow_cases.flag_expected)."""
    _RAN.add(request.node.nodeid)
    flags, opts, case = C.walk_case(oracle, seed)
    label = "walk draw %d: %r %dx%d %r at %s (2^%d)" % (seed, flags, case.x.shape[1], case.x.shape[2], opts, case.target, case.e)
    with _engine(case.cfg, case.weights, load=dict(winograd=opts["winograd"], fold_tail=opts["fold"])) as eng:
        flagged = C.flag_expected(oracle, case.cfg, eng.ops(), case.target) is True
        _finish(_contract(oracle, "F walk, flagged" if flagged else "F walk", label, eng, case, flagged, marking="plan"))


N_TESTS = len(CASES_A) + len(CASES_A_TAIL) + 1 + len(CASES_B) + len(CASES_C) + len(NETS_D) * (6 + 3 + 1 + 2) + len(CASES_E) + len(WALK)


def _whole_file_ran():
    if len(_RAN) != N_TESTS:
        pytest.skip("%d of this file's %d tests ran before this one: it speaks about the whole file" % (len(_RAN), N_TESTS))


def test_every_split16_kernel_was_reached_by_a_hot_case():
    """Every name of exec.hip: kernel_name that runs a split16 kernel is in the launch list of at least one hot case."""
    _whole_file_ran()
    print("REACH hot cases per kernel (of %d)" % len(_CASES))
    for k in KERNEL_NAMES:
        print("REACH %-16s %d" % (k, _REACH[k]))
    assert set(SPLIT16_NAMES) <= set(KERNEL_NAMES)
    assert not [k for k in SPLIT16_NAMES if _REACH[k] == 0], _REACH


def test_the_float32_restatement_clause_is_the_exception_for_hot_cases():
    """At most 2 % of the file's cases were beyond 5e-6 and had to be judged by their float32 restatement."""
    _whole_file_ran()
    legs = {}
    for leg, label, rel, clause in _CASES:
        if leg not in legs or rel > legs[leg][0]:
            legs[leg] = (rel, label, 0)
    for leg in sorted(legs):
        print("WORST %s (%d cases): %.3g on %s" % (leg, sum(1 for c in _CASES if c[0] == leg), legs[leg][0], legs[leg][1]))
    used = [(leg, label, rel) for leg, label, rel, clause in _CASES if clause]
    print("CLAUSE %d of %d cases used the float32-restatement clause" % (len(used), len(_CASES)))
    for leg, label, rel in used:
        print("CLAUSE   %s | %s | %.3g" % (leg, label, rel))
    assert len(used) <= 0.02 * len(_CASES), used
