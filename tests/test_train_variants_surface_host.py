"""The cases of tests/test_train_variants_surface_hip.py checked on the CPU (tests/train_variant_cases.py): what the 200 draws of its walk
cover, the margin that torch float32 autograd of the same graph leaves under the GPU file's bar on every case, the draws that are left out
for want of that margin, and the split counts the directed shapes were chosen for."""
import collections

import numpy as np
import pytest

import train_ref_transposed as T
import train_variant_cases as V


def test_the_walk_covers_the_three_kinds_and_the_shapes_the_kernels_branch_on(oracle):
    """Read from the generator's output alone.  Of the kept draws: every kind at least 40 times, every activator on every kind, scales
    2, 3 and 4 on both transposed kinds, a depthwise layer with cin > 64 (tdw_wgrad: blockIdx.y > 0) and with cin > 128, an Up-TCNN with
    C > 64 (three column tiles) and one with C <= 4 (one ragged k-step)."""
    assert len(V.WALK_EXCLUDED) <= 4 and all(0 <= s < V.WALK_DRAWS for s in V.WALK_EXCLUDED)
    assert len(V.WALK_KEPT) == V.WALK_DRAWS - len(V.WALK_EXCLUDED)
    kinds = collections.Counter()
    activators, scales = collections.defaultdict(set), collections.defaultdict(set)
    dw_cin, tc, ks, psf, rl, l1_dropout = set(), set(), set(), set(), set(), 0
    for seed in V.WALK_KEPT:
        kind, flags, n, h, w, l1, keep = V.walk_draw(seed)
        cfg = oracle.make_config(**flags)                          # every config builds
        assert cfg["pixel_shuffler"] == (kind == 0) and cfg["depthwise_separable"] == (kind != 1)
        assert 1 <= n <= 4 and 1 <= h <= 24 and 1 <= w <= 24
        kinds[kind] += 1
        activators[kind].add(flags["activator"])
        scales[kind].add(flags["scale"])
        cins = V.depthwise_cins(cfg)
        assert bool(cins) == (kind != 1) and (V.tconv_channels(cfg) is not None) == (kind != 0)
        dw_cin.update(cins)
        if kind != 0:
            tc.add(V.tconv_channels(cfg))
        if kind != 1:
            ks.add((flags["cnn_size"], flags["cnn_size"] > min(h, w)))
        if kind == 0:
            psf.add(flags["pixel_shuffler_filters"])
        rl.add((kind, flags["reconstruct_layers"]))
        l1_dropout += l1 and keep < 1.0
    print("kinds %r; depthwise cin up to %d; Up-TCNN C %r" % (dict(kinds), max(dw_cin), sorted(tc)))
    assert all(kinds[k] >= 40 for k in (0, 1, 2)), kinds
    for kind in (0, 1, 2):
        assert activators[kind] == {"prelu", "relu", "leaky_relu", "sigmoid", "tanh", "selu"}, (kind, activators[kind])
    assert scales[1] == {2, 3, 4} and scales[2] == {2, 3, 4}, scales
    assert max(dw_cin) > 128 and any(64 < c <= 128 for c in dw_cin), sorted(dw_cin)
    assert max(tc) > 64 and min(tc) <= 4, sorted(tc)
    # what the issue lists as never run before: depthwise 1x1 and 7x7 (one of them wider than its image), pixel_shuffler_filters other than
    # 1 on a separable Up-PS, three reconstruction layers on every kind, L1 with dropout
    assert {k for k, _ in ks} >= {1, 3, 5, 7} and (7, True) in ks, ks
    assert psf >= {0, 5, 16}, psf
    assert {(kind, 3) for kind in (0, 1, 2)} <= rl, rl
    assert l1_dropout >= 5


@pytest.mark.parametrize("seed", range(V.WALK_DRAWS))
def test_float32_carries_every_kept_draw_and_no_excluded_one(seed):
    """torch float32 autograd of draw ``seed`` against float64, on every tensor whose float64 gradient is not identically zero: within
    2.5e-5 * max|g64| (a quarter of the GPU file's bar) for a draw the GPU file runs, above it for a draw in WALK_EXCLUDED, so that the
    list cannot grow quietly.  Measured over draws 0..199: 198 are within 1.05e-5 (worst draw 87, CNN2/prelu/CNN2_prelu, then draw 198,
    CNN5/prelu/CNN5_prelu); draw 151 is 2.5e-4 off on Up-TCNN/Tconv_W and draw 185 7.0e-5 on Up-PS/Up-PS_CNN/depthwise_W.  Draws 3 and 76
    have tensors whose gradient is identically zero (dead relu layers with k = 1)."""
    ratios, zeros = V.walk_float32(seed)
    worst, name = V.worst_nonzero(ratios, zeros)
    print("F32 draw %d: %.3g (%s); identically zero %r; %s" % (seed, worst, name, zeros, V.walk_context(seed)))
    assert all(ratios[k] == 0.0 for k in zeros), (zeros, ratios)   # float32 gives exact zeros there too
    if seed in V.WALK_EXCLUDED:
        assert worst > V.F32_BAR, (seed, worst, name)
        assert 0.5 * V.WALK_EXCLUDED[seed] <= worst <= 2.0 * V.WALK_EXCLUDED[seed], (seed, worst, V.WALK_EXCLUDED[seed])   # the figure beside it
    else:
        assert worst <= V.F32_BAR, (seed, worst, name)


def test_the_walk_has_draws_with_gradients_that_are_identically_zero():
    """Draws 3 and 76 are kept: they exercise the exact-zero assertion of the GPU file."""
    for seed in (3, 76):
        assert seed in V.WALK_KEPT and V.walk_float32(seed)[1], seed


@pytest.mark.parametrize("case", list(V.SPLIT_CASES), ids=V.case_id)
def test_the_split_cases_have_several_up_tcnn_splits_and_a_ragged_last_one(case):
    """wgrad_splits restated (tests/train_ref_separable.py): why these shapes were chosen, not a reference for the kernel.  Every
    transposed case of tests/train_ref_transposed.py has one split."""
    k, c, pixels, splits, chunk, last = V.up_tcnn_splits(case)
    assert (k, c, pixels, splits, chunk, last) == V.SPLIT_CASES[case]
    assert splits >= 2 and 0 < last < chunk and chunk % 16 == 0
    name, n, h, w = case[:4]
    if name == "t3":
        assert chunk % (h * w) != 0 and h * w < chunk < 2 * h * w  # the boundary between the splits lies inside image 1
    if name == "t4":
        assert (c + 31) // 32 == 3
    if name == "t2":
        assert splits == 5
    for other in T.MAIN_CASES + T.EDGE_CASES:
        assert V.up_tcnn_splits(other)[3] == 1, other


def test_wgrad_splits_restates_the_separable_rule_too():
    """A separable layer's pointwise filter takes half the pixels per split and at most 256 splits (train.hip: wgrad_splits)."""
    assert V.wgrad_splits(1, 32, 32, 1311, ds=True) == (3, 448)
    assert V.wgrad_splits(1, 32, 32, 1311) == (2, 656)
    assert V.wgrad_splits(1, 8, 8, 10 ** 6, ds=True)[0] <= 256
    assert V.wgrad_splits(3, 64, 64, 5) == (1, 16)


def _assert_float32_margin(label, ratios, zeros):
    worst, name = V.worst_nonzero(ratios, zeros)
    print("F32 %s: %.3g (%s)" % (label, worst, name))
    assert not zeros, zeros                                         # no gradient of a directed case vanishes
    assert worst <= V.F32_BAR, (label, worst, name)


@pytest.mark.parametrize("case", list(V.SPLIT_CASES) + V.SHARD_CASES, ids=V.case_id)
def test_float32_is_well_inside_the_gpu_bar_on_the_directed_cases(case):
    """Measured: within 2.4e-6 on the split cases (worst tds, B2/prelu/B2_prelu), within 1.7e-6 on the shard cases."""
    _assert_float32_margin(V.case_id(case), *V.case_float32(case))


@pytest.mark.parametrize("name", V.MOVED_NETS)
def test_float32_is_well_inside_the_gpu_bar_at_the_weights_set_train_tensor_installs(name):
    """The second comparison of the moved-weights test: synthetic_weights(seed 5), 2x18x22, keep 0.8, key 78, l2_decay 1e-3.  (The
    weights after 5 Adam steps exist only on the device; the GPU test prints float32's ratio there.)"""
    cfg, weights, x, x2, y = V.moved_inputs(name)
    _assert_float32_margin("moved " + name, *V.float32_ratios(cfg, weights, x, x2, y, keep=V.MOVED_KEEP, key=78, l1=False, l2_decay=V.L2_DECAY))


def test_dropping_the_decay_of_tconv_w_misses_the_bar_on_the_shard_cases():
    """The l2 term is counted once over the shards, Tconv_W in it: without it the gradient of Tconv_W moves by l2_decay * max|Tconv_W|,
    which the bar of the shard test sees on every case."""
    for case in V.SHARD_CASES:
        cfg, weights, x, x2, y = V.case_inputs(case)
        _, g = V.reference(case)
        name = "Up-TCNN/Tconv_W"
        moved, bar = T.L2_DECAY * float(np.max(np.abs(weights[name]))), V.BAR * float(np.max(np.abs(g[name])))
        print("%s: the decay is %.3g of Tconv_W's gradient, the bar %.3g: %.1f x" % (V.case_id(case), moved, bar, moved / bar))
        assert moved > 2.0 * bar, case
