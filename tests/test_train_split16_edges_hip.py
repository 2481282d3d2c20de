"""Option "train_split16" at the edges of its scaling and tiling (csrc/train_h.hip): the cases come from the kernels' own branch points,
not from the f32 path's test surface.

The reference is the float64 restatement of tests/train_ref.py; a second run of the library is the reference only where bit-identity
is the stated property.  The bar is the f32 path's: every gradient tensor within C.TOL = 1e-4 of max|g64| and the other assertions of
test_train_surface_hip._compare.  Wherever an input is unusual the option-off handle is held to the same bar on the same input
first, so that a failure points at split16 and not at the input.  ``RATIO`` lines (pytest -s) print the device's and float32 torch's
worst max|g - g64| / max|g64| side by side.
1 magnitudes by exact rebalancing, 2 zero, tiny and non-finite tensors, 3 where the maximum sits, 4 past the reduction's block clamp and
the aligned load classes, 5 the shard and patch routes.  tests/test_train_split16_edges_host.py shows that the cases reach every branch
class."""
import numpy as np
import pytest
import torch

import dcscn_oracle as O
import train_ref as R
import train_split16_cases as C
import test_train_parallel_hip as P
from test_train_surface_hip import _compare, _ratios, _worst

pytestmark = pytest.mark.gpu

KEEP = C.EDGE_KEEP


def _device(cfg, weights, x, x2, y, on, **flags):
    """(stats, gradients) of a fresh handle with the option off / on; keep 0.8 and _compare's l2_decay unless ``flags`` say otherwise."""
    with C.engine_for(cfg, weights, on, **dict(dict(dropout_rate=KEEP, l2_decay=C.L2_DECAY), **flags)) as eng:
        return C.grads_and_stats(eng, weights, x, x2, y)


def _both(label, cfg, weights, x, x2, y):
    """The full _compare of the option-off handle, then of the option-on handle, on the same input; the two differ in bits."""
    out = {}
    for on in (False, True):
        out[on] = _device(cfg, weights, x, x2, y, on)
        _compare("%s, option %s" % (label, "on" if on else "off"), cfg, weights, x, x2, y, *out[on], keep=KEEP, key=C.KEY, tol=C.TOL)
    assert not C.same_bits(C.bits(*out[False]), C.bits(*out[True])), "the option changed no bit"
    return out


def _bar(label, cfg, weights, x, x2, y, stats, got, l2_decay, floor=0.0):
    """_compare's assertions with an l2_decay of the caller's: gradients within C.TOL * max|g64|, exact zeros where the float64 gradient is
    identically zero, image loss / mse / total loss to 1e-6 relative, the global norm to 1e-4 relative, everything finite.  A tensor
    whose max|g64| is below ``floor`` is only asked to be finite; returns the names of those."""
    ref, g64 = R.loss_and_grads(cfg, weights, x, x2, y, keep=KEEP, key=C.KEY, l2_decay=l2_decay)
    _, g32 = R.loss_and_grads(cfg, {k: v.astype(np.float32) for k, v in weights.items()}, x, x2, y, keep=KEEP, key=C.KEY, l2_decay=l2_decay,
                              dtype=torch.float32)
    _, norm = R.clip_factor(g64, 0.0)
    below = sorted(k for k, g in g64.items() if float(np.max(np.abs(g))) < floor)
    held = {k: g for k, g in g64.items() if k not in below}
    dev, f32 = _ratios(got, held), _ratios(g32, held)
    (dr, dn), (fr, fn) = _worst(dev), _worst(f32)
    print("RATIO %s: device %.3g (%s), float32 torch %.3g (%s); float32 torch at the device's tensor %.3g" % (label, dr, dn, fr, fn, f32[dn]))
    print("STATS %s: device %r; reference %r norm %.17g" % (label, tuple(stats), ref, norm))
    bad = ["%s: not finite" % k for k in g64 if not np.isfinite(got[k]).all()]
    for k, g in held.items():
        if not np.any(g):
            if np.any(got[k]):
                bad.append("%s: the float64 gradient is identically zero, the device's max is %.3g" % (k, float(np.max(np.abs(got[k])))))
        elif not dev[k] <= C.TOL:
            bad.append("%s: max err %.3g of max|g64| (bound %.3g); float32 torch %.3g" % (k, dev[k], C.TOL, f32[k]))
    if not np.isfinite(np.asarray(stats)).all():
        bad.append("stats not finite: %r" % (stats,))
    for i, k in ((0, "image_loss"), (1, "mse"), (3, "loss")):
        if not abs(stats[i] - ref[k]) <= 1e-6 * abs(ref[k]):
            bad.append("stats[%d] %.17g, reference %s %.17g" % (i, stats[i], k, ref[k]))
    if not abs(stats[2] - norm) <= 1e-4 * norm:
        bad.append("stats[2] %.17g, float64 global norm %.17g" % (stats[2], norm))
    assert not bad, "%s\n%s" % (label, "\n".join(bad))
    return below


# ---------------------------------------------------------------------------------------------
# 1. magnitudes: an exact symmetry of the net moves three tensors' exponents by k and nothing else
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on", [False, True], ids=["off", "on"])
def test_rebalancing_b1_against_b2_changes_no_bit(on):
    """Gradients of B1's filter and bias scale by 2^-k, of B2's filter by 2^k, everything else and the loss stats keep their bits: the
    scales are powers of two and ldexpf is exact, so the option's result does not depend on a tensor's magnitude.  No l2 term (it does
    not share the symmetry) and no clipping."""
    cfg, weights, x, x2, y = C.edge_inputs("odd-2x7x9")
    flags = dict(l2_decay=0.0, clipping_norm=0.0)
    stats0, got0 = _device(cfg, weights, x, x2, y, on, **flags)
    _bar("edges 1 rebalancing k 0, option %d" % on, cfg, weights, x, x2, y, stats0, got0, 0.0)
    base = C.bits(stats0, got0)
    for k in C.REBALANCE:
        moved = C.rebalanced(weights, k)
        stats, got = _device(cfg, moved, x, x2, y, on, **flags)
        _bar("edges 1 rebalancing k %d, option %d" % (k, on), cfg, moved, x, x2, y, stats, got, 0.0)
        back = C.bits(stats, C.undo_rebalancing(got, k))
        differ = [n for n in got if not np.array_equal(back[n], base[n])]
        assert not differ, "k = %d: not the bits of k = 0 in %s" % (k, differ)
        assert (stats[0], stats[1], stats[3]) == (stats0[0], stats0[1], stats0[3]), (k, stats, stats0)


# ---------------------------------------------------------------------------------------------
# 2. zero, tiny and non-finite tensors
# ---------------------------------------------------------------------------------------------
def test_a_zero_filter_and_a_zero_input_slice():
    """B1's filter and bias zero: e_w = 0 for B1 and an all-zero input slice (e_in = 0) for B2."""
    cfg, weights, x, x2, y = C.edge_inputs("odd-2x7x9")
    zero = dict(weights)
    zero["B1/conv_W"], zero["B1/conv_B"] = np.zeros_like(weights["B1/conv_W"]), np.zeros_like(weights["B1/conv_B"])
    taps = {"B1": None}
    R.loss_and_grads(cfg, zero, x, x2, y, keep=KEEP, key=C.KEY, taps=taps)
    assert not np.any(taps["B1"]["out"]) and np.any(taps["B1"]["dz"])
    _both("edges 2a zero B1", cfg, zero, x, x2, y)


def test_a_zero_dz():
    """The Up-PS filter's input channels 17.. (A1's half of Concat2 = [B2 | A1]) zero: A1's dz is all zero (e = 0), its bias and
    slope gradients are identically zero and its filter's is the l2 term alone."""
    cfg, weights, x, x2, y = C.edge_inputs("odd-2x7x9")
    cut = dict(weights)
    cut["Up-PS/Up-PS_CNN/conv_W"] = weights["Up-PS/Up-PS_CNN/conv_W"].copy()
    cut["Up-PS/Up-PS_CNN/conv_W"][:, :, cfg["nin_filters2"]:, :] = 0.0
    taps = {"A1": None, "B2": None}
    _, g64 = R.loss_and_grads(cfg, cut, x, x2, y, keep=KEEP, key=C.KEY, taps=taps)
    assert not np.any(taps["A1"]["dz"]) and np.any(taps["B2"]["dz"])
    assert not any(np.any(g64[k]) for k in g64 if k.startswith("A1/"))
    out = _both("edges 2b zero dz of A1", cfg, cut, x, x2, y)
    for on in (False, True):
        assert not np.any(out[on][1]["A1/conv_B"]) and not np.any(out[on][1]["A1/prelu/A1_prelu"])


def test_a_subnormal_maximum_reaches_the_exponent_clamp():
    """Every element of B1's filter and bias +-2^-130 (subnormal): e_w is clamped to 126 and e_in + e_w = 130; B2's input is about
    2^-120 and its e_in is clamped as well.  Tensors whose max|g64| is below 1e-30 are only asked to be finite, and those are B1's or
    B2's own."""
    cfg, weights, x, x2, y = C.edge_inputs("odd-2x7x9")
    tiny = dict(weights)
    for k in ("B1/conv_W", "B1/conv_B"):
        tiny[k] = np.copysign(np.float32(2.0 ** -130), weights[k]).astype(np.float32)
        assert np.all(np.abs(tiny[k]) == np.float32(2.0 ** -130)) and tiny[k].dtype == np.float32
    taps = {"B1": None}
    R.loss_and_grads(cfg, tiny, x, x2, y, keep=KEEP, key=C.KEY, taps=taps)
    assert C.split16_exponent(np.max(np.abs(tiny["B1/conv_W"]))) == 126 and C.split16_exponent(np.max(np.abs(taps["B1"]["out"]))) == 126
    for on in (False, True):
        stats, got = _device(cfg, tiny, x, x2, y, on)
        below = _bar("edges 2c subnormal B1, option %d" % on, cfg, tiny, x, x2, y, stats, got, C.L2_DECAY, floor=1e-30)
        assert all(k.startswith(("B1/", "B2/")) for k in below), below


def test_a_non_finite_input_leaves_nothing_behind():
    """One inf in x: the call returns in both modes with a loss that is not finite, and the next call on the same handle with the finite
    batch gives the bits of a fresh handle (nothing stale in the exponents or the partial maxima)."""
    cfg, weights, x, x2, y = C.edge_inputs("odd-2x7x9")
    bad = x.copy()
    bad[1, 3, 4, 0] = np.inf
    for on in (False, True):
        fresh = C.bits(*_device(cfg, weights, x, x2, y, on))
        with C.engine_for(cfg, weights, on, dropout_rate=KEEP, l2_decay=C.L2_DECAY) as eng:
            stats, _ = C.grads_and_stats(eng, weights, bad, x2, y)
            assert not np.isfinite(stats[0]), (on, stats)
            assert C.same_bits(C.bits(*C.grads_and_stats(eng, weights, x, x2, y)), fresh), "option %d: not the bits of a fresh handle" % on


# ---------------------------------------------------------------------------------------------
# 3. where the maximum sits: a missed maximum overflows f16
# ---------------------------------------------------------------------------------------------
FILTERS = {"CNN2": 9 * 40 * 26, "B2": 9 * 17 * 17}      # 5 blocks and 2 blocks of the reduction


@pytest.mark.parametrize("position", ["first", "last", "chunk-end", "chunk-start"])
@pytest.mark.parametrize("layer", sorted(FILTERS))
def test_the_largest_weight_at_the_ends_and_at_a_chunk_boundary(layer, position):
    cfg, weights, x, x2, y = C.edge_inputs("odd-2x7x9")
    count = weights[layer + "/conv_W"].size
    assert count == FILTERS[layer] and C.texp_partition(count)[0] == {"CNN2": 5, "B2": 2}[layer]
    index = C.filter_positions(count)[position]
    moved = C.filter_outlier(weights, layer, index)
    w = np.abs(moved[layer + "/conv_W"]).reshape(-1)
    assert int(np.argmax(w)) == index and w[index] >= 64.0 * np.max(np.delete(w, index))
    _both("edges 3 %s largest weight at %s (%d)" % (layer, position, index), cfg, moved, x, x2, y)


@pytest.mark.parametrize("where", ["x-first", "x-last", "y-first", "y-last"])
def test_an_outlier_pixel_in_the_first_and_in_the_last_chunk(where):
    """One row of 150 pixels, so that the 3x3 layers spread the outlier over three pixels on each side at the most: the largest magnitude
    of A1's input slice (x) or of A1's dz (y_true) lies in the first, respectively the last, block of the reduction."""
    cfg, weights, x, x2, y = C.edge_inputs("odd-1x1x150")
    x, x2, y = C.pixel_outlier(x, x2, y, where)
    (in_block, in_blocks), (dz_block, dz_blocks) = C.blocks_of_the_maxima(cfg, weights, x, x2, y, KEEP, C.KEY)
    block, blocks = (in_block, in_blocks) if where[0] == "x" else (dz_block, dz_blocks)
    assert blocks > 1 and block == (0 if where.endswith("first") else blocks - 1), (where, block, blocks)
    _both("edges 3 outlier %s" % where, cfg, weights, x, x2, y)


# ---------------------------------------------------------------------------------------------
# 4. past the reduction's block clamp, and the aligned load classes
# ---------------------------------------------------------------------------------------------
def test_the_aligned_net_on_exactly_one_pixel_block():
    cfg, weights, x, x2, y = C.edge_inputs("aligned-2x8x8")
    assert O.filter_schedule(cfg["layers"], cfg["filters"], cfg["min_filters"], cfg["filters_decay_gamma"]) == [48, 32, 24]
    _both("edges 4a aligned 2x8x8", cfg, weights, x, x2, y)


def _concat_count(cfg, x):
    return x.size * sum(O.filter_schedule(cfg["layers"], cfg["filters"], cfg["min_filters"], cfg["filters_decay_gamma"]))


def test_a_tensor_past_the_block_clamp_of_the_reduction():
    """5112 pixels x 104 channels: 256 blocks whose chunk is a multiple of neither 256 nor the row width, so the division-free
    (row, column) walk of tabsmax_part wraps at every step."""
    cfg, weights, x, x2, y = C.edge_inputs("aligned-1x72x71")
    count = _concat_count(cfg, x)
    blocks, chunk = C.texp_partition(count)
    assert count > C.ABS_MAX_BLOCKS * C.ABS_MAX_CHUNK and blocks == C.ABS_MAX_BLOCKS and chunk % 256 and chunk % (count // x.size)
    stats, got = _device(cfg, weights, x, x2, y, True)
    _compare("edges 4b aligned 1x72x71, option on", cfg, weights, x, x2, y, stats, got, keep=KEEP, key=C.KEY, tol=C.TOL)


def test_the_maximum_in_the_last_chunk_past_the_block_clamp():
    cfg, weights, x, x2, y = C.edge_inputs("aligned-1x1x5112")
    assert _concat_count(cfg, x) > C.ABS_MAX_BLOCKS * C.ABS_MAX_CHUNK
    x, x2, y = C.pixel_outlier(x, x2, y, "x-last")
    (block, blocks), _ = C.blocks_of_the_maxima(cfg, weights, x, x2, y, KEEP, C.KEY)
    assert (block, blocks) == (C.ABS_MAX_BLOCKS - 1, C.ABS_MAX_BLOCKS)
    _both("edges 4c aligned 1x1x5112 outlier x-last", cfg, weights, x, x2, y)


# ---------------------------------------------------------------------------------------------
# 5. routes: records of shards, and the patch route
# ---------------------------------------------------------------------------------------------
class _Rig(P.PatchRig):
    """test_train_parallel_hip's rig of handles on device 0 for a net of this module, the option set before train_begin."""

    def __init__(self, cfg, weights, splits, on, **flags):
        self.engines = [C.engine_for(cfg, weights, on, **flags) for _ in splits]
        self.bounds = np.concatenate([[0], np.cumsum(splits)])
        self.stream = torch.cuda.Stream()
        self.records = torch.zeros((len(splits), self.engines[0].train_record_floats()), dtype=torch.float32, device="cuda")
        self.ids = [{} for _ in splits]
        torch.cuda.synchronize()


def test_two_uneven_shards_give_the_gradient_of_the_whole_batch_and_the_same_bits_twice():
    cfg, weights, x, x2, y = C.edge_inputs("odd-3x7x9")
    dev = P._device((x, x2, y))
    runs = []
    for _ in range(2):
        with _Rig(cfg, weights, (2, 1), True, dropout_rate=KEEP, l2_decay=C.L2_DECAY) as rig:
            rig.local(dev, C.KEY)
            stats = rig.apply(1e-3, which=[0])[0]
            got = {k: rig.engines[0].get_tensor(k + "/grad") for k in weights}
            runs.append(dict(C.bits(stats, got), records=rig.records.cpu().numpy().view(np.uint32)))
    _compare("edges 5 shards 2 + 1 of odd 3x7x9, option on", cfg, weights, x, x2, y, stats, got, keep=KEEP, key=C.KEY, tol=C.TOL)
    assert C.same_bits(runs[0], runs[1])


def test_the_patch_route_writes_the_record_of_the_array_route_with_the_option_on():
    cfg, weights, x, _, _ = C.edge_inputs("odd-5x8x8")
    d, patches, want = P._set14_draw(cfg["scale"], 5, 255.0)
    assert want[0].shape == x.shape and P.LR_SIZE == x.shape[1]
    dev = P._device(want)
    splits = (3, 2)
    with _Rig(cfg, weights, splits, True, dropout_rate=KEEP) as by_patch, _Rig(cfg, weights, splits, True, dropout_rate=KEEP) as by_array, \
            _Rig(cfg, weights, splits, False, dropout_rate=KEEP) as off:
        by_patch.local_patches(d, patches, C.KEY)
        by_array.local(dev, C.KEY)
        off.local(dev, C.KEY)
        torch.cuda.synchronize()
        a, b, c = (r.records.cpu().numpy().view(np.uint32) for r in (by_patch, by_array, off))
    assert np.any(a[:, :1000]) and a.shape == b.shape
    for r in range(len(splits)):
        bad = np.flatnonzero(a[r] != b[r])
        assert bad.size == 0, "rank %d: %d of %d record floats differ, first at %d" % (r, bad.size, a.shape[1], bad[0])
        assert not np.array_equal(b[r], c[r]), "rank %d: the option changed no bit of the record" % r
