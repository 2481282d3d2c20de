"""Option "train_split16_wgrad" (include/dcscn.h) on the device: the weight gradient of every layer with min(cin, cout) >= 16 on the f16
matrix pipe as three scaled f16 products over chunks of 32 pixels (csrc/train_wgrad_h.hip), everything else untouched, for either
setting of "train_split16".

The reference is the float64 restatement of tests/train_ref.py; a second run of the library is the reference only where bit-identity
is the stated property.  The bar is the f32 path's: every gradient tensor within C.TOL = 1e-4 of max|g64| and the other assertions of
test_train_surface_hip._compare (tests/train_split16_wgrad_cases.py says why the mode gets no wider one).  ``RATIO`` lines (pytest -s)
print the device's and float32 torch's worst max|g - g64| / max|g64| side by side.
1 parity per case, 2 only the eligible layers' filter gradients move, 3 splits and borders, 4 scaling edges, 5 determinism and state,
6 the entry points."""
import functools

import numpy as np
import pytest
import torch

import train_ref as R
import train_split16_cases as C
import train_split16_wgrad_cases as G
import test_train_parallel_hip as P
from test_train_hip import _assert_same_bits, _batch, _state
from test_train_split16_edges_hip import _bar
from test_train_surface_hip import _compare

pytestmark = pytest.mark.gpu

BOTH = [False, True]
IDS = ["split16-off", "split16-on"]


def _grads(cfg, weights, x, x2, y, split16, wgrad, key=C.KEY, **flags):
    with G.engine_for(cfg, weights, split16, wgrad, **flags) as eng:
        return C.grads_and_stats(eng, weights, x, x2, y, key=key)


@functools.lru_cache(maxsize=None)
def _case(name, split16, wgrad):
    """(stats, gradients) of a case of C.CASES on a fresh handle; shared, not to be written to."""
    cfg, weights, x, x2, y = C.inputs(name)
    return _grads(cfg, weights, x, x2, y, split16, wgrad, **C.train_flags(name))


def _odd(oracle, **over):
    cfg = oracle.make_config(**dict(C.ODD, **over))
    return cfg, oracle.synthetic_weights(cfg, seed=0)


# ---------------------------------------------------------------------------------------------
# 1. gradient parity with the option on
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split16", BOTH, ids=IDS)
@pytest.mark.parametrize("name", sorted(C.CASES))
def test_gradients_match_float64_autograd_with_the_option_on(name, split16):
    cfg, weights, x, x2, y = C.inputs(name)
    _, _, _, keep, l1 = C.CASES[name]
    assert C.eligible_layers(cfg), "the case has no eligible layer"
    stats, got = _case(name, split16, True)
    _compare("train_split16_wgrad %s, train_split16 %d" % (name, split16), cfg, weights, x, x2, y, stats, got, keep=keep, key=C.KEY, l1=l1, tol=C.TOL)


# ---------------------------------------------------------------------------------------------
# 2. only the filter gradients of eligible layers move
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split16", BOTH, ids=IDS)
@pytest.mark.parametrize("name", C.NETS)
def test_only_the_filter_gradients_of_eligible_layers_change_bits(name, split16):
    cfg, weights, x, x2, y = C.inputs(name)
    _, _, _, keep, l1 = C.CASES[name]
    (s0, g0), (s1, g1) = _case(name, split16, False), _case(name, split16, True)
    assert (s0[0], s0[1], s0[3]) == (s1[0], s1[1], s1[3]), (s0, s1)
    assert abs(s1[2] - s0[2]) <= 1e-6 * s0[2], (s0, s1)
    _, g64 = R.loss_and_grads(cfg, weights, x, x2, y, keep=keep, key=C.KEY, l1=l1, l2_decay=C.L2_DECAY)
    moved = {v + "/conv_W" for v in C.eligible_layers(cfg)}
    assert moved
    for k in weights:
        same = np.array_equal(g0[k].view(np.uint32), g1[k].view(np.uint32))
        if k in moved and np.any(g64[k]):
            assert not same, "%s: the option changed no bit of an eligible layer's filter gradient" % k
        else:
            assert same, "%s: bits changed outside the eligible layers' filter gradients" % k


@pytest.mark.parametrize("split16", BOTH, ids=IDS)
def test_a_net_without_an_eligible_layer_keeps_every_bit(oracle, split16):
    cfg = oracle.make_config(**C.NARROW)
    assert not C.eligible_layers(cfg)
    weights = oracle.synthetic_weights(cfg, seed=0)
    x, x2, y = _batch(cfg, 2, 9, 7, 1)
    out = [C.bits(*_grads(cfg, weights, x, x2, y, split16, wgrad, dropout_rate=0.8)) for wgrad in (False, True)]
    assert C.same_bits(out[0], out[1])


# ---------------------------------------------------------------------------------------------
# 3. splits and borders
# ---------------------------------------------------------------------------------------------
def _plans(cfg, n, h, w):
    """{layer: the kernel's plan} of the eligible layers of a net on a batch shape (the layers behind Up-PS run at its resolution)."""
    import dcscn_oracle as O
    out, res = {}, 1
    for op in O.build_topology(cfg):
        if op["op"] != "conv":
            continue
        if C.eligible(op["cin"], op["cout"]):
            out[op["var"]] = G.wgrad_h_plan(op["k"], op["cin"], op["cout"], n, h * res, w * res)
        if op["var"].startswith("Up-PS"):
            res *= 2 if cfg["scale"] == 4 else cfg["scale"]
    return out


@pytest.mark.parametrize("split16", BOTH, ids=IDS)
def test_small_gradients_over_several_splits_with_ragged_ends(oracle, split16):
    """The wide odd-channel net as an x4 net on 3x37x50 with inputs and targets on the 0-1 scale: 88,800 HR pixels, dz ~ 7e-7.  Up-PS2
    runs on 3x74x100: two column blocks of 64 and 36 columns, 74 splits, and a last k-chunk that the tile does not fill; Up-PS on
    3x37x50 has a last row block of one row.  (The ragged last split is test_a_pixel_count_around_a_multiple_of_the_split_chunk's.)"""
    cfg, weights = _odd(oracle, scale=4)
    plans = _plans(cfg, 3, 37, 50)
    p = plans["Up-PS2/Up-PS2_CNN"]
    assert p.tiles_x == 2 and 100 % p.tc and p.splits > 1 and (p.tr * p.tcp) % 32, p
    assert 37 % plans["Up-PS/Up-PS_CNN"].tr == 1, plans["Up-PS/Up-PS_CNN"]
    x, x2, y = (a / np.float32(255.0) for a in _batch(cfg, 3, 37, 50, 1))
    stats, got = _grads(cfg, weights, x, x2, y, split16, True, key=0, l2_decay=C.L2_DECAY)
    _compare("train_split16_wgrad small gradients, train_split16 %d" % split16, cfg, weights, x, x2, y, stats, got, tol=C.TOL)


@pytest.mark.parametrize("split16", BOTH, ids=IDS)
@pytest.mark.parametrize("nhw", [(1, 1, 150), (1, 150, 1)], ids=["one-row", "one-column"])
def test_one_row_and_one_column(oracle, nhw, split16):
    """Every vertical, respectively horizontal, tap but the centre's is outside the image."""
    cfg, weights = _odd(oracle)
    x, x2, y = _batch(cfg, *nhw, 1)
    stats, got = _grads(cfg, weights, x, x2, y, split16, True, dropout_rate=C.EDGE_KEEP, l2_decay=C.L2_DECAY)
    _compare("train_split16_wgrad %dx%dx%d, train_split16 %d" % (nhw + (split16,)), cfg, weights, x, x2, y, stats, got, keep=C.EDGE_KEEP, key=C.KEY,
             tol=C.TOL)


@pytest.mark.parametrize("split16", BOTH, ids=IDS)
@pytest.mark.parametrize("name", ["aligned-2x8x8", "aligned-1x72x71"])
def test_the_aligned_net_takes_the_vector_staging_path(name, split16):
    """Every slice of the schedule 48, 32, 24 starts on a 16-byte boundary and every dz has a multiple of 4 columns but B2's."""
    cfg, weights, x, x2, y = C.edge_inputs(name)
    stats, got = _grads(cfg, weights, x, x2, y, split16, True, dropout_rate=C.EDGE_KEEP, l2_decay=C.L2_DECAY)
    _compare("train_split16_wgrad %s, train_split16 %d" % (name, split16), cfg, weights, x, x2, y, stats, got, keep=C.EDGE_KEEP, key=C.KEY, tol=C.TOL)


@pytest.mark.parametrize("h", [2399, 2400, 2401])
def test_a_pixel_count_around_a_multiple_of_the_split_chunk(oracle, h):
    """One pixel wide, so that a tile is tr consecutive pixels and a split tps * tr = 16 of them for CNN2 (40 -> 26): 2400 pixels are 150
    full splits, 2399 leave the last tile one row short, 2401 add a split of one tile of one row."""
    cfg, weights = _odd(oracle)
    p = _plans(cfg, 1, h, 1)["CNN2"]
    chunk = p.tps * p.tr * p.tc
    assert chunk == 16 and 2400 % chunk == 0 and p.splits == -(-h // chunk) and p.tps > 1, p
    assert (p.tiles % p.tps != 0) == (h == 2401) and (h % p.tr != 0) == (h != 2400), p
    x, x2, y = _batch(cfg, 1, h, 1, 1)
    stats, got = _grads(cfg, weights, x, x2, y, True, True, dropout_rate=C.EDGE_KEEP, l2_decay=C.L2_DECAY)
    _compare("train_split16_wgrad 1x%dx1" % h, cfg, weights, x, x2, y, stats, got, keep=C.EDGE_KEEP, key=C.KEY, tol=C.TOL)


# ---------------------------------------------------------------------------------------------
# 4. scaling edges
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split16", BOTH, ids=IDS)
def test_rebalancing_b1_against_b2_changes_no_bit(split16):
    """tests/test_train_split16_edges_hip.py's symmetry under its flags (no l2 term, no clipping): the exponents of B1's dz and of B2's
    input slice move by k and the gradients by exact powers of two."""
    cfg, weights, x, x2, y = C.edge_inputs("odd-2x7x9")
    flags = dict(dropout_rate=C.EDGE_KEEP, l2_decay=0.0, clipping_norm=0.0)
    stats0, got0 = _grads(cfg, weights, x, x2, y, split16, True, **flags)
    _bar("wgrad rebalancing k 0, train_split16 %d" % split16, cfg, weights, x, x2, y, stats0, got0, 0.0)
    base = C.bits(stats0, got0)
    for k in (40, -40, 90, -90):
        moved = C.rebalanced(weights, k)
        stats, got = _grads(cfg, moved, x, x2, y, split16, True, **flags)
        _bar("wgrad rebalancing k %d, train_split16 %d" % (k, split16), cfg, moved, x, x2, y, stats, got, 0.0)
        back = C.bits(stats, C.undo_rebalancing(got, k))
        differ = [n for n in got if not np.array_equal(back[n], base[n])]
        assert not differ, "k = %d: not the bits of k = 0 in %s" % (k, differ)
        assert (stats[0], stats[1], stats[3]) == (stats0[0], stats0[1], stats0[3]), (k, stats, stats0)


@pytest.mark.parametrize("split16", BOTH, ids=IDS)
def test_a_zero_input_slice(split16):
    """B1's filter and bias zero: B2's input slice is all zero (e_in = 0) while its dz is not."""
    cfg, weights, x, x2, y = C.edge_inputs("odd-2x7x9")
    zero = dict(weights)
    zero["B1/conv_W"], zero["B1/conv_B"] = np.zeros_like(weights["B1/conv_W"]), np.zeros_like(weights["B1/conv_B"])
    taps = {"B1": None, "B2": None}
    R.loss_and_grads(cfg, zero, x, x2, y, keep=C.EDGE_KEEP, key=C.KEY, taps=taps)
    assert not np.any(taps["B1"]["out"]) and np.any(taps["B2"]["dz"])
    stats, got = _grads(cfg, zero, x, x2, y, split16, True, dropout_rate=C.EDGE_KEEP, l2_decay=C.L2_DECAY)
    _compare("train_split16_wgrad zero B1, train_split16 %d" % split16, cfg, zero, x, x2, y, stats, got, keep=C.EDGE_KEEP, key=C.KEY, tol=C.TOL)


@pytest.mark.parametrize("split16", BOTH, ids=IDS)
def test_a_zero_dz(split16):
    """A target equal to the output: the last conv is zero and has no bias, so the output is x2 exactly, and so is the target.  Every dz
    is all zero (e_dz = 0), every gradient is its l2 term alone, and biases and slopes have exact zeros."""
    cfg, weights, x, x2, _ = C.edge_inputs("odd-2x7x9")
    flat = dict(weights)
    flat["R-CNN1/conv_W"] = np.zeros_like(weights["R-CNN1/conv_W"])
    assert "R-CNN1/conv_B" not in weights
    stats, got = _grads(cfg, flat, x, x2, x2, split16, True, dropout_rate=C.EDGE_KEEP, l2_decay=C.L2_DECAY)
    _, g64 = R.loss_and_grads(cfg, flat, x, x2, x2, keep=C.EDGE_KEEP, key=C.KEY, l2_decay=C.L2_DECAY)
    assert stats[1] == 0.0 and not any(np.any(g) for k, g in g64.items() if not k.endswith("/conv_W"))
    _compare("train_split16_wgrad zero dz, train_split16 %d" % split16, cfg, flat, x, x2, x2, stats, got, keep=C.EDGE_KEEP, key=C.KEY, tol=C.TOL)
    for k in weights:
        if k.endswith("/conv_W"):
            assert np.array_equal(got[k], np.float32(C.L2_DECAY) * flat[k]), k


@pytest.mark.parametrize("split16", BOTH, ids=IDS)
def test_a_non_finite_input_leaves_nothing_behind(split16):
    cfg, weights, x, x2, y = C.edge_inputs("odd-2x7x9")
    bad = x.copy()
    bad[1, 3, 4, 0] = np.inf
    flags = dict(dropout_rate=C.EDGE_KEEP, l2_decay=C.L2_DECAY)
    fresh = C.bits(*_grads(cfg, weights, x, x2, y, split16, True, **flags))
    with G.engine_for(cfg, weights, split16, True, **flags) as eng:
        stats, got = C.grads_and_stats(eng, weights, bad, x2, y)
        assert not np.isfinite(stats[0]), stats
        assert not np.isfinite(got["CNN2/conv_W"]).all(), "a non-finite input gave a finite weight gradient"
        assert C.same_bits(C.bits(*C.grads_and_stats(eng, weights, x, x2, y)), fresh), "not the bits of a fresh handle"


# ---------------------------------------------------------------------------------------------
# 5. determinism and state
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split16", BOTH, ids=IDS)
def test_two_handles_agree_over_six_adam_steps_and_the_gradient_there_is_right(oracle, split16):
    cfg, weights = _odd(oracle)
    batches = [_batch(cfg, 2, 12, 10, s) for s in (1, 2, 3)]
    x, x2, y = _batch(cfg, 1, 13, 11, 4)
    states, stats = [], []
    for _ in range(2):
        with G.engine_for(cfg, weights, split16, True, dropout_rate=0.8, l2_decay=C.L2_DECAY) as eng:
            for i in range(6):
                stats.append(eng.train_step(*batches[i % 3], 1e-3, dropout_key=1000 + i))
            states.append(_state(eng, weights))
            if len(states) == 2:
                moved = {k: states[1][k] for k in weights}
                assert all(not np.array_equal(moved[k], weights[k]) for k in weights)
                st, got = C.grads_and_stats(eng, weights, x, x2, y, key=77)
                _compare("train_split16_wgrad after 6 adam steps, train_split16 %d" % split16, cfg, moved, x, x2, y, st, got, keep=0.8, key=77, tol=C.TOL)
    _assert_same_bits(states[0], states[1])
    assert stats[:6] == stats[6:]


COMBOS = [(0, 0), (0, 1), (1, 0), (1, 1)]
KEYS = [("train_split16", 0), ("train_split16_wgrad", 1)]


def test_toggling_either_option_in_any_order_gives_the_bits_of_a_fresh_handle():
    name = "odd-1x13x11"
    cfg, weights, x, x2, y = C.inputs(name)
    fresh = {c: C.bits(*_case(name, bool(c[0]), bool(c[1]))) for c in COMBOS}
    assert len({fresh[c]["CNN2/conv_W"].tobytes() for c in COMBOS}) == 4, "the four settings do not give four different gradients"
    for start in COMBOS:
        with G.engine_for(cfg, weights, bool(start[0]), bool(start[1]), **C.train_flags(name)) as eng:
            assert C.same_bits(C.bits(*C.grads_and_stats(eng, weights, x, x2, y)), fresh[start]), start
            at = start
            for i, to in enumerate(COMBOS + COMBOS[::-1]):
                for key, idx in KEYS if i % 2 else KEYS[::-1]:          # one option at a time, in either order
                    eng.set_option(key, to[idx])
                assert C.same_bits(C.bits(*C.grads_and_stats(eng, weights, x, x2, y)), fresh[to]), "%r -> %r is not a fresh %r handle" % (at, to, to)
                at = to


def test_a_new_batch_shape_leaves_nothing_of_the_old_one(oracle):
    cfg, weights = _odd(oracle)
    a, b = _batch(cfg, 2, 7, 9, 1), _batch(cfg, 2, 16, 15, 2)
    with G.engine_for(cfg, weights, True, True, dropout_rate=0.8) as eng:
        first = C.bits(*C.grads_and_stats(eng, weights, *a))
        larger = C.bits(*C.grads_and_stats(eng, weights, *b))
        back = C.bits(*C.grads_and_stats(eng, weights, *a))
    assert C.same_bits(first, back)
    with G.engine_for(cfg, weights, True, True, dropout_rate=0.8) as fresh:
        assert C.same_bits(larger, C.bits(*C.grads_and_stats(fresh, weights, *b)))


# ---------------------------------------------------------------------------------------------
# 6. entry points, both options on
# ---------------------------------------------------------------------------------------------
def test_device_steps_and_records_match_host_steps(oracle):
    """train_step_device on a caller's stream = train_step in bits; train_local_gradients_device + train_apply_records at world 1 leave
    the bits of train_step_device."""
    cfg, weights = _odd(oracle)
    shape = (2, 12, 10)
    batches = [_batch(cfg, *shape, s) for s in (1, 2, 3)]
    flags = dict(dropout_rate=0.8, clipping_norm=0.5)
    with G.engine_for(cfg, weights, True, True, **flags) as eng:
        for i, b in enumerate(batches):
            last = eng.train_step(*b, 1e-3, dropout_key=1000 + i)
        host = _state(eng, weights)
    dev = [tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in b) for b in batches]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with G.engine_for(cfg, weights, True, True, **flags) as eng:
        for i, (x, x2, y) in enumerate(dev):
            stats = eng.train_step_device(x.data_ptr(), x2.data_ptr(), y.data_ptr(), *shape, 1e-3, dropout_key=1000 + i,
                                          stream=stream.cuda_stream, want_stats=(i == 2))
        _assert_same_bits(host, _state(eng, weights))
        assert stats == last
    with G.engine_for(cfg, weights, True, True, **flags) as eng:
        rec = torch.zeros((1, eng.train_record_floats()), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for i, (x, x2, y) in enumerate(dev):
            eng.train_local_gradients_device(x.data_ptr(), x2.data_ptr(), y.data_ptr(), *shape, rec.data_ptr(), dropout_key=1000 + i,
                                             first_index=0, stream=stream.cuda_stream)
            stats = eng.train_apply_records(rec.data_ptr(), 1, 1e-3, stream=stream.cuda_stream)
        _assert_same_bits(host, _state(eng, weights))
        assert stats[2] > 0.5 and tuple(stats) == tuple(last)
    stream.synchronize()


class _Rig(P.PatchRig):
    """test_train_parallel_hip's rig of handles on device 0, both options set before train_begin."""

    def __init__(self, cfg, weights, splits, **flags):
        self.engines = [G.engine_for(cfg, weights, True, True, **flags) for _ in splits]
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
        with _Rig(cfg, weights, (2, 1), dropout_rate=C.EDGE_KEEP, l2_decay=C.L2_DECAY) as rig:
            rig.local(dev, C.KEY)
            stats = rig.apply(1e-3, which=[0])[0]
            got = {k: rig.engines[0].get_tensor(k + "/grad") for k in weights}
            runs.append(dict(C.bits(stats, got), records=rig.records.cpu().numpy().view(np.uint32)))
    _compare("train_split16_wgrad shards 2 + 1 of odd 3x7x9", cfg, weights, x, x2, y, stats, got, keep=C.EDGE_KEEP, key=C.KEY, tol=C.TOL)
    assert C.same_bits(runs[0], runs[1])
