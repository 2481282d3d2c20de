"""dcscn_train_apply_records against the arithmetic include/dcscn.h states for it, bit for bit.

The records are filled on the host (tests/train_ref.py make_records: seeded gradients with planted +-0, subnormals, a pair that
cancels across ranks and values near the float32 maximum; uneven patch counts; padding that is not zero), one handle reduces
worlds of 1 to 16 of them, and tests/train_ref.py reduce_records restates the weights, the reduction, the stats and the norm in
numpy float64 with one rounding per operation.  train.hip is compiled with fp contract(off), so nothing here has a tolerance
except adam's update (sqrtf and a float32 division chain: the 1e-6 bar of tests/test_train_surface_hip.py).  The four nets have
variable counts of every residue mod 4, which is what the ragged last quad of treduce_ranks depends on."""
import functools

import numpy as np
import pytest
import torch

from conftest import CONFIGS
import train_ref as R
from test_train_surface_hip import _close

pytestmark = pytest.mark.gpu

FLAGS = dict(optimizer="gd", beta1=0.9, beta2=0.999, epsilon=1e-8, momentum=0.9, l2_decay=1e-4, clipping_norm=5.0,
             dropout_rate=1.0, use_l1_loss=False)
# variable count mod 4 -> net
NETS = {0: CONFIGS["L2_F4to4_x2"], 1: CONFIGS["L7_F32to8_x2"], 2: CONFIGS["L7_F32to8_x3"],
        3: dict(layers=2, filters=5, min_filters=5, nin_filters=3, nin_filters2=3, reconstruct_filters=4)}
COUNTS = {0: 2604, 1: 27209, 2: 28654, 3: 1823}
WORLDS = (2, 16, 1, 8, 3)     # on one handle, in this order: the weights' buffer grows at 16, then smaller worlds run on the larger buffer
INVALID_ARG = 1


@functools.lru_cache(maxsize=None)
def _net(residue):
    import dcscn_oracle
    cfg = dcscn_oracle.make_config(**NETS[residue])
    weights = dcscn_oracle.synthetic_weights(cfg, seed=0)
    count = sum(v.size for v in weights.values())
    assert count == COUNTS[residue] and count % 4 == residue, (count, residue)
    return cfg, weights, count


@functools.lru_cache(maxsize=None)
def _records(residue, world, large=False, salt=0, fractional=False):
    """(records, restated g, stats, clip at clipping_norm 5) -- computed once, never written to."""
    count = COUNTS[residue]
    rec = R.make_records(count, world, R.RECORD_SEEDS[count] + 1000 * salt, large=large, fractional=fractional)
    for a in (rec,) + R.record_parts(rec, count):
        a.setflags(write=False)
    return rec, R.reduce_records(rec, count, 5.0)


def _engine(residue, **flags):
    from dcscn_amd import engine
    cfg, weights, count = _net(residue)
    eng = engine.Engine(cfg, device=0)
    eng.load_weights(weights)
    eng.train_begin(dict(FLAGS, **flags))
    assert eng.train_record_floats() == R.record_pad(count) + R.RECORD_TRAILER_FLOATS
    return eng


def _upload(rec):
    t = torch.from_numpy(np.array(rec)).cuda()
    torch.cuda.synchronize()
    return t


def _names(eng):
    return [(name, tuple(shape)) for name, shape in eng.tensor_specs()]


def _flat(eng, suffix=""):
    """Every variable's "<var><suffix>" in dcscn_tensor_info order as one flat float32 vector: the layout of a record."""
    return np.concatenate([eng.get_tensor(name + suffix).ravel() for name, _ in _names(eng)])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if np.asarray(a).dtype == np.float64 else np.uint32)


def _assert_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.flatnonzero(_bits(got).ravel() != _bits(want).ravel())
    assert bad.size == 0, "%s: %d of %d values differ, first at %d: %r, restated %r" % (
        what, bad.size, got.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]])


def _assert_reduction(eng, stats, want, what):
    g, ref_stats, _ = want
    _assert_bits(_flat(eng, "/grad"), g, what + " gradient")
    for i in (0, 1, 3):
        _assert_bits(np.float64(stats[i]), np.float64(ref_stats[i]), what + " stats[%d]" % i)
    _assert_bits(np.float32(stats[2]), ref_stats[2], what + " norm")
    assert np.float64(stats[2]) == np.float64(ref_stats[2])         # the double the call returns is that float32, widened


@pytest.mark.parametrize("residue", [0, 1, 2, 3])
def test_reduction_stats_and_norm_are_the_stated_arithmetic(residue):
    """Worlds 2, 16, 1, 8, 3 on one handle, each with and without values near the float32 maximum and once with fractional patch
    counts (the only ones whose sum depends on its order); a second handle gets the same tensors.  lr = 0 keeps the variables finite under the large gradients (gd: w - 0 * g)."""
    with _engine(residue) as eng, _engine(residue) as twin:
        start = _flat(eng)
        for world in WORLDS:
            for large, fractional in ((False, False), (True, False), (False, True)):
                rec, want = _records(residue, world, large, fractional=fractional)
                dev = _upload(rec)
                what = "count %d world %d large %d fractional counts %d" % (COUNTS[residue], world, large, fractional)
                stats = eng.train_apply_records(dev.data_ptr(), world, 0.0)
                _assert_reduction(eng, stats, want, what)
                assert np.isfinite(want[0]).all() and np.isfinite(want[1][2])
                stats2 = twin.train_apply_records(dev.data_ptr(), world, 0.0)
                _assert_bits(np.array(stats2), np.array(stats), what + " second handle stats")
                _assert_bits(_flat(twin, "/grad"), _flat(eng, "/grad"), what + " second handle")
        _assert_bits(_flat(eng), start, "variables after steps of lr 0")


def test_padding_floats_do_not_reach_the_gradient_or_the_norm():
    """The same records with other padding (the three nets that have some): the same bits."""
    for residue in (1, 2, 3):
        count = COUNTS[residue]
        rec, want = _records(residue, 8)
        other = np.array(rec)
        other[:, count:R.record_pad(count)] = np.float32("inf")
        with _engine(residue) as eng:
            _assert_reduction(eng, eng.train_apply_records(_upload(other).data_ptr(), 8, 0.0), want, "count %d, padding inf" % count)


@pytest.mark.parametrize("residue", [0, 1, 2, 3])
@pytest.mark.parametrize("opt", ["gd", "momentum"])
def test_unclipped_update_is_the_float32_rule_on_the_restated_gradient(residue, opt):
    """clipping_norm = 0: the factor is 1.0f, so two steps (worlds 8 and 3; the second from a non-zero accumulator) equal the numpy
    float32 emulation of tests/test_train_surface_hip.py applied to the restated g, bit for bit, on two handles."""
    lr, mu = np.float32(1e-4), np.float32(0.9)
    with _engine(residue, optimizer=opt, clipping_norm=0.0) as eng, _engine(residue, optimizer=opt, clipping_norm=0.0) as twin:
        w = start = _flat(eng)
        a = np.zeros_like(w)
        for step, world in enumerate((8, 3)):
            rec, (g, _, _) = _records(residue, world, salt=step)
            dev = _upload(rec)
            for e in (eng, twin):
                e.train_apply_records(dev.data_ptr(), world, float(lr))
            if opt == "momentum":
                a = (mu * a).astype(np.float32) + g
                w = w - (lr * a).astype(np.float32)
            else:
                w = w - (lr * g).astype(np.float32)
            assert w.dtype == np.float32 and a.dtype == np.float32
            what = "%s count %d step %d" % (opt, COUNTS[residue], step)
            for e in (eng, twin):
                _assert_bits(_flat(e), w, what + " variables")
                if opt == "momentum":
                    _assert_bits(_flat(e, "/Momentum"), a, what + " accumulator")
        assert np.isfinite(w).all() and np.count_nonzero(w != start) > w.size // 2           # the steps moved the variables


@pytest.mark.parametrize("residue", [0, 1, 2, 3])
def test_clipped_adam_update_from_the_restated_gradient(residue):
    """clipping_norm 5 is below the restated norm: variables and slots within the 1e-6 bar of R.adam applied to g * clip (clip the
    restated float32 factor), over two steps; the beta powers advance by the float32 product, bit for bit; a second handle ends
    with the same bits."""
    lr, b1, b2, eps = (float(np.float32(v)) for v in (1e-3, 0.9, 0.999, 1e-8))
    p1, p2 = np.float32(0.9), np.float32(0.999)
    with _engine(residue, optimizer="adam") as eng, _engine(residue, optimizer="adam") as twin:
        w, m, v = (_flat(eng, s).astype(np.float64) for s in ("", "/Adam", "/Adam_1"))
        for step, world in enumerate((16, 2)):
            rec, (g, stats, clip) = _records(residue, world, salt=step)
            assert stats[2] > 5.0 and clip < 1.0                   # the clip is active
            dev = _upload(rec)
            got = eng.train_apply_records(dev.data_ptr(), world, lr)
            twin.train_apply_records(dev.data_ptr(), world, lr)
            _assert_bits(np.float32(got[2]), stats[2], "norm")
            gg = g.astype(np.float64) * np.float64(clip)
            w, m, v = R.adam(w, gg, m, v, float(p1), float(p2), lr, b1=b1, b2=b2, eps=eps)
            what = "adam count %d step %d" % (COUNTS[residue], step)
            _close(_flat(eng, "/Adam"), m, what + " m")
            _close(_flat(eng, "/Adam_1"), v, what + " v")
            _close(_flat(eng), w, what)
            p1, p2 = p1 * np.float32(0.9), p2 * np.float32(0.999)
            _assert_bits(eng.get_tensor("beta1_power").reshape(()), p1, what + " beta1_power")
            _assert_bits(eng.get_tensor("beta2_power").reshape(()), p2, what + " beta2_power")
            # the next step's reference starts from the state the device really has, as the surface test does
            w, m, v = (_flat(eng, s).astype(np.float64) for s in ("", "/Adam", "/Adam_1"))
            for s in ("", "/Adam", "/Adam_1", "/grad"):
                _assert_bits(_flat(twin, s), _flat(eng, s), what + " second handle " + (s or "variables"))
            for s in ("beta1_power", "beta2_power"):
                _assert_bits(twin.get_tensor(s), eng.get_tensor(s), what + " second handle " + s)


@pytest.mark.parametrize("residue", [1, 3])
def test_refused_records_leave_zeros_in_grad_and_the_handle_recovers(residue):
    """A patch count of 0 and a count sum that is not finite, with finite gradients: DCSCN_ERR_INVALID_ARG, variables, slots and
    powers keep their bits, "<var>/grad" reads zeros (include/dcscn.h) -- and the next valid call on the handle is the restated
    step again."""
    from dcscn_amd import engine
    count, world = COUNTS[residue], 3
    pad = R.record_pad(count)
    rec, want = _records(residue, world, large=True)
    assert np.isfinite(rec[:, :count]).all()
    lr = np.float32(1e-4)
    with _engine(residue, optimizer="momentum", clipping_norm=0.0) as eng:
        first, (g0, _, _) = _records(residue, world, salt=1)
        eng.train_apply_records(_upload(first).data_ptr(), world, float(lr))          # a state that is not the initial one
        before = {s: _flat(eng, s) for s in ("", "/Momentum")}
        assert np.any(before["/Momentum"]) and np.any(_flat(eng, "/grad"))
        for counts in ((3.0, 0.0, 2.0), (1e308, 1e308, 1.0)):
            bad = np.array(rec)
            tr = bad[:, pad:].view(np.float64)
            tr[:, 2] = counts
            assert not np.isfinite(np.sum(counts)) or min(counts) == 0.0
            with pytest.raises(engine.EngineError) as e:
                eng.train_apply_records(_upload(bad).data_ptr(), world, float(lr))
            assert e.value.status == INVALID_ARG, counts
            for s in before:
                _assert_bits(_flat(eng, s), before[s], "after refused counts %r: %s" % (counts, s or "variables"))
            grad = _flat(eng, "/grad")
            assert not np.any(grad), "grad after refused counts %r: %d values are not zero, max %r" % (
                counts, np.count_nonzero(grad), float(np.max(np.abs(grad))))
        stats = eng.train_apply_records(_upload(rec).data_ptr(), world, 0.0)          # recovery: the valid records, large values and all
        _assert_reduction(eng, stats, want, "recovery, count %d" % count)
        rec2, (g2, _, _) = _records(residue, world, salt=2)
        eng.train_apply_records(_upload(rec2).data_ptr(), world, float(lr))
        # momentum's accumulator went through the large step of lr 0 as well: a = mu * a + g each time
        a = before["/Momentum"]
        a = (np.float32(0.9) * a).astype(np.float32) + want[0]
        a = (np.float32(0.9) * a).astype(np.float32) + g2
        _assert_bits(_flat(eng, "/Momentum"), a, "accumulator after recovery")
        _assert_bits(_flat(eng), before[""] - (lr * a).astype(np.float32), "variables after recovery")
