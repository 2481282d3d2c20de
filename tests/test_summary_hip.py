"""The device reduction of csrc/summary.hip (Engine.summarize_device) and the log pass (Engine.train_log_pass / summary) against the numpy
restatement of tests/tf_summary_model.py.

Bars (all double against double): bucket counts, min, max, num and nonfinite exact; sum and sum_squares within 1e-12 of fsum(|v|) resp.
fsum(v^2); mean and stddev within 1e-10 relative.  A relative bar on a mean says nothing where the values cancel to exactly zero, so the
families with both signs draw their signs at random instead of pairing them."""
import numpy as np
import pytest
import torch

from conftest import CONFIGS
import tf_summary_model as M

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 4097, 2 ** 20 + 3]
FAMILIES = ["zeros", "constant", "limits", "tiny", "huge", "nonfinite", "weights"]


def _nearest_f32(limit):
    """The float32 values next to a limit: the nearest one, and its neighbours below and above."""
    a = np.float32(limit)
    return [np.nextafter(a, np.float32(-np.inf)), a, np.nextafter(a, np.float32(np.inf))]


def family(name, n, seed=0):
    rng = np.random.default_rng(seed + n)
    if name == "zeros":
        return np.zeros(n, np.float32)
    if name == "constant":
        return np.full(n, 0.1234567, np.float32)
    if name == "limits":
        # a sample of the limits of both signs (all of them that float32 can hold lie inside the table's -1e20 .. 1e20), and 0.0
        idx = np.concatenate([rng.choice(np.arange(1, M.LIMITS.size - 1), 96, replace=False), [775, 776, 774, 1, M.LIMITS.size - 2]])
        pool = np.array([v for i in idx for v in _nearest_f32(M.LIMITS[i])], np.float32)
    elif name == "tiny":
        # between 0 and +-1e-12: +-1e-13 and denormals (the smallest, a middle one, the largest), and the first limits themselves
        pool = np.array([1e-13, -1e-13, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38, -1.1754942e-38, 1e-12, -1e-12, 0.0, -0.0], np.float32)
    elif name == "huge":
        pool = np.array([3e38, -3e38, 3.4028235e38, -3.4028235e38, 1e20, -1e20, 9.9207756e19], np.float32)
    elif name == "nonfinite":
        v = rng.normal(0, 1, n).astype(np.float32)
        v[::7] = np.nan
        v[3::11] = np.inf
        v[5::13] = -np.inf
        return v
    elif name == "weights":
        return (rng.normal(0, 1, n) * 1e-3).astype(np.float32)
    else:
        raise KeyError(name)
    return pool[rng.integers(0, pool.size, n)]


@pytest.fixture(scope="module")
def eng():
    from dcscn_amd import engine
    with engine.Engine(CONFIGS["L2_F4to4_x2"], device=0) as e:      # (no weights, no finalize: summarize_device needs neither)
        yield e


# every family at every size, and with the pointer one float past the allocation's start at the smallest size, a ragged one and one of two chunks
CASES = [(f, n, 0) for f in FAMILIES for n in SIZES] + [(f, n, 1) for f in FAMILIES for n in (1, 65, 4097)]


@pytest.mark.parametrize("name,n,offset", CASES, ids=["%s-%d%s" % (f, n, "-offset" if o else "") for f, n, o in CASES])
def test_summarize_device_matches_restatement(eng, name, n, offset):
    v = family(name, n)
    buf = torch.zeros(n + offset, dtype=torch.float32, device="cuda")
    buf[offset:] = torch.from_numpy(v).cuda()
    torch.cuda.synchronize()
    ptr = buf.data_ptr() + 4 * offset
    got = eng.summarize_device(ptr, n)
    again = eng.summarize_device(ptr, n)
    want = M.summarize(v)
    print(name, n, {k: got[k] for k in got if k != "buckets"})
    M.check_record(got, want, exact_stddev_zero=name in ("zeros", "constant"))
    for k in got:
        assert np.asarray(got[k]).tobytes() == np.asarray(again[k]).tobytes(), k      # two calls, the same bytes
    assert int(got["buckets"].sum()) == want["num"]


def test_bucket_limits_on_the_device_are_the_host_table(eng):
    """Every limit itself, as the float32 nearest to it, lands where the restatement puts it: the device searches the uploaded table."""
    v = np.array([x for l in M.LIMITS[1:-1] for x in _nearest_f32(l)], np.float32)
    buf = torch.from_numpy(v).cuda()
    got = eng.summarize_device(buf.data_ptr(), v.size)
    assert np.array_equal(got["buckets"], M.summarize(v)["buckets"])


# ---- log pass ----
NIN = dict(layers=3, filters=8, min_filters=4, nin_filters=6, nin_filters2=4)
NETS = {
    "L2_x2": (CONFIGS["L2_F4to4_x2"], ()),
    "nin_x2": (NIN, ()),
    "nin_x4": (dict(NIN, scale=4), ()),
    "nin_x2_separable": (dict(NIN, depthwise_separable=True), ("train_separable",)),
    "nin_x2_transposed": (dict(NIN, pixel_shuffler=False), ("train_transposed",)),
}
TRAIN = dict(optimizer="adam", beta1=0.9, beta2=0.999, epsilon=1e-8, momentum=0.9, l2_decay=1e-4, clipping_norm=5.0, dropout_rate=1.0,
             use_l1_loss=False)


def _net(oracle, name, **flags):
    """(engine, weights, x, x2, y) of a net of NETS on the 1 x 8 x 12 batch."""
    from dcscn_amd import engine
    from train_ref_separable import batch
    spec, options = NETS[name]
    cfg = oracle.make_config(**spec)
    weights = oracle.synthetic_weights(cfg, seed=3)
    e = engine.Engine(cfg, device=0)
    e.load_weights(weights)
    for key in options:
        e.set_option(key, 1)
    e.train_begin(dict(TRAIN, **flags))
    return (e, weights) + batch(cfg, 1, 8, 12, 4)


def _state(e, weights):
    out = {}
    for k in weights:
        for suffix in ("", "/Adam", "/Adam_1"):
            out[k + suffix] = e.get_tensor(k + suffix)
    out["beta1_power"], out["beta2_power"] = e.get_tensor("beta1_power"), e.get_tensor("beta2_power")
    return out


def _same_bits(a, b):
    assert a.keys() == b.keys()
    return [k for k in a if not np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32))]


@pytest.mark.parametrize("net", list(NETS))
def test_log_pass_summaries_are_the_restatement_of_the_tensors(oracle, net):
    e, weights, x, x2, y = _net(oracle, net, dropout_rate=0.8)
    with e:
        stats = e.train_log_pass(x, x2, y)
        names = e.summary_names()
        assert len(names) == 2 * len(weights) + len(e.layers()) + 2
        outputs = {}
        for name in names:
            t = e.get_tensor(name)
            if name.endswith("/output") or name in ("x", "y_"):
                outputs[name] = t
            M.check_record(e.summary(name), M.summarize(t))
            assert e.summary(name)["nonfinite"] == 0
        # the activations are the graph's: x is the input, y_ the last layer + x2, and every layer's output has the layer's shape
        assert np.array_equal(outputs["x"], x.reshape(outputs["x"].shape))
        last = e.layers()[-1]["name"] + "/output"
        assert np.array_equal(outputs["y_"], outputs[last] + x2.reshape(outputs[last].shape))
        for l in e.layers():
            assert outputs[l["name"] + "/output"].shape[3] == l["out_channels"] and np.any(outputs[l["name"] + "/output"] != 0)
        assert stats[3] >= stats[0] > 0


def test_log_pass_runs_with_dropout_off(oracle):
    e, weights, x, x2, y = _net(oracle, "nin_x2", dropout_rate=0.8)
    twin = _net(oracle, "nin_x2", dropout_rate=1.0)[0]
    with e, twin:
        s = e.train_log_pass(x, x2, y)
        g = {k: e.get_tensor(k + "/grad") for k in weights}
        st = twin.train_gradients(x, x2, y)
        gt = {k: twin.get_tensor(k + "/grad") for k in weights}
        assert s == st and not _same_bits(g, gt)
        e.train_gradients(x, x2, y, dropout_key=5)
        gd = {k: e.get_tensor(k + "/grad") for k in weights}
        assert len(_same_bits(g, gd)) > 0                      # the handle's own gradients drop units: other bits
        with pytest.raises(Exception) as err:                  # ... and that call took the activations
            e.get_tensor("CNN1/output")
        assert err.value.status == 6
        M.check_record(e.summary("CNN1/conv_W/grad"), M.summarize(g["CNN1/conv_W"]))   # the records of the pass stay


def test_log_pass_changes_no_training_state_and_no_later_step(oracle):
    e, weights, x, x2, y = _net(oracle, "nin_x2", dropout_rate=0.8)
    twin = _net(oracle, "nin_x2", dropout_rate=0.8)[0]
    with e, twin:
        for h in (e, twin):
            h.train_step(x, x2, y, 1e-3, dropout_key=1)
        before = _state(e, weights)
        e.train_log_pass(x, x2, y)
        e.train_log_pass(np.concatenate([x, x]), np.concatenate([x2, x2]), np.concatenate([y, y]))     # another carve in between
        assert not _same_bits(before, _state(e, weights))
        for h in (e, twin):
            h.train_step(x, x2, y, 1e-3, dropout_key=2)
        assert not _same_bits(_state(e, weights), _state(twin, weights))


def test_summary_before_any_log_pass_is_a_state_error(oracle):
    e, weights, x, x2, y = _net(oracle, "L2_x2")
    with e:
        e.train_step(x, x2, y, 1e-3)
        with pytest.raises(Exception) as err:
            e.summary("CNN1/conv_W")
        assert err.value.status == 6
        e.train_log_pass(x, x2, y)
        with pytest.raises(Exception) as err:
            e.summary("no/such/tensor")
        assert err.value.status == 4
