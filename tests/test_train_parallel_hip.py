"""Data-parallel training (dcscn_train_local_gradients_* / dcscn_train_apply_records of include/dcscn.h).

Tests A-E run in one process: several Engine handles on device 0 stand in for the ranks, each writes its record into its row of
one [world, record_floats] tensor, and the handles reduce that tensor -- no process group.  The reference for values is the
float64 restatement of tests/train_ref.py run on the WHOLE batch (its dropout masks index the whole batch).  Test F runs
train.py under torch.distributed.run with the ranks sharing device 0 (gloo), as tests/test_multi_rank_gpu.py runs evaluate.py.
"""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import CONFIGS, GOLDEN, synthetic_batch
import train_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = dict(optimizer="adam", beta1=0.9, beta2=0.999, epsilon=1e-8, momentum=0.9, l2_decay=1e-4, clipping_norm=5.0,
             dropout_rate=1.0, use_l1_loss=False)
KEY = 0x1234567
X2, X4 = "L7_F32to8_x2", "L7_F32to8_x4"
SHAPES = {X2: (5, 8, 8), X4: (3, 6, 5)}


def _oracle():
    import dcscn_oracle
    return dcscn_oracle


@functools.lru_cache(maxsize=None)
def _net(name):
    cfg = _oracle().make_config(**CONFIGS[name])
    return cfg, _oracle().synthetic_weights(cfg, seed=0)


@functools.lru_cache(maxsize=None)
def _batch(name, seed=1):
    cfg, _ = _net(name)
    n, h, w = SHAPES[name]
    x, x2 = synthetic_batch(n, h, w, cfg["scale"], seed=seed)
    y = (x2 + np.random.default_rng(seed + 100).normal(0, 8, x2.shape)).astype(np.float32)   # a target the net does not already produce
    return x, x2, y


@functools.lru_cache(maxsize=None)
def _reference(name, keep, l1):
    """(stats, float64 gradients, global norm) of the whole batch: computed once, shared by every split of it."""
    cfg, weights = _net(name)
    x, x2, y = _batch(name)
    ref, g64 = R.loss_and_grads(cfg, weights, x, x2, y, keep=keep, key=KEY, l1=l1, l2_decay=1e-4)
    return ref, g64, R.clip_factor(g64, 0.0)[1]


def _engine(name, **flags):
    from dcscn_amd import engine
    cfg, weights = _net(name)
    eng = engine.Engine(cfg, device=0)
    eng.load_weights(weights)
    eng.train_begin(dict(FLAGS, **flags))
    return eng


def _state(eng, names, opt="adam"):
    out = {k: eng.get_tensor(k) for k in names}
    if opt == "adam":
        for k in names:
            out[k + "/Adam"] = eng.get_tensor(k + "/Adam")
            out[k + "/Adam_1"] = eng.get_tensor(k + "/Adam_1")
        out["beta1_power"] = eng.get_tensor("beta1_power")
        out["beta2_power"] = eng.get_tensor("beta2_power")
    return out


def _assert_same_bits(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]).view(np.uint32), np.asarray(b[k]).view(np.uint32)), k


class Rig:
    """`world` handles on device 0, one stream, one [world, record_floats] tensor of records."""

    def __init__(self, name, splits, make=None, **flags):
        """`make(name, **flags)` opens a rank's handle: _engine by default, another net's for tests/test_train_variants_surface_hip.py."""
        self.engines = [(make or _engine)(name, **flags) for _ in splits]
        self.bounds = np.concatenate([[0], np.cumsum(splits)])
        self.stream = torch.cuda.Stream()
        self.records = torch.zeros((len(splits), self.engines[0].train_record_floats()), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

    def close(self):
        for e in self.engines:
            e.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def local(self, dev, key):
        """Every rank's gradient of its shard of the device batch `dev` into its row of the records."""
        x, x2, y = dev
        for r, eng in enumerate(self.engines):
            b, e = int(self.bounds[r]), int(self.bounds[r + 1])
            eng.train_local_gradients_device(x[b:e].data_ptr(), x2[b:e].data_ptr(), y[b:e].data_ptr(), e - b, x.shape[1], x.shape[2],
                                             self.records[r].data_ptr(), dropout_key=key, first_index=b, stream=self.stream.cuda_stream)

    def apply(self, lr, which=None):
        """The handles `which` (all of them by default) reduce the same records; returns their stats."""
        engines = self.engines if which is None else [self.engines[i] for i in which]
        return [eng.train_apply_records(self.records.data_ptr(), len(self.engines), lr, stream=self.stream.cuda_stream) for eng in engines]


def _device(batch):
    dev = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in batch)
    torch.cuda.synchronize()
    return dev


# ---- A ------------------------------------------------------------------------------------------------------------------------

def test_world_of_one_reproduces_the_single_process_step_bit_for_bit():
    """3 adam steps with dropout and an active clip: train_step on one handle, local_gradients + apply_records(world = 1) on another."""
    from dcscn_amd import shard
    _, weights = _net(X2)
    batches = [_batch(X2, seed=s) for s in (1, 2, 3)]
    flags = dict(dropout_rate=0.8, clipping_norm=0.5)
    with _engine(X2, **flags) as one, Rig(X2, [SHAPES[X2][0]], **flags) as rig:
        assert rig.engines[0].train_record_floats() == shard.record_floats(sum(v.size for v in weights.values()))
        for i, batch in enumerate(batches):
            want = one.train_step(*batch, 1e-3, dropout_key=KEY + i)
            rig.local(_device(batch), KEY + i)
            got = rig.apply(1e-3)[0]
            print("step %d: stats %r (clipping_norm 0.5)" % (i, want))
            assert want[2] > 0.5                                              # the clip factor is < 1
            assert np.array_equal(np.array(want).view(np.uint64), np.array(got).view(np.uint64)), (want, got)
            _assert_same_bits(_state(one, weights), _state(rig.engines[0], weights))


# ---- B ------------------------------------------------------------------------------------------------------------------------

def _check_parity(name, splits, keep, l1):
    _, weights = _net(name)
    ref, g64, norm = _reference(name, keep, l1)
    with Rig(name, splits, dropout_rate=keep, use_l1_loss=l1) as rig:
        rig.local(_device(_batch(name)), KEY)
        stats = rig.apply(1e-3, which=[0])[0]
        got = {k: rig.engines[0].get_tensor(k + "/grad") for k in weights}
    _assert_parity("%s %s keep %g l1 %d" % (name, splits, keep, l1), ref, g64, norm, stats, got)


def _assert_parity(label, ref, g64, norm, stats, got):
    """The reduced gradient and the stats of rank 0 against the float64 reference of the whole batch."""
    print("%s: stats %r, reference %r norm %r" % (label, stats, ref, norm))
    for k, g in g64.items():
        err, top = float(np.max(np.abs(got[k].astype(np.float64) - g))), float(np.max(np.abs(g)))
        print("  %-40s max err %.3g  bound %.3g" % (k, err, 1e-4 * top))
        assert err <= 1e-4 * top, (k, err, top)
    assert abs(stats[0] - ref["image_loss"]) <= 1e-6 * abs(ref["image_loss"]), (stats, ref)
    assert abs(stats[1] - ref["mse"]) <= 1e-6 * abs(ref["mse"]), (stats, ref)
    assert abs(stats[3] - ref["loss"]) <= 1e-6 * abs(ref["loss"]), (stats, ref)
    assert abs(stats[2] - norm) <= 1e-4 * norm, (stats[2], norm)


@pytest.mark.parametrize("l1", [False, True], ids=["mse", "l1"])
@pytest.mark.parametrize("keep", [0.8, 1.0])
@pytest.mark.parametrize("splits", [(3, 2), (2, 2, 1)], ids=["3+2", "2+2+1"])
def test_uneven_shards_give_the_gradient_of_the_whole_batch(splits, keep, l1):
    """Fails if first_index is ignored (keep 0.8), if the shard weights are 1 / world, or if the l2 term is counted world times."""
    _check_parity(X2, splits, keep, l1)


def test_uneven_shards_x4():
    _check_parity(X4, (2, 1), 0.8, False)


# ---- C ------------------------------------------------------------------------------------------------------------------------

def test_replicas_stay_identical_and_two_runs_give_the_same_bits():
    _, weights = _net(X2)
    batches = [_device(_batch(X2, seed=s)) for s in (1, 2)]
    runs = []
    for _ in range(2):
        steps = []
        with Rig(X2, (2, 2, 1), dropout_rate=0.8) as rig:
            for i in range(6):
                rig.local(batches[i % 2], KEY + i)
                stats = rig.apply(2e-3)
                states = [_state(e, weights) for e in rig.engines]
                for s in states[1:]:
                    _assert_same_bits(states[0], s)
                assert all(np.array_equal(np.array(stats[0]).view(np.uint64), np.array(s).view(np.uint64)) for s in stats[1:])
                steps.append(states[0])
        runs.append(steps)
    assert not np.array_equal(runs[0][0]["CNN1/conv_W"], runs[0][5]["CNN1/conv_W"])          # it trains
    for a, b in zip(*runs):
        _assert_same_bits(a, b)


# ---- D ------------------------------------------------------------------------------------------------------------------------

def test_one_gd_step_of_two_ranks_against_one_handle_on_the_whole_batch():
    """Both gradients sit within 1e-4 * max|g64| of float64 (the bar of test B and of tests/test_train_hip.py), so the stepped
    weights differ by at most lr * 2e-4 * max|g64|, plus one float32 ulp of the largest |w| for the final rounding."""
    _, weights = _net(X2)
    _, g64, _ = _reference(X2, 0.8, False)
    lr = 1e-3
    flags = dict(optimizer="gd", clipping_norm=0.0, dropout_rate=0.8)
    batch = _batch(X2)
    with _engine(X2, **flags) as one, Rig(X2, (3, 2), **flags) as rig:
        one.train_step(*batch, lr, dropout_key=KEY)
        rig.local(_device(batch), KEY)
        rig.apply(lr)
        a = {k: one.get_tensor(k) for k in weights}
        b = {k: rig.engines[1].get_tensor(k) for k in weights}
    for k in weights:
        top = float(np.max(np.abs(np.concatenate([a[k].ravel(), b[k].ravel()]))))
        bound = lr * 2e-4 * float(np.max(np.abs(g64[k]))) + float(np.spacing(np.float32(top)))
        err = float(np.max(np.abs(a[k].astype(np.float64) - b[k].astype(np.float64))))
        print("%-40s max |w_a - w_b| %.3g  bound %.3g" % (k, err, bound))
        assert err <= bound, (k, err, bound)
        assert not np.array_equal(a[k], weights[k])                           # the step moved the variable


# ---- E ------------------------------------------------------------------------------------------------------------------------

def _status(call, *args, **kwargs):
    from dcscn_amd import engine
    with pytest.raises(engine.EngineError) as e:
        call(*args, **kwargs)
    return e.value.status


def test_refusals():
    from dcscn_amd import engine, shard
    cfg, weights = _net(X2)
    n, h, w = SHAPES[X2]
    x, x2, y = _device(_batch(X2))
    s = torch.cuda.Stream()
    INVALID_ARG, STATE = 1, 6
    with engine.Engine(cfg, device=0) as eng:
        eng.load_weights(weights)
        rf = eng.train_record_floats()
        rec = torch.zeros((2, rf), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        local = lambda **kw: eng.train_local_gradients_device(**dict(dict(
            x_ptr=x.data_ptr(), x2_ptr=x2.data_ptr(), y_ptr=y.data_ptr(), n=n, h=h, w=w, record_ptr=rec.data_ptr(), dropout_key=KEY,
            first_index=0, stream=s.cuda_stream), **kw))
        # before dcscn_train_begin
        assert _status(local) == STATE
        assert _status(eng.train_local_gradients_patches, [(0, 0, 0, 0)], 8, rec.data_ptr(), stream=s.cuda_stream) == STATE
        assert _status(eng.train_apply_records, rec.data_ptr(), 1, 1e-3, stream=s.cuda_stream) == STATE
        eng.train_begin(dict(FLAGS))
        image = eng.train_add_image(np.zeros((32, 32, 3), np.uint8))
        patches = lambda **kw: eng.train_local_gradients_patches(**dict(dict(
            patches=[(image, 0, 0, 0)], lr_size=8, record_ptr=rec.data_ptr(), first_index=0, stream=s.cuda_stream), **kw))
        # world < 1, first_index < 0, null pointers, n < 1
        assert _status(eng.train_apply_records, rec.data_ptr(), 0, 1e-3, stream=s.cuda_stream) == INVALID_ARG
        assert _status(eng.train_apply_records, rec.data_ptr(), -2, 1e-3, stream=s.cuda_stream) == INVALID_ARG
        assert _status(eng.train_apply_records, 0, 1, 1e-3, stream=s.cuda_stream) == INVALID_ARG
        assert _status(local, first_index=-1) == INVALID_ARG
        assert _status(patches, first_index=-1) == INVALID_ARG
        for name in ("x_ptr", "x2_ptr", "y_ptr", "record_ptr"):
            assert _status(local, **{name: 0}) == INVALID_ARG, name
        assert _status(patches, record_ptr=0) == INVALID_ARG
        assert _status(local, n=0) == INVALID_ARG
        assert _status(patches, patches=[]) == INVALID_ARG
        # records with a patch count that is not > 0, or a sum that is no finite number: nothing moves, and the call says so when asked for stats
        local()
        patches(record_ptr=rec[1].data_ptr(), first_index=n)
        s.synchronize()
        pad = rf - shard.RECORD_TRAILER_FLOATS
        before = _state(eng, weights)
        for counts in ((0.0, 0.0), (float("inf"), 1.0), (float("nan"), 1.0), (-1.0, 3.0), (0.0, 2.0)):     # the last two: a positive sum
            for r, c in enumerate(counts):
                rec[r, pad:].view(torch.float64)[2] = c
            torch.cuda.synchronize()
            assert _status(eng.train_apply_records, rec.data_ptr(), 2, 1e-3, stream=s.cuda_stream) == INVALID_ARG, counts
            _assert_same_bits(before, _state(eng, weights))
        for r, c in enumerate((float(n), 1.0)):
            rec[r, pad:].view(torch.float64)[2] = c
        torch.cuda.synchronize()
        stats = eng.train_apply_records(rec.data_ptr(), 2, 1e-3, stream=s.cuda_stream)      # the same records with their counts: a step
        assert all(np.isfinite(stats))
        assert not np.array_equal(before["CNN1/conv_W"], eng.get_tensor("CNN1/conv_W"))


# ---- G: the patch route (dcscn_train_local_gradients_patches), the one SuperResolution._train_shard_step takes -------------------

LR_SIZE = 8


@functools.lru_cache(maxsize=None)
def _set14_draw(scale, count, max_value):
    """(dataset, descriptors, the host loader's arrays) of `count` Set14 patches in which grey img_003 and RGB images both occur in
    the first 5; the seed is searched on the CPU (what a seed draws depends on the directory's file order)."""
    from test_train_batches_hip import SET14, _draw, _kinds, _seed_where
    mixed = lambda kinds: set(kinds[:5]) == {1, 3}         # (Set14 has one grey image: at most one grey patch per 14 draws)
    seed = _seed_where(SET14, scale, LR_SIZE, count, mixed)
    d, patches, want = _draw(SET14, scale, LR_SIZE, count, seed=seed, max_value=max_value)
    assert mixed(_kinds(d, patches))
    return d, tuple(patches), tuple(want)


def _descriptors(eng, d, patches, ids):
    """Device descriptors of `patches`; `ids` = this engine's {filename: image id}, filled as images are first used."""
    out = []
    for f, top, left, flip in patches:
        if f not in ids:
            ids[f] = eng.train_add_image(d.image(f))
        out.append((ids[f], top, left, flip))
    return out


class PatchRig(Rig):
    """Rig whose ranks compute their records from patch descriptors, each rank uploading only the images of its own shard."""

    def __init__(self, name, splits, **flags):
        super().__init__(name, splits, **flags)
        self.ids = [{} for _ in splits]

    def local_patches(self, d, patches, key, max_value=255.0):
        for r, eng in enumerate(self.engines):
            b, e = int(self.bounds[r]), int(self.bounds[r + 1])
            eng.train_local_gradients_patches(_descriptors(eng, d, patches[b:e], self.ids[r]), LR_SIZE, self.records[r].data_ptr(),
                                              max_value=max_value, dropout_key=key, first_index=b, stream=self.stream.cuda_stream)


@pytest.mark.parametrize("max_value", [255.0, 1.0])
@pytest.mark.parametrize("name", [X2, X4])
def test_patch_route_writes_the_record_of_the_array_route_bit_for_bit(name, max_value):
    """For the shards 3+2 and 2+2+1 of one batch: the record from descriptors equals the record from the host loader's arrays of the
    same shard with the same key and first_index, over the whole record -- gradient, padding, trailer.  Fails if first_index does
    not reach the dropout hash on the patch route (keep 0.8), or if the shard's batch is not the loader's."""
    cfg, _ = _net(name)
    d, patches, want = _set14_draw(cfg["scale"], 5, max_value)
    dev = _device(want)
    for splits in ((3, 2), (2, 2, 1)):
        with PatchRig(name, splits, dropout_rate=0.8) as by_patch, Rig(name, splits, dropout_rate=0.8) as by_array:
            by_patch.local_patches(d, patches, KEY, max_value)
            by_array.local(dev, KEY)
            torch.cuda.synchronize()
            a, b = by_patch.records.cpu().numpy(), by_array.records.cpu().numpy()
        assert np.any(a[:, :1000]) and a.shape == b.shape == (len(splits), by_patch.records.shape[1])
        for r in range(len(splits)):
            bad = np.flatnonzero(a[r].view(np.uint32) != b[r].view(np.uint32))
            assert bad.size == 0, "%s max_value %g shards %r rank %d: %d of %d record floats differ, first at %d" % (
                name, max_value, splits, r, bad.size, a.shape[1], bad[0])
        if len(splits) == 2:                                  # (and the shards differ: no rank trained on another's patches)
            assert not np.array_equal(a[0], a[1])


def test_world_of_one_through_patches_reproduces_train_step_patches_bit_for_bit():
    """3 clipped adam steps with dropout: train_step_patches on one handle, local_gradients_patches + apply_records(world = 1) on
    another.  Test A's property for the entry point train.py uses."""
    _, weights = _net(X2)
    d, patches, _ = _set14_draw(2, 15, 255.0)
    flags = dict(dropout_rate=0.8, clipping_norm=0.5)
    with _engine(X2, **flags) as one, PatchRig(X2, [5], **flags) as rig:
        ids = {}
        for i in range(3):
            batch = patches[5 * i:5 * i + 5]
            want = one.train_step_patches(_descriptors(one, d, batch, ids), LR_SIZE, 1e-3, dropout_key=KEY + i)
            rig.local_patches(d, batch, KEY + i)
            got = rig.apply(1e-3)[0]
            print("step %d: stats %r (clipping_norm 0.5)" % (i, want))
            assert want[2] > 0.5                                              # the clip factor is < 1
            assert np.array_equal(np.array(want).view(np.uint64), np.array(got).view(np.uint64)), (want, got)
            _assert_same_bits(_state(one, weights), _state(rig.engines[0], weights))


def test_shards_through_patches_give_the_gradient_of_the_whole_batch():
    """Shards 3+2 from descriptors, reduced on rank 0, against the float64 restatement on the WHOLE batch's host arrays at the bars
    of tests/test_train_surface_hip.py (gradients 1e-4 * max|g64|, losses 1e-6, norm 1e-4); keep 0.8, MSE.  Fails if both ranks
    train on shard 0, if first_index is dropped, or if the shards are weighted 1 / world."""
    from test_train_surface_hip import L2_DECAY, _compare
    cfg, weights = _net(X2)
    d, patches, (x, x2, y) = _set14_draw(2, 5, 255.0)
    with PatchRig(X2, (3, 2), dropout_rate=0.8, l2_decay=L2_DECAY) as rig:
        rig.local_patches(d, patches, KEY)
        stats = rig.apply(1e-3, which=[0])[0]
        got = {k: rig.engines[0].get_tensor(k + "/grad") for k in weights}
    _compare("patch route, shards 3+2 of 5 Set14 patches", cfg, weights, x, x2, y, stats, got, keep=0.8, key=KEY)


# ---- F ------------------------------------------------------------------------------------------------------------------------

NET_FLAGS = ["--scale=2", "--layers=7", "--filters=32", "--min_filters=8", "--filters_decay_gamma=1.2", "--nin_filters=24",
             "--nin_filters2=8", "--reconstruct_layers=0", "--pixel_shuffler_filters=1", "--self_ensemble=1", "--data_dir=" + GOLDEN,
             "--test_dataset=set5"]
TRAIN_FLAGS = ["--dataset=set14", "--batch_num=5", "--batch_image_size=24", "--training_images=80", "--initial_lr=0.002",
               "--lr_decay_epoch=1", "--end_lr=0.0015"]


def _train_py(world, port, work):
    """train.py with `world` ranks sharing device 0; returns (log, [(rank, step, digest)], flags of its directories)."""
    work.mkdir()
    dump = work / "dump.txt"
    dirs = ["--checkpoint_dir=" + str(work / "models"), "--output_dir=" + str(work / "out")]
    env = dict(os.environ, DCSCN_SHARE_GPU="1", DCSCN_TRAIN_DUMP=str(dump), MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    script = os.path.join(ROOT, "train.py")
    if world == 1:
        cmd = [sys.executable, script]
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
               "--master-port", str(port), script]
    p = subprocess.run(cmd + TRAIN_FLAGS + NET_FLAGS + dirs, env=env, cwd=str(work), capture_output=True, text=True, timeout=300)
    log = p.stdout + p.stderr
    assert p.returncode == 0, "\n".join(ln for ln in log.splitlines() if "Error" in ln)[-1500:] + "\n...\n" + log[-3000:]
    lines = [ln.split() for ln in open(dump)]
    return log, sorted((int(r), int(step), digest) for r, step, digest in lines), dirs


@pytest.fixture(scope="module")
def one_process_steps(tmp_path_factory):
    _, lines, _ = _train_py(1, 0, tmp_path_factory.mktemp("train_parallel") / "w1")
    assert len(lines) == 1 and lines[0][0] == 0
    return lines[0][1]


@pytest.mark.parametrize("world,port", [(2, 29661), (3, 29662)])
def test_train_py_with_two_and_three_ranks(tmp_path, one_process_steps, world, port):
    log, lines, dirs = _train_py(world, port, tmp_path / ("w%d" % world))
    assert [r for r, _, _ in lines] == list(range(world)), lines
    assert len({(step, digest) for _, step, digest in lines}) == 1, lines      # every replica at the same step with the same bits
    assert lines[0][1] == one_process_steps, (lines, one_process_steps)
    m = re.findall(r"Model Average \[set5\] PSNR:([0-9.]+)", log)
    assert m and len(set(m)) == 1, log[-3000:]
    trained = float(m[0])
    saved = [f for f in os.listdir(str(tmp_path / ("w%d" % world) / "models")) if f.endswith(".ckpt.index")]
    assert saved == ["dcscn_L7_F32to8_G1.20_NIN_A24_B8_PS_R1F32.ckpt.index"], saved
    e = subprocess.run([sys.executable, os.path.join(ROOT, "evaluate.py"), "--save_results=false"] + NET_FLAGS + dirs,
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    elog = e.stdout + e.stderr
    assert e.returncode == 0, elog[-3000:]
    m2 = re.search(r"Model Average \[set5\] PSNR:([0-9.]+)", elog)
    assert m2, elog[-3000:]
    assert abs(float(m2.group(1)) - trained) < 1e-3, (trained, m2.group(1))
    assert np.isfinite(trained) and trained > 0.0


# ---- H: SuperResolution.train_batch under a real process group, against the reference --------------------------------------------

@functools.lru_cache(maxsize=None)
def _driver_reference():
    """The batch tests/parallel_step_driver.py draws, drawn again on the host (load_batch_image), and the float64 restatement on
    the WHOLE batch with the dropout key of step 0: computed once for the three worlds."""
    import parallel_step_driver as D
    from test_train_batches_hip import SET14, _draw
    cfg, weights = _net(D.NET)
    _, patches, (x, x2, y) = _draw(SET14, cfg["scale"], D.BATCH_IMAGE_SIZE, D.BATCH_NUM, seed=D.SEED, max_value=255.0)
    ref, g64 = R.loss_and_grads(cfg, weights, x, x2, y, keep=D.FLAGS["dropout_rate"], key=0, l1=False, l2_decay=1e-4)
    return patches, ref, g64


@pytest.mark.parametrize("world,port", [(1, 0), (2, 29663), (3, 29664)])
def test_model_step_under_a_process_group_against_the_reference(tmp_path, world, port):
    """One gd step of SuperResolution (build_input_batch + train_batch) with `world` ranks sharing device 0 (gloo), as train.py
    runs it, from a fixed draw seed: every rank's variables lie within lr * 1e-4 * max|g64| + one float32 ulp of max|w| of
    w0 - lr * g64 (test D's bound, against the reference instead of a second run), the loss within 1e-6, all ranks hold the same
    bits.  Every rank training on shard 0, first_index = 0 on every rank, or first_index lost on the patch route each move the
    gradient by far more than that."""
    import parallel_step_driver as D
    patches, ref, g64 = _driver_reference()
    _, weights = _net(D.NET)
    env = dict(os.environ, DCSCN_SHARE_GPU="1", MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    script = os.path.join(ROOT, "tests", "parallel_step_driver.py")
    cmd = [sys.executable]
    if world > 1:
        cmd += ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
                "--master-port", str(port)]
    p = subprocess.run(cmd + [script, str(tmp_path)], env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    log = p.stdout + p.stderr
    assert p.returncode == 0, "\n".join(ln for ln in log.splitlines() if "Error" in ln)[-1500:] + "\n...\n" + log[-3000:]
    ranks = [np.load(str(tmp_path / ("rank%d.npz" % r))) for r in range(world)]
    worst = 0.0
    for r, z in enumerate(ranks):
        assert int(z["world"]) == world and int(z["key"]) == 0 and int(z["step"]) == 1 and float(z["max_value"]) == 255.0
        assert float(z["l2_decay"]) == 1e-4 and float(z["lr"]) == D.LR
        assert [(f, tuple(c)) for f, c in zip(z["files"], z["crops"].tolist())] == \
            [(os.path.basename(f), (top, left, flip)) for f, top, left, flip in patches]      # the batch the reference was given
        got = {str(n): z["t%d" % i] for i, n in enumerate(z["names"])}
        assert set(got) == set(weights)
        for k, w0 in weights.items():
            want = w0.astype(np.float64) - D.LR * g64[k]
            bound = D.LR * 1e-4 * float(np.max(np.abs(g64[k]))) + float(np.spacing(np.float32(np.max(np.abs(want)))))
            err = float(np.max(np.abs(got[k].astype(np.float64) - want)))
            moved = float(np.max(np.abs(got[k].astype(np.float64) - w0)))
            worst = max(worst, err / bound)
            print("world %d rank %d %-40s max |w - (w0 - lr g64)| %.3g  bound %.3g  (the step moved it by %.3g)" % (world, r, k, err, bound, moved))
            assert err <= bound, (world, r, k, err, bound)
            assert moved > 0.0
            assert np.array_equal(got[k].view(np.uint32), ranks[0]["t%d" % list(ranks[0]["names"]).index(k)].view(np.uint32)), (r, k)
        loss = float(z["training_loss_sum"])
        assert abs(loss - ref["image_loss"]) <= 1e-6 * abs(ref["image_loss"]), (world, r, loss, ref)
        assert loss == float(ranks[0]["training_loss_sum"])
    print("world %d: worst error / bound %.3g, image loss %.17g (reference %.17g)" % (world, worst, float(ranks[0]["training_loss_sum"]), ref["image_loss"]))
