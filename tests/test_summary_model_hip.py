"""SuperResolution.log_to_tensorboard with --tensorboard on the GPU: the event file it writes, read back by the independent reader of
tests/tf_summary_model.py, against the reference's tags (tests/golden/ref_summary_tags.json) and the engine's summary records."""
import json
import os
import random

import numpy as np
import pytest

from conftest import CONFIGS, GOLDEN
from test_host import _flags
import tf_summary_model as M

pytestmark = pytest.mark.gpu

NAME = "dcscn_L2_F4to4_PS_R1F4"      # the shipped toy graph: the one whose tags the rules give exactly, written with l2_decay = 0
L2 = dict(layers=2, filters=4, min_filters=4, use_nin=False, reconstruct_filters=4, self_ensemble=1)
IMAGE = os.path.join(GOLDEN, "set5", "img_003.png")      # 256 x 256 RGB


def _trained_model(oracle, tmp_path, steps=2, **flags):
    from dcscn_amd.model import SuperResolution
    from helper import loader
    log = tmp_path / "tf_log"
    (log / "train").mkdir(parents=True)
    (log / "train" / "events.out.tfevents.0000000001.stale").write_bytes(b"stale")       # initialize_tf_log clears it
    m = SuperResolution(_flags(checkpoint_dir=str(tmp_path / "models"), tf_log_dir=str(log), batch_num=4, tensorboard=True, **dict(L2, **flags)))
    m.build_graph()
    m.build_optimizer()
    m.load_weights(oracle.synthetic_weights(oracle.make_config(**CONFIGS["L2_F4to4_x2"]), seed=0))
    assert m.name == NAME
    m.init_train_step()
    d = loader.DynamicDataSets(2, 24)
    d.set_data_dir(os.path.join(GOLDEN, "set14"))
    random.seed(0)
    d.init_batch_index()
    for _ in range(steps):
        m.batch_input, m.batch_input_bicubic, m.batch_true = (list(t) for t in zip(*[d.load_batch_image(255.0) for _ in range(4)]))
        m.train_batch()
    m.epochs_completed = 3
    return m, log


def _events(log):
    files = os.listdir(str(log / "train"))
    assert len(files) == 1 and files[0].startswith("events.out.tfevents.") and not files[0].endswith(".stale"), files
    assert os.listdir(str(log)) == ["train"]
    ev = M.read_events(str(log / "train" / files[0]))             # (both CRCs of every record are verified there)
    assert ev[0]["file_version"] == "brain.Event:2" and not ev[0]["values"]
    return ev[1:]


def test_log_to_tensorboard_writes_the_reference_summaries(oracle, tmp_path):
    from dcscn_amd import events
    with open(os.path.join(GOLDEN, "ref_summary_tags.json")) as f:
        ref = json.load(f)["models"][NAME]
    m, log = _trained_model(oracle, tmp_path, l2_decay=0.0)
    m.log_to_tensorboard(IMAGE, 30.0)
    eng = m._engine
    summary, psnr, lr = _events(log)
    assert summary["step"] == psnr["step"] == lr["step"] == 3 == m.epochs_completed
    scalars = {v["tag"]: v["simple_value"] for v in summary["values"] if "simple_value" in v}
    histos = {v["tag"]: v["histo"] for v in summary["values"] if "histo" in v}
    assert len(scalars) + len(histos) == len(summary["values"])
    assert sorted(scalars) == ref["scalar"] and sorted(histos) == ref["histogram"]
    assert psnr["values"] == [{"tag": "PSNR", "simple_value": np.float32(m.training_psnr_sum / 2)}] and m.training_step == 2
    assert lr["values"] == [{"tag": "LR", "simple_value": np.float32(m.lr)}]
    # every value is the engine's record of the tensor the tag names (the image is 256 x 256: x is 128 x 128)
    assert eng.summary("x")["num"] == 128 * 128 and eng.summary("y_")["num"] == 256 * 256
    checked = 0
    for kind, tag, source, field in events.summary_plan(eng.layers(), [n for n, _ in eng.tensor_specs()], NAME, l2_decay=0.0):
        if source == "loss":
            assert scalars[tag] > 0 and np.isfinite(scalars[tag])
            continue
        rec = eng.summary(source)
        if kind == "scalar":
            assert scalars[tag] == np.float32(rec[field]), tag
        else:
            h = histos[tag]
            assert (h["min"], h["max"], h["num"], h["sum"], h["sum_squares"]) == (rec["min"], rec["max"], float(rec["num"]), rec["sum"], rec["sum_squares"]), tag
            assert (h["bucket_limit"], h["bucket"]) == M.collapse(rec["buckets"]), tag
        checked += 1
    assert checked == len(summary["values"]) - 1
    # ... spelled out for a few, so that the plan does not check itself alone
    by_hand = {"CNN1/weight/mean/": ("CNN1/conv_W", "mean"), "Up-PS/Up-PS_CNN/output/stddev/": ("Up-PS/Up-PS_CNN/output", "stddev"),
               "X_1/output/mean/": ("x", "mean"), "Y_/output/stddev/": ("y_", "stddev"),
               "gradients/CNN2/CNN2_add_grad/Reshape_1_0/mean/": ("CNN2/conv_B/grad", "mean"),
               "gradients/CNN1/prelu/Mul_grad/Reshape_0/stddev/": ("CNN1/prelu/CNN1_prelu/grad", "stddev")}
    for tag, (source, field) in by_hand.items():
        assert scalars[tag + NAME] == np.float32(eng.summary(source)[field]), tag
    assert histos["CNN1/prelu/prelu_alpha/" + NAME]["num"] == 4.0
    # the records are those of the tensors the pass left behind
    M.check_record(eng.summary("R-CNN1/output"), M.summarize(eng.get_tensor("R-CNN1/output")))
    # a second call appends to the same file
    m.epochs_completed = 4
    m.log_to_tensorboard(IMAGE, 30.0)
    again = _events(log)
    assert len(again) == 6 and [e["step"] for e in again] == [3, 3, 3, 4, 4, 4]
    m.close()


def test_without_save_weights_only_the_scalars_are_written(oracle, tmp_path):
    m, log = _trained_model(oracle, tmp_path, save_weights=False, l2_decay=1e-4)
    m.log_to_tensorboard(IMAGE, 30.0)
    summary, psnr, lr = _events(log)
    values = {v["tag"]: v["simple_value"] for v in summary["values"]}
    assert sorted(values) == ["L2WeightDecayLoss/" + NAME, "Loss/" + NAME]
    assert 0 < values["L2WeightDecayLoss/" + NAME] < values["Loss/" + NAME]
    assert [v["tag"] for v in psnr["values"]] == ["PSNR"] and [v["tag"] for v in lr["values"]] == ["LR"]
    m.close()
