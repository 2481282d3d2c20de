"""Wall-clock time of SuperResolution.log_to_tensorboard (--tensorboard: one log pass, every summary reduced on the device, one Event
written) against the alternative it avoids, in the same process and alternating call by call: the same log pass, then every summarised
tensor downloaded with get_tensor and summarised with numpy (float64 sums, np.searchsorted over the same limits, np.bincount), then the
same Event written.  For c-DCSCN x2 and L12 x2 on one Set5 image; one JSON line per net with both medians in ms, the bytes the
alternative downloads and the bytes of the event.  There is no pass / fail ratio: the numbers go to profiles/r21_tensorboard.txt.

    python tools/tensorboard_time.py [--image tests/golden/set5/img_003.png] [--reps 3]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

NETS = {
    "c-DCSCN_x2": dict(layers=7, filters=32, min_filters=8, filters_decay_gamma=1.2, nin_filters=24, nin_filters2=8, reconstruct_layers=0,
                       pixel_shuffler_filters=1),
    "L12_x2": dict(),
}


class Flags(dict):
    __getattr__ = dict.__getitem__


def make_model(net, log_dir):
    from helper import args
    from dcscn_amd.model import SuperResolution
    flags = Flags({n: args.FLAGS._flags[n].default for n in args.FLAGS})
    flags.update(NETS[net], tensorboard=True, tf_log_dir=log_dir, checkpoint_dir=os.path.join(log_dir, "models"), log_filename="", self_ensemble=1)
    m = SuperResolution(flags)
    m.build_graph()
    m.build_optimizer()
    m.init_all_variables()
    m.init_train_step()
    return m


def numpy_record(values, limits):
    v = np.asarray(values, np.float32).ravel()
    d = v[np.isfinite(v)].astype(np.float64)
    mean = d.sum() / max(d.size, 1)
    return {"num": int(d.size), "nonfinite": int(v.size - d.size), "min": float(d.min()), "max": float(d.max()), "sum": float(d.sum()),
            "sum_squares": float(np.dot(d, d)), "mean": float(mean), "stddev": float(np.sqrt(np.mean((d - mean) ** 2))),
            "buckets": np.bincount(np.searchsorted(limits, d, side="right"), minlength=limits.size).astype(np.int64)}


def host_alternative(m, image, limits):
    """log_to_tensorboard with the summaries taken on the host: the records of the device are replaced, name by name, by numpy's of the
    downloaded tensor."""
    eng = m._engine
    device_summary = eng.summary
    downloaded = [0]

    def summary(name, want_buckets=True):
        t = eng.get_tensor(name)
        downloaded[0] += t.nbytes
        return numpy_record(t, limits)

    eng.summary = summary
    try:
        m.log_to_tensorboard(image, 0.0)
    finally:
        eng.summary = device_summary
    return downloaded[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--image", default=os.path.join(ROOT, "tests", "golden", "set5", "img_003.png"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--nets", default=",".join(NETS))
    a = ap.parse_args()
    from dcscn_amd import engine
    limits = engine.summary_bucket_limits()
    for net in a.nets.split(","):
        with tempfile.TemporaryDirectory() as tmp:
            m = make_model(net, tmp)
            m.log_to_tensorboard(a.image, 0.0)                     # warm-up: training begun, workspace carved, event file opened
            size0 = os.path.getsize(m._train_writer.path)
            device_ms, host_ms, downloaded = [], [], 0
            for _ in range(a.reps):
                t0 = time.perf_counter()
                m.log_to_tensorboard(a.image, 0.0)
                device_ms.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                downloaded = host_alternative(m, a.image, limits)
                host_ms.append((time.perf_counter() - t0) * 1e3)
            m._train_writer.flush()
            event_bytes = (os.path.getsize(m._train_writer.path) - size0) // (2 * a.reps)
            print(json.dumps({"net": net, "image": os.path.basename(a.image), "reps": a.reps,
                              "device_summaries_ms": round(statistics.median(device_ms), 2), "host_numpy_ms": round(statistics.median(host_ms), 2),
                              "ratio": round(statistics.median(host_ms) / statistics.median(device_ms), 2),
                              "host_downloaded_bytes": downloaded, "event_bytes": event_bytes,
                              "summaries": len(m._engine.summary_names())}), flush=True)
            m.close()


if __name__ == "__main__":
    main()
