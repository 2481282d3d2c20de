#!/usr/bin/env python
"""Per-image time of evaluate.py's loop with the PSNR / SSIM on the host (numpy + scipy, the default) and on the device
(--device_metrics, csrc/metrics.hip), over Set14, for two nets: c-DCSCN x2 (golden L7 weights, self_ensemble 1) and L12 x4
(synthetic weights, self_ensemble 8).  Both settings run in one process, alternating, three repeats each; reported per image are
the serial do_for_evaluate loop and do_for_evaluate_many.  GPU box:  python tools/eval_metrics_time.py"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

REPEATS = 3


def _models(name):
    import dcscn_oracle as O
    from test_host import _flags
    from dcscn_amd.model import SuperResolution
    golden = os.path.join(ROOT, "tests", "golden")
    if name == "c-DCSCN x2":
        from conftest import CONFIGS
        over, ens = dict(CONFIGS["L7_F32to8_x2"]), 1
        weights = dict(np.load(os.path.join(golden, "weights_L7_x2.npz")))
    else:
        over, ens = dict(scale=4), 8
        weights = O.synthetic_weights(O.make_config(scale=4), seed=0)
    out = []
    for device_metrics in (False, True):
        m = SuperResolution(_flags(self_ensemble=ens, checkpoint_dir="/tmp", device_metrics=device_metrics, **over))
        m.build_graph()
        m.init_all_variables()
        m.load_weights(weights)
        out.append(m)
    return out


def main():
    d = os.path.join(ROOT, "tests", "golden", "set14")
    files = [os.path.join(d, f) for f in sorted(os.listdir(d))]
    n = len(files)
    for name in ("c-DCSCN x2", "L12 x4 ensemble 8"):
        host, dev = _models(name)
        values = {}
        for m in (host, dev):                                          # warm-up: buffers, plans, page cache
            values[m.device_metrics] = [m.do_for_evaluate(f) for f in files]
            m.do_for_evaluate_many(files)
        same_psnr = all(a[0] == b[0] for a, b in zip(values[False], values[True]))
        worst_ssim = max(abs(a[1] - b[1]) for a, b in zip(values[False], values[True]))
        serial = {False: [], True: []}
        many = {False: [], True: []}
        for _ in range(REPEATS):
            for m in (host, dev):
                t0 = time.perf_counter()
                for f in files:
                    m.do_for_evaluate(f)
                serial[m.device_metrics].append((time.perf_counter() - t0) / n * 1e3)
                t0 = time.perf_counter()
                m.do_for_evaluate_many(files)
                many[m.device_metrics].append((time.perf_counter() - t0) / n * 1e3)
        print("%s, Set14 (%d images), ms per image, %d repeats each, settings alternating" % (name, n, REPEATS))
        for label, runs in (("serial do_for_evaluate loop", serial), ("do_for_evaluate_many", many)):
            for on in (False, True):
                r = runs[on]
                print("  %-28s device_metrics %-5s  %s   min %.2f  spread %.2f" % (label, on, "  ".join("%.2f" % v for v in r), min(r), max(r) - min(r)))
        print("  PSNR identical: %s; worst |SSIM device - host|: %.3g" % (same_psnr, worst_ssim))
        host.close()
        dev.close()


if __name__ == "__main__":
    main()
