#!/usr/bin/env python
"""Compute time of sr.py's colour branch (model.do_for_file) per image, PNG coding excluded, two ways in one process:

  host    the host path's sequence: Pillow's RGB BICUBIC twice, convert_rgb_to_y + Pillow's mode-'F' BICUBIC, dcscn_sr_rgb
          (uploads both RGB images, downloads y and rgb as float64), save_image's four astype(uint8) casts
  device  one dcscn_sr_rgb_bytes call: one upload of the input, both resizes, the casts on the device, four uint8 downloads

for the golden c-DCSCN x2 and x4 weights on inputs of 256 x 256, 512 x 512 and 1080 x 1920 (a golden Set5 image, tiled).  Both
calls are synchronous.  After a warm-up the two alternate; reported is the median of the alternations.  The bytes of the two
are compared once per setting.  GPU box:  python tools/sr_file_time.py [--reps 20] [--out FILE]
--launches N: no timing, only N device calls per setting (for a kernel trace of the resize launches)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = ((256, 256), (512, 512), (1080, 1920))
OUTPUTS = ("rgb_bicubic", "y_bicubic", "y_out", "rgb_out")


def _engine(scale):
    import dcscn_oracle as O
    from conftest import CONFIGS, GOLDEN
    from dcscn_amd import engine
    eng = engine.Engine(O.make_config(**CONFIGS["L7_F32to8_x%d" % scale]), device=0)
    eng.load_weights(dict(np.load(os.path.join(GOLDEN, "weights_L7_x%d.npz" % scale))))
    return eng


def _image(h, w):
    from PIL import Image
    from conftest import GOLDEN
    tile = np.asarray(Image.open(os.path.join(GOLDEN, "set5", "img_003.png")).convert("RGB"))
    reps = (-(-h // tile.shape[0]), -(-w // tile.shape[1]), 1)
    return np.ascontiguousarray(np.tile(tile, reps)[:h, :w])


def host_sequence(eng, img):
    from dcscn_amd import imaging as util
    s = eng.scale
    bicubic = util.resize_image_by_pil(img, s)
    bicubic_y = util.resize_image_by_pil(util.convert_rgb_to_y(img), s)
    y, rgb = eng.sr_rgb(img, util.resize_image_by_pil(img, s), 1)
    with np.errstate(invalid="ignore"):
        return {"rgb_bicubic": bicubic.astype(np.uint8), "y_bicubic": bicubic_y.astype(np.uint8), "y_out": y.astype(np.uint8),
                "rgb_out": rgb.astype(np.uint8)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="alternations per setting (the median is reported)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    lines = ["c-DCSCN (golden L7 weights), self_ensemble 1, one MI355X; ms per image, PNG coding excluded; median of %d alternations "
             "(min .. max)" % args.reps,
             "%-6s %-12s %28s %28s %8s  %s" % ("scale", "input", "host sequence", "dcscn_sr_rgb_bytes", "ratio", "same bytes")]
    for scale in (2, 4):
        eng = _engine(scale)
        for h, w in SIZES:
            img = _image(h, w)
            if args.launches:
                for _ in range(args.launches):
                    eng.sr_rgb_bytes(img, 1)
                continue
            same = None
            for _ in range(args.warmup):
                a, b = host_sequence(eng, img), eng.sr_rgb_bytes(img, 1)
                same = all(np.array_equal(a[k].reshape(b[k].shape), b[k]) for k in OUTPUTS)
            t = {"host": [], "device": []}
            for _ in range(args.reps):
                t0 = time.perf_counter()
                host_sequence(eng, img)
                t1 = time.perf_counter()
                eng.sr_rgb_bytes(img, 1)
                t2 = time.perf_counter()
                t["host"].append((t1 - t0) * 1e3)
                t["device"].append((t2 - t1) * 1e3)
            med = {k: float(np.median(v)) for k, v in t.items()}
            cell = {k: "%9.2f (%8.2f .. %8.2f)" % (med[k], min(v), max(v)) for k, v in t.items()}
            note = "" if med["device"] <= med["host"] else "   <- the device call is slower here"
            lines.append("x%-5d %-12s %28s %28s %7.1fx  %s%s" % (scale, "%d x %d" % (h, w), cell["host"], cell["device"],
                                                                 med["host"] / med["device"], same, note))
            print(lines[-1], flush=True)
        eng.close()
    if args.launches:
        return
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
