#!/usr/bin/env python
"""Throughput of the other BASELINE.json configurations (bench.py measures configs[2]):
   python tools/bench_configs.py [--steps 5]   -> one line per config, per-launch table with --ops.
   --fast16: every config is timed with the options (fast16, S) = (0,0), (1,0), (0,1), (1,1) ALTERNATING in one process, S being the
   streamed kernels' own option -- fast16_stream where the plan has a feat3_stream launch, fast16_separable where it has a feat_stream
   or tail_stream launch (the separable configs) -- (--rounds blocks of --steps passes each, median block per setting), one line per
   setting plus their ratios; with --ops the per-launch times of the settings side by side and the streamed launches' own times per setting.
   --set KEY=VALUE (repeatable): engine options set before the weights are loaded, e.g. --set fold_whole_tail=0 for C5 with tail_stream."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

L7 = dict(layers=7, filters=32, min_filters=8, filters_decay_gamma=1.2, nin_filters=24, nin_filters2=8,
          reconstruct_layers=0, pixel_shuffler_filters=1)
CONFIGS = [
    ("C2 dcscn_L8_F96to48 x2, 256 patches", dict(layers=8, filters=96), 256),
    ("C3 dcscn_L12_F196to48 x2, 1024 patches", dict(), 1024),
    ("C4-net dcscn_L12_F196to48 x4, 512 patches", dict(scale=4), 512),
    ("C5 dcscn_L7_F32to8 x4 DS, 1024 patches", dict(L7, scale=4, depthwise_separable=True), 1024),
    ("L7 dcscn_L7_F32to8 x2 (c-DCSCN), 1024 patches", dict(L7), 1024),
    ("L7x3 dcscn_L7_F32to8 x3 (c-DCSCN), 1024 patches", dict(L7, scale=3), 1024),
    ("L7x4 dcscn_L7_F32to8 x4 (c-DCSCN), 1024 patches", dict(L7, scale=4), 1024),
    ("L8n dcscn_L8_F32to1 G1.5 x2 (octets 4 .. 1), 1024 patches", dict(L7, layers=8, min_filters=1, filters_decay_gamma=1.5), 1024),
]


SETTINGS = ((0, 0), (1, 0), (0, 1), (1, 1))           # (fast16, the streamed kernels' option)
STREAM_OPTION = {"feat3_stream": "fast16_stream", "feat_stream": "fast16_separable", "tail_stream": "fast16_separable"}


def _set(eng, setting, key):
    eng.set_option("fast16", setting[0])
    if key:
        eng.set_option(key, setting[1])


def fast16_compare(args, name, eng, torch, io):
    """(fast16, S) = (0,0), (1,0), (0,1), (1,1) in alternating blocks of args.steps passes on one handle; median block per setting.  S is
    fast16_stream or fast16_separable, whichever governs the plan's streamed launches; a plan without one ignores both: only the first two
    settings are timed there."""
    x, x2, y, n, st = io
    run = lambda: eng.forward_device(x.data_ptr(), x2.data_ptr(), y.data_ptr(), n, 48, 48, st)
    streamed = [i for i, o in enumerate(eng.ops()) if o["kernel"] in STREAM_OPTION]
    keys = sorted({STREAM_OPTION[eng.ops()[i]["kernel"]] for i in streamed})
    assert len(keys) <= 1, keys
    key = keys[0] if keys else None
    settings = SETTINGS if streamed else SETTINGS[:2]
    tag = lambda v: "fast16 %d %s %d" % (v[0], key or "fast16_stream", v[1])
    for v in settings:                                 # warm every setting (and capture its graph with --graph)
        _set(eng, v, key)
        for _ in range(3):
            run()
    torch.cuda.synchronize()
    times = {v: [] for v in settings}
    for _ in range(args.rounds):
        for v in settings:
            _set(eng, v, key)
            run()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                run()
            torch.cuda.synchronize()
            times[v].append((time.perf_counter() - t0) / args.steps * 1e3)
    med = {v: sorted(t)[len(t) // 2] for v, t in times.items()}
    for v in settings:
        print("%-48s %s  %8.3f ms/step median of %d blocks (min %.3f max %.3f)" % (name, tag(v), med[v], args.rounds, min(times[v]), max(times[v])), flush=True)
    print("%-48s (1,0) / (0,0) = %.4f" % (name, med[(1, 0)] / med[(0, 0)]), flush=True)
    if streamed:
        print("%-48s (0,1) / (0,0) = %.4f   (1,1) / (1,0) = %.4f   (1,1) / (0,0) = %.4f" % (
            name, med[(0, 1)] / med[(0, 0)], med[(1, 1)] / med[(1, 0)], med[(1, 1)] / med[(0, 0)]), flush=True)
    if args.ops and not args.graph:
        per = {}
        eng.set_option("profile", 1)
        rows = {v: [] for v in settings}
        for _ in range(args.steps):                    # alternating here too: one profiled pass per setting and round
            for v in settings:
                _set(eng, v, key)
                run()
                torch.cuda.synchronize()
                rows[v].append(eng.profile())
        for v in settings:
            per[v] = [sorted(c)[len(c) // 2] for c in zip(*rows[v])]
        eng.set_option("profile", 0)
        for i, o in enumerate(eng.ops()):
            base = per[settings[0]][i]
            print("    %-26s %-12s k%d %4d->%-4d res%d  " % (o["name"], o["kernel"], o["kernel_size"], o["in_channels"], o["out_channels"], o["resolution"])
                  + "  ".join("(%d,%d) %7.3f ms" % (v + (per[v][i],)) for v in settings)
                  + "  ratio to (0,0) " + " ".join("%.3f" % (per[v][i] / base if base else 0) for v in settings[1:]))
        print("    %-26s " % "sum of launches" + "  ".join("(%d,%d) %7.3f ms" % (v + (sum(per[v]),)) for v in settings), flush=True)
        for i in streamed:                             # the streamed launch's own time per setting
            print("    %s launch %-22s " % (eng.ops()[i]["kernel"], eng.ops()[i]["name"]) + "  ".join("(%d,%d) %7.3f ms" % (v + (per[v][i],)) for v in settings)
                  + "  (0,1) / (0,0) = %.4f  (1,1) / (1,0) = %.4f" % (per[(0, 1)][i] / per[(0, 0)][i], per[(1, 1)][i] / per[(1, 0)][i]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--ops", action="store_true")
    ap.add_argument("--only", default="")
    ap.add_argument("--graph", action="store_true", help="option graph_replay: the pass replayed from a hipGraph")
    ap.add_argument("--fast16", action="store_true", help="time (fast16, fast16_stream or fast16_separable) = (0,0), (1,0), (0,1), (1,1) alternating in one process and print the ratios")
    ap.add_argument("--set", action="append", default=[], metavar="KEY=VALUE", help="engine option set before the weights are loaded (repeatable)")
    ap.add_argument("--rounds", type=int, default=7, help="--fast16: timed blocks per setting")
    args = ap.parse_args()
    import torch
    import dcscn_oracle as O
    from dcscn_amd import engine
    for name, flags, n in CONFIGS:
        if args.only and args.only not in name:
            continue
        cfg = O.make_config(**flags)
        eng = engine.Engine(cfg)
        for kv in args.set:
            k, v = kv.split("=")
            eng.set_option(k, int(v))
            name = "%s %s" % (name, kv)
        eng.load_weights(O.synthetic_weights(cfg, seed=0))
        s = cfg["scale"]
        x = torch.rand((n, 48, 48, 1), device="cuda") * 255
        x2 = torch.rand((n, 48 * s, 48 * s, 1), device="cuda") * 255
        y = torch.empty_like(x2)
        st = torch.cuda.current_stream().cuda_stream
        if args.graph:
            eng.set_option("graph_replay", 1)
        if args.fast16:
            fast16_compare(args, name, eng, torch, (x, x2, y, n, st))
            eng.close()
            continue
        for _ in range(3):
            eng.forward_device(x.data_ptr(), x2.data_ptr(), y.data_ptr(), n, 48, 48, st)
        if not args.graph:
            eng.set_option("profile", 1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            eng.forward_device(x.data_ptr(), x2.data_ptr(), y.data_ptr(), n, 48, 48, st)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.steps
        ms = eng.profile()
        ops = eng.ops()
        px = n * 48 * 48
        macs = sum(o["macs_per_lr_pixel"] for o in ops)
        by = sum(o["bytes_per_lr_pixel"] for o in ops)
        print("%-48s %8.3f ms/step  %8.2f LR Mpix/s  %7.2f TFLOP/s  %7.1f GB/s (unfused activation bytes)  kernels %.3f ms"
              % (name, dt * 1e3, px / dt / 1e6, 2 * macs * px / dt / 1e12, by * px / dt / 1e9, sum(ms)), flush=True)
        if args.ops:
            for o, m in zip(ops, ms):
                # a folded tail executes the composite 5x5 conv, not the layers it replaces: the direct-form MACs of those layers over its
                # time would read as a rate above the chip's peak -- the executed MACs are the ones that make a rate
                folded = "(folded)" in o["name"]
                macs_o = o["executed_macs_per_lr_pixel"] if folded else o["macs_per_lr_pixel"]
                print("    %-26s %-11s k%d %4d->%-4d res%d  %8.3f ms  %7.2f TFLOP/s%s  %7.1f GB/s" % (
                    o["name"], o["kernel"], o["kernel_size"], o["in_channels"], o["out_channels"], o["resolution"], m,
                    2 * macs_o * px / (m * 1e-3) / 1e12 if m else 0, " (executed, composite)" if folded else "",
                    o["bytes_per_lr_pixel"] * px / (m * 1e-3) / 1e9 if m else 0))
        eng.close()


if __name__ == "__main__":
    main()
