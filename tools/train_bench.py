"""Training step time of the HIP path (dcscn_train_step_device) and of a torch-ROCm fp32 autograd + Adam step of the same net.

Prints one JSON line: ms per step (median over --steps after --warmup, HIP events), the conv FLOPs of one step and their rate
as a fraction of the 157.3 TFLOP/s f32 matrix peak, and -- from a child process of its own -- the torch step time.  The split
into forward / dgrad / wgrad / loss / optimizer comes from a separate profiler run of this script with --no-torch
(tools/summarize_train_prof.py groups the kernel names).

    python tools/train_bench.py --config L7_x2 --batch 20 --size 48

--loop times train.py's loop body instead, build_input_batch() + train_batch() of SuperResolution over Set14, for c-DCSCN x2
(20 x 48^2), L12 x2 (20 x 48^2) and c-DCSCN x4 (20 x 32^2): host batches (the arrays of helper/loader.py load_batch_image,
stepped with dcscn_train_step) against device batches (patch descriptors, dcscn_train_step_patches), alternating step by step in
one process, each timed on the host clock up to the step's stats read-back; one JSON line per net, with the bare
dcscn_train_step_device time of the same batch shape for scale.  --device-only runs only the device leg (profiler runs).

    python tools/train_bench.py --loop

--split16 times option "train_split16" = 0 and 1 (include/dcscn.h) on two handles of one process, alternating step by step, for L12 x2
and c-DCSCN x2 at 20 x 48^2: one JSON line per net with both medians and their ratio.  --train-split16 sets the option on the
plain run's handle (profiler runs of the option-on step).  --library PATH times another build of the library, e.g. the parent
commit's, in a process of its own.

    python tools/train_bench.py --split16

--split16-wgrad does the same with three handles, (train_split16, train_split16_wgrad) = (0, 0), (1, 0), (1, 1); --train-split16-wgrad
sets the second option on the plain run's handle.

    python tools/train_bench.py --split16-wgrad

--separable times the depthwise-separable nets (option "train_separable"; L7_x4_DS is BASELINE C5, 20 x 32^2): the HIP step and a torch
fp32 autograd + Adam step of the same net (a grouped conv2d + a 1x1 conv per separable layer), alternating step by step in ONE process;
one JSON line per net with both medians and their ratio.  --config L7_x4_DS --no-torch is the profiler run's command.

    python tools/train_bench.py --separable

--transposed does the same for the transposed-conv nets (--pixel_shuffler=false, option "train_transposed"): L12_x2_T is the reference's
defaults with pixel_shuffler = false (its README's training command line), L7_x2_T the c-DCSCN x2 topology, both at 20 x 48^2.
--config L7_x2_T --no-torch is the profiler run's command (its pixel-shuffler twin at the same shape: --config L7_x2_PS32; L12_x2_T's is L12_x2).

    python tools/train_bench.py --transposed

--optimizer NAME sets --optimizer of the plain run's handle (adadelta, adagrad and rmsprop behind option "train_optimizers"); a comma-separated
list times one handle per name, alternating step by step in ONE process, and prints one JSON line with every median.

    python tools/train_bench.py --optimizer adam,adagrad,adadelta,rmsprop

--augment times the device-batch loop of --loop at --train_augment_level 0 and 8 (helper/loader.py: the eight flipped / rotated variants of
every image, cut from the one uploaded image by batch_gather's index map) on two models of one process, alternating step by step, for
c-DCSCN x2 at 20 x 48^2: one JSON line with both medians and their ratio.

    python tools/train_bench.py --augment
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dcscn_oracle as O  # noqa: E402

CONFIGS = {
    "L7_x2": dict(layers=7, filters=32, min_filters=8, filters_decay_gamma=1.2, nin_filters=24, nin_filters2=8,
                  reconstruct_layers=0, pixel_shuffler_filters=1),
    "L12_x2": dict(),
    "L7_x4": dict(scale=4, layers=7, filters=32, min_filters=8, filters_decay_gamma=1.2, nin_filters=24, nin_filters2=8,
                  reconstruct_layers=0, pixel_shuffler_filters=1),
    "L7_x4_DS": dict(scale=4, layers=7, filters=32, min_filters=8, filters_decay_gamma=1.2, nin_filters=24, nin_filters2=8,
                     reconstruct_layers=0, pixel_shuffler_filters=1, depthwise_separable=True),
    "L7_x2_DS": dict(layers=7, filters=32, min_filters=8, filters_decay_gamma=1.2, nin_filters=24, nin_filters2=8,
                     reconstruct_layers=0, pixel_shuffler_filters=1, depthwise_separable=True),
    # the pixel-shuffler twin of L7_x2_T at the same shape: Up-PS from 32 to 4 x 32 channels (L7_x2's has pixel_shuffler_filters = 1)
    "L7_x2_PS32": dict(layers=7, filters=32, min_filters=8, filters_decay_gamma=1.2, nin_filters=24, nin_filters2=8, reconstruct_layers=0),
    "L12_x2_T": dict(pixel_shuffler=False),
    "L7_x2_T": dict(layers=7, filters=32, min_filters=8, filters_decay_gamma=1.2, nin_filters=24, nin_filters2=8,
                    reconstruct_layers=0, pixel_shuffler=False),
}
TRANSPOSED_CASES = (("L12_x2_T", 20, 48), ("L7_x2_T", 20, 48))
SEPARABLE_CASES = (("L7_x4_DS", 20, 32), ("L7_x2_DS", 20, 48))
LOOP_CASES = (("L7_x2", 20, 48), ("L12_x2", 20, 48), ("L7_x4", 20, 32))
PEAK_F32_MATRIX = 157.3e12


def step_flops(cfg, n, h, w):
    """f32 FLOPs of the convs of one step: forward, data gradient (not for CNN1) and weight gradient, 2 per MAC each."""
    total = 0
    first = True
    res = 1
    for op in O.build_topology(cfg):
        if op["op"] == "depth_to_space":
            res *= op["block"]
        if op["op"] == "conv_transpose":      # k^2 C^2 MACs per input pixel in each of the three directions
            k = 2 * op["scale"] - op["scale"] % 2
            total += 2 * n * h * w * res * res * k * k * op["channels"] ** 2 * 3
            res *= op["scale"]
        if op["op"] != "conv":
            continue
        per_pixel = op["k"] * op["k"] * op["cin"] + op["cin"] * op["cout"] if op["ds"] else op["k"] * op["k"] * op["cin"] * op["cout"]
        macs = n * h * w * res * res * per_pixel
        total += 2 * macs * (2 if first else 3)
        first = False
    return total


def flags(optimizer="adam"):
    return dict(optimizer=optimizer, momentum=0.9, beta1=0.9, beta2=0.999, epsilon=1e-8, l2_decay=1e-4, clipping_norm=5.0, dropout_rate=0.8)


def batch(cfg, n, h, w):
    rng = np.random.default_rng(0)
    s = cfg["scale"]
    x = rng.uniform(0, 255, (n, h, w, 1)).astype(np.float32)
    x2 = np.repeat(np.repeat(x, s, axis=1), s, axis=2)
    y = (x2 + rng.normal(0, 8, x2.shape)).astype(np.float32)
    return x, x2, y


def bench_split16(name, n, size, steps, warmup):
    """train_split16 = 0 and 1 on two handles with the same weights and batch, alternating step by step on one stream."""
    from dcscn_amd import engine
    cfg = O.make_config(**CONFIGS[name])
    engs = []
    for on in (0, 1):
        eng = engine.Engine(cfg, device=0)
        eng.load_weights(O.synthetic_weights(cfg, seed=0))
        eng.set_option("train_split16", on)
        eng.train_begin(flags())
        engs.append(eng)
    x, x2, y = (torch.from_numpy(a).cuda() for a in batch(cfg, n, size, size))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    times = ([], [])
    for i in range(warmup + steps):
        for on, eng in enumerate(engs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            eng.train_step_device(x.data_ptr(), x2.data_ptr(), y.data_ptr(), n, size, size, 1e-4, i, stream=sp, want_stats=False)
            b.record(stream)
            b.synchronize()
            if i >= warmup:
                times[on].append(a.elapsed_time(b))
    for eng in engs:
        eng.close()
    off, on = float(np.median(times[0])), float(np.median(times[1]))
    return dict(split16_compare=name, batch=n, lr_size=size, steps=steps, warmup=warmup, train_split16_0_ms=round(off, 4),
                train_split16_1_ms=round(on, 4), ratio_1_over_0=round(on / off, 4),
                min_ms=[round(float(np.min(times[0])), 4), round(float(np.min(times[1])), 4)])


WGRAD_LEGS = ((0, 0), (1, 0), (1, 1))       # (train_split16, train_split16_wgrad)


def bench_split16_wgrad(name, n, size, steps, warmup):
    """(train_split16, train_split16_wgrad) = (0, 0), (1, 0), (1, 1) on three handles with the same weights and batch, alternating step
    by step on one stream."""
    from dcscn_amd import engine
    cfg = O.make_config(**CONFIGS[name])
    engs = []
    for s16, wg in WGRAD_LEGS:
        eng = engine.Engine(cfg, device=0)
        eng.load_weights(O.synthetic_weights(cfg, seed=0))
        eng.set_option("train_split16", s16)
        eng.set_option("train_split16_wgrad", wg)
        eng.train_begin(flags())
        engs.append(eng)
    x, x2, y = (torch.from_numpy(a).cuda() for a in batch(cfg, n, size, size))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    times = [[] for _ in engs]
    for i in range(warmup + steps):
        for k, eng in enumerate(engs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            eng.train_step_device(x.data_ptr(), x2.data_ptr(), y.data_ptr(), n, size, size, 1e-4, i, stream=sp, want_stats=False)
            b.record(stream)
            b.synchronize()
            if i >= warmup:
                times[k].append(a.elapsed_time(b))
    for eng in engs:
        eng.close()
    med = [float(np.median(t)) for t in times]
    return dict(split16_wgrad_compare=name, batch=n, lr_size=size, steps=steps, warmup=warmup, legs=[list(leg) for leg in WGRAD_LEGS],
                ms=[round(m, 4) for m in med], min_ms=[round(float(np.min(t)), 4) for t in times],
                ratio_11_over_10=round(med[2] / med[1], 4), ratio_11_over_00=round(med[2] / med[0], 4))


def hip_engine(cfg, optimizer="adam"):
    """A training handle on synthetic weights; a separable net gets option "train_separable", a transposed-conv net option
    "train_transposed" and adadelta / adagrad / rmsprop option "train_optimizers", which train_begin reads."""
    from dcscn_amd import engine
    eng = engine.Engine(cfg, device=0)
    eng.load_weights(O.synthetic_weights(cfg, seed=0))
    if cfg["depthwise_separable"]:
        eng.set_option("train_separable", 1)
    if not cfg["pixel_shuffler"]:
        eng.set_option("train_transposed", 1)
    if optimizer in engine.MORE_OPTIMIZERS:
        eng.set_option("train_optimizers", 1)
    eng.train_begin(flags(optimizer))
    return eng


def bench_optimizers(name, optimizers, n, size, steps, warmup):
    """One handle per optimizer with the same weights and batch, alternating step by step on one stream."""
    cfg = O.make_config(**CONFIGS[name])
    engs = [hip_engine(cfg, opt) for opt in optimizers]
    x, x2, y = (torch.from_numpy(a).cuda() for a in batch(cfg, n, size, size))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    times = [[] for _ in engs]
    for i in range(warmup + steps):
        for k, eng in enumerate(engs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            eng.train_step_device(x.data_ptr(), x2.data_ptr(), y.data_ptr(), n, size, size, 1e-4, i, stream=stream.cuda_stream, want_stats=False)
            b.record(stream)
            b.synchronize()
            if i >= warmup:
                times[k].append(a.elapsed_time(b))
    for eng in engs:
        eng.close()
    med = [float(np.median(t)) for t in times]
    return dict(optimizer_compare=name, batch=n, lr_size=size, steps=steps, warmup=warmup, optimizers=list(optimizers),
                ms=[round(m, 4) for m in med], min_ms=[round(float(np.min(t)), 4) for t in times],
                ratio_to_first=[round(m / med[0], 4) for m in med])


def bench_hip(cfg, n, h, w, steps, warmup, train_split16=False, train_split16_wgrad=False, optimizer="adam"):
    eng = hip_engine(cfg, optimizer)
    if train_split16:
        eng.set_option("train_split16", 1)
    if train_split16_wgrad:
        eng.set_option("train_split16_wgrad", 1)
    x, x2, y = (torch.from_numpy(a).cuda() for a in batch(cfg, n, h, w))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()          # a real stream: the events below are recorded where the steps run
    sp = stream.cuda_stream
    for i in range(warmup):
        eng.train_step_device(x.data_ptr(), x2.data_ptr(), y.data_ptr(), n, h, w, 1e-4, i, stream=sp, want_stats=False)
    torch.cuda.synchronize()
    times = []
    for i in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        eng.train_step_device(x.data_ptr(), x2.data_ptr(), y.data_ptr(), n, h, w, 1e-4, warmup + i, stream=sp, want_stats=False)
        b.record(stream)
        b.synchronize()
        times.append(a.elapsed_time(b))
    eng.close()
    return float(np.median(times)), float(np.min(times))


def torch_step(cfg, n, h, w):
    """The same net as torch fp32 modules on the GPU: autograd + torch.optim.Adam (dropout included); a separable layer is a grouped
    conv2d followed by a 1x1 conv.  Returns the function that takes one step."""
    import torch.nn.functional as F
    torch.backends.cudnn.benchmark = True
    dev = torch.device("cuda")
    params = {k: torch.tensor(v, device=dev, requires_grad=True) for k, v in O.synthetic_weights(cfg, seed=0).items()}
    conv_w = {k: v for k, v in params.items() if k.endswith(("/conv_W", "/Tconv_W"))}
    opt = torch.optim.Adam(params.values(), lr=1e-4, betas=(0.9, 0.999), eps=1e-8)
    x, x2, y = (torch.from_numpy(a).to(dev).permute(0, 3, 1, 2).contiguous() for a in batch(cfg, n, h, w))
    ops = O.build_topology(cfg)

    def step():
        t = {"x": x, "x2": x2}
        for op in ops:
            if op["op"] == "conv":
                v = op["var"]
                if op["ds"]:
                    z = F.conv2d(t[op["src"]], params[v + "/depthwise_W"].permute(2, 3, 0, 1), padding=op["k"] // 2, groups=op["cin"])
                    z = F.conv2d(z, params[v + "/pointwise_W"].permute(3, 2, 0, 1))
                else:
                    z = F.conv2d(t[op["src"]], params[v + "/conv_W"].permute(3, 2, 0, 1), padding=op["k"] // 2)
                if op["bias"]:
                    z = z + params[v + "/conv_B"].view(1, -1, 1, 1)
                if op["act"] == "prelu":
                    z = F.dropout(torch.where(z > 0, z, params[v + "/prelu/" + op["name"] + "_prelu"].view(1, -1, 1, 1) * z), 0.2)
                elif op["act"]:
                    z = F.dropout(F.relu(z), 0.2)
                t[op["dst"]] = z
            elif op["op"] == "concat":
                t[op["dst"]] = torch.cat([t[s] for s in op["srcs"]], 1)
            elif op["op"] == "depth_to_space":
                t[op["dst"]] = F.pixel_shuffle(t[op["src"]], op["block"])
            elif op["op"] == "conv_transpose":
                wt, sc = params[op["var"] + "/Tconv_W"], op["scale"]
                t[op["dst"]] = F.conv_transpose2d(t[op["src"]], wt.permute(3, 2, 0, 1), stride=sc, padding=(wt.shape[0] - sc) // 2)
            elif op["op"] == "add":
                t[op["dst"]] = t[op["srcs"][0]] + t[op["srcs"][1]]
        loss = F.mse_loss(t["y_"], y) + 1e-4 * sum(0.5 * (wt * wt).sum() for wt in conv_w.values())
        opt.zero_grad(set_to_none=True)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(list(params.values()), 5.0)
        opt.step()

    return step


def bench_torch(cfg, n, h, w, steps, warmup):
    step = torch_step(cfg, n, h, w)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def bench_separable(name, n, size, steps, warmup):
    """The HIP step and the torch step of a separable (or transposed-conv) net, alternating step by step in one process, each between events on its stream."""
    cfg = O.make_config(**CONFIGS[name])
    eng = hip_engine(cfg)
    step = torch_step(cfg, n, size, size)
    x, x2, y = (torch.from_numpy(a).cuda() for a in batch(cfg, n, size, size))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    times = ([], [])
    for i in range(warmup + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        eng.train_step_device(x.data_ptr(), x2.data_ptr(), y.data_ptr(), n, size, size, 1e-4, i, stream=stream.cuda_stream, want_stats=False)
        b.record(stream)
        b.synchronize()
        c, d = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        c.record()
        step()
        d.record()
        d.synchronize()
        if i >= warmup:
            times[0].append(a.elapsed_time(b))
            times[1].append(c.elapsed_time(d))
    eng.close()
    hip, ref = float(np.median(times[0])), float(np.median(times[1]))
    return dict([("separable_compare" if cfg["depthwise_separable"] else "transposed_compare", name)], batch=n, lr_size=size, steps=steps, warmup=warmup, hip_ms_per_step=round(hip, 4),
                torch_ms_per_step=round(ref, 4), hip_over_torch=round(hip / ref, 4),
                min_ms=[round(float(np.min(times[0])), 4), round(float(np.min(times[1])), 4)])


def loop_model(name, n, size, tmp, augment_level=0):
    from dcscn_amd.model import SuperResolution
    from helper import args
    f = {k: args.FLAGS._flags[k].default for k in args.FLAGS}
    f.update(CONFIGS[name], self_ensemble=1, batch_num=n, batch_image_size=size, checkpoint_dir=tmp, log_filename="", train_augment_level=augment_level, **flags())
    m = SuperResolution(type("Flags", (dict,), {"__getattr__": dict.__getitem__})(f))
    m.build_graph()
    m.build_optimizer()
    m.load_weights(O.synthetic_weights(O.make_config(**CONFIGS[name]), seed=0))
    m.load_dynamic_datasets(os.path.join(ROOT, "tests", "golden", "set14"), size)
    m.init_train_step()
    m.init_epoch_index()
    return m


def host_batch(m):
    """build_input_batch before device batches: every patch cut and resized on the host."""
    for i in range(m.batch_num):
        m.batch_input[i], m.batch_input_bicubic[i], m.batch_true[i] = m.train.load_batch_image(m.max_value)


def bench_loop(name, n, size, steps, warmup, device_only):
    import random
    import tempfile
    import time
    random.seed(0)
    legs = {"device": lambda m: m.build_input_batch()}
    if not device_only:
        legs["host"] = host_batch
    with tempfile.TemporaryDirectory() as tmp:
        models = {k: loop_model(name, n, size, os.path.join(tmp, k)) for k in legs}
        times = {k: [] for k in legs}
        for i in range(warmup + steps):           # warm-up: every image decoded (and uploaded) at least once
            for k, draw in legs.items():
                t0 = time.perf_counter()
                draw(models[k])
                models[k].train_batch()           # returns after the step's stats are on the host
                if i >= warmup:
                    times[k].append((time.perf_counter() - t0) * 1e3)
        for m in models.values():
            m.close()
    out = dict(loop=name, batch=n, lr_size=size, steps=steps, warmup=warmup, device_batches_ms=round(float(np.median(times["device"])), 4))
    if not device_only:
        bare, _ = bench_hip(O.make_config(**CONFIGS[name]), n, size, size, steps, warmup)
        out.update(host_batches_ms=round(float(np.median(times["host"])), 4), bare_train_step_device_ms=round(bare, 4),
                   device_over_bare=round(out["device_batches_ms"] / bare, 3),
                   host_over_device=round(float(np.median(times["host"])) / out["device_batches_ms"], 2))
    return out


def bench_augment(name, n, size, steps, warmup, levels=(0, 8)):
    """build_input_batch() + train_batch() at every train_augment_level of `levels`, one model each, alternating step by step."""
    import random
    import tempfile
    import time
    random.seed(0)
    with tempfile.TemporaryDirectory() as tmp:
        models = [loop_model(name, n, size, os.path.join(tmp, str(level)), level) for level in levels]
        times = [[] for _ in levels]
        for i in range(warmup + steps):
            for k, m in enumerate(models):
                t0 = time.perf_counter()
                m.build_input_batch()
                m.train_batch()                   # returns after the step's stats are on the host
                if i >= warmup:
                    times[k].append((time.perf_counter() - t0) * 1e3)
        uploads = [len(m._device_images) for m in models]
        for m in models:
            m.close()
    med = [float(np.median(t)) for t in times]
    return dict(augment_compare=name, batch=n, lr_size=size, steps=steps, warmup=warmup, levels=list(levels), ms=[round(v, 4) for v in med],
                min_ms=[round(float(np.min(t)), 4) for t in times], ratio_to_first=[round(v / med[0], 4) for v in med], uploaded_images=uploads)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="L7_x2", choices=sorted(CONFIGS))
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--size", type=int, default=48)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch comparison (profiler runs)")
    ap.add_argument("--torch-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--loop", action="store_true", help="time build_input_batch() + train_batch() with host and device batches")
    ap.add_argument("--device-only", action="store_true", help="--loop: the device-batch leg only (profiler runs)")
    ap.add_argument("--split16", action="store_true", help="time train_split16 = 0 and 1 alternating in one process (L12 x2, c-DCSCN x2)")
    ap.add_argument("--train-split16", action="store_true", help="set option train_split16 on the timed handle")
    ap.add_argument("--split16-wgrad", action="store_true",
                    help="time (train_split16, train_split16_wgrad) = (0, 0), (1, 0), (1, 1) alternating in one process (L12 x2, c-DCSCN x2)")
    ap.add_argument("--train-split16-wgrad", action="store_true", help="set option train_split16_wgrad on the timed handle")
    ap.add_argument("--separable", action="store_true", help="time the separable nets' HIP step and torch step alternating in one process")
    ap.add_argument("--transposed", action="store_true", help="time the transposed-conv nets' HIP step and torch step alternating in one process")
    ap.add_argument("--optimizer", default="adam",
                    help="--optimizer of the timed handle; a comma-separated list times one handle each, alternating in one process")
    ap.add_argument("--augment", action="store_true", help="time the device-batch loop at train_augment_level 0 and 8 alternating in one process (c-DCSCN x2)")
    ap.add_argument("--library", help="load this libdcscn_hip.so instead of the tree's (e.g. one built from the parent commit)")
    a = ap.parse_args()
    if a.library:
        from dcscn_amd import build
        build.LIB_PATH = os.path.abspath(a.library)
    if "," in a.optimizer:
        print(json.dumps(bench_optimizers(a.config, a.optimizer.split(","), a.batch, a.size, a.steps, a.warmup)), flush=True)
        return
    if a.split16:
        for name in ("L12_x2", "L7_x2"):
            print(json.dumps(bench_split16(name, a.batch, a.size, a.steps, a.warmup)), flush=True)
        return
    if a.split16_wgrad:
        for name in ("L12_x2", "L7_x2"):
            print(json.dumps(bench_split16_wgrad(name, a.batch, a.size, a.steps, a.warmup)), flush=True)
        return
    if a.separable or a.transposed:
        for name, n, size in (SEPARABLE_CASES if a.separable else TRANSPOSED_CASES):
            print(json.dumps(bench_separable(name, n, size, a.steps, a.warmup)), flush=True)
        return
    if a.augment:
        print(json.dumps(bench_augment("L7_x2", a.batch, a.size, a.steps, a.warmup)), flush=True)
        return
    if a.loop:
        for name, n, size in LOOP_CASES:
            print(json.dumps(bench_loop(name, n, size, a.steps, a.warmup, a.device_only)), flush=True)
        return
    cfg = O.make_config(**CONFIGS[a.config])
    if a.torch_only:
        print(json.dumps({"torch_ms_per_step": bench_torch(cfg, a.batch, a.size, a.size, a.steps, a.warmup)}))
        return
    med, best = bench_hip(cfg, a.batch, a.size, a.size, a.steps, a.warmup, a.train_split16, a.train_split16_wgrad, a.optimizer)
    flops = step_flops(cfg, a.batch, a.size, a.size)
    out = dict(config=a.config, optimizer=a.optimizer, batch=a.batch, lr_size=a.size, steps=a.steps, warmup=a.warmup, ms_per_step=round(med, 4),
               ms_per_step_min=round(best, 4), conv_gflop_per_step=round(flops / 1e9, 3),
               conv_tflops=round(flops / (med * 1e-3) / 1e12, 3), fraction_of_f32_matrix_peak=round(flops / (med * 1e-3) / PEAK_F32_MATRIX, 4))
    if not a.no_torch:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--config", a.config, "--batch", str(a.batch), "--size", str(a.size),
                            "--steps", str(a.steps), "--warmup", str(a.warmup), "--torch-only"], capture_output=True, text=True, timeout=900)
        if p.returncode == 0:
            out.update(json.loads(p.stdout.strip().splitlines()[-1]))
        else:
            out["torch_error"] = (p.stderr or p.stdout).strip().splitlines()[-1:]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
