"""Step time of data-parallel training (dcscn_train_local_gradients_device + dcscn_train_apply_records) of the L12 x2 net.

    python tools/train_parallel_bench.py [--share-gpu-ranks 2]

Prints one JSON line per leg, median over --steps after --warmup (50 after 10, as DESIGN.md section 8 measures training):

* world = 1, always: the split path (local_gradients, then apply_records with world = 1) beside dcscn_train_step_device on the same
  20 x 48^2 batch, two handles alternating step by step in one process, each step between HIP events on its stream.
* world = 2, 4, 8, where the machine has that many GPUs: one rank per GPU under torch.distributed.run, records exchanged over RCCL
  (shard.Group.all_gather_records); "strong" splits the 20 x 48^2 batch over the ranks, "weak" gives every rank 20 x 48^2.  A step
  is timed on the host clock from a barrier to the return of apply_records with its stats (a device synchronise); the figure is
  the slowest rank's median.  A world the machine has too few GPUs for is reported as not measured, never emulated.
* --share-gpu-ranks N: N ranks on device 0 over gloo (the test rig's path, records through host memory).  The ranks contend for one
  GPU: this is the cost of the plumbing, not a speed-up measurement.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dcscn_oracle as O  # noqa: E402
from train_bench import CONFIGS, batch, flags  # noqa: E402

NET, BATCH, SIZE = "L12_x2", 20, 48


def _engine(cfg, device=0):
    from dcscn_amd import engine
    eng = engine.Engine(cfg, device=device)
    eng.load_weights(O.synthetic_weights(cfg, seed=0))
    eng.train_begin(flags())
    return eng


def world_one(steps, warmup):
    cfg = O.make_config(**CONFIGS[NET])
    step_eng, split_eng = _engine(cfg), _engine(cfg)
    x, x2, y = (torch.from_numpy(a).cuda() for a in batch(cfg, BATCH, SIZE, SIZE))
    record = torch.zeros(split_eng.train_record_floats(), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    args = (x.data_ptr(), x2.data_ptr(), y.data_ptr(), BATCH, SIZE, SIZE)

    def whole(i):
        step_eng.train_step_device(*args, 1e-4, i, stream=sp, want_stats=False)

    def split(i):
        split_eng.train_local_gradients_device(*args, record.data_ptr(), dropout_key=i, first_index=0, stream=sp)
        split_eng.train_apply_records(record.data_ptr(), 1, 1e-4, stream=sp, want_stats=False)

    times = {"train_step_device": [], "split": []}
    for i in range(warmup + steps):
        for name, fn in (("train_step_device", whole), ("split", split)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn(i)
            b.record(stream)
            b.synchronize()
            if i >= warmup:
                times[name].append(a.elapsed_time(b))
    same = all(np.array_equal(step_eng.get_tensor(k), split_eng.get_tensor(k)) for k, _ in step_eng.tensor_specs())
    step_eng.close()
    split_eng.close()
    whole_ms, split_ms = float(np.median(times["train_step_device"])), float(np.median(times["split"]))
    return dict(leg="world1", net=NET, batch=BATCH, lr_size=SIZE, steps=steps, warmup=warmup, train_step_device_ms=round(whole_ms, 4),
                split_path_ms=round(split_ms, 4), split_minus_step_ms=round(split_ms - whole_ms, 4),
                split_over_step=round(split_ms / whole_ms, 4), record_mb=round(record.numel() * 4 / 1e6, 3),
                variables_bit_identical_after_run=bool(same))


def worker(scaling, steps, warmup):
    """One rank of a multi-rank leg (under torch.distributed.run)."""
    from dcscn_amd import shard
    group = shard.init_from_env()
    cfg = O.make_config(**CONFIGS[NET])
    total = BATCH if scaling == "strong" else BATCH * group.world
    begin, end = shard.train_shard(total, group.rank, group.world)
    n = end - begin
    device = torch.device("cuda", group.local_rank)
    eng = _engine(cfg, device=group.local_rank)
    with torch.cuda.device(device):
        x, x2, y = (torch.from_numpy(a).to(device) for a in batch(cfg, n, SIZE, SIZE))
        record = torch.zeros(eng.train_record_floats(), dtype=torch.float32, device=device)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream(device=device)
        times, gather = [], []
        with torch.cuda.stream(stream):
            for i in range(warmup + steps):
                group.barrier()
                t0 = time.perf_counter()
                eng.train_local_gradients_device(x.data_ptr(), x2.data_ptr(), y.data_ptr(), n, SIZE, SIZE, record.data_ptr(), dropout_key=i,
                                                 first_index=begin, stream=stream.cuda_stream)
                stream.synchronize()
                t1 = time.perf_counter()
                records = group.all_gather_records(record)
                stream.synchronize()
                t2 = time.perf_counter()
                eng.train_apply_records(records.data_ptr(), group.world, 1e-4, stream=stream.cuda_stream)      # returns with the stats
                t3 = time.perf_counter()
                if i >= warmup:
                    times.append((t3 - t0) * 1e3)
                    gather.append((t2 - t1) * 1e3)
    every = group.gather([(float(np.median(times)), float(np.median(gather)))])
    if group.rank == 0:
        print(json.dumps(dict(leg="world%d" % group.world, scaling=scaling, net=NET, global_batch=total, patches_per_rank=n, lr_size=SIZE,
                              steps=steps, warmup=warmup, step_ms_slowest_rank=round(max(t for t, _ in every), 4),
                              all_gather_ms_slowest_rank=round(max(g for _, g in every), 4),
                              exchange="gloo through host memory, ranks share device 0" if os.environ.get("DCSCN_SHARE_GPU") == "1"
                              else "RCCL, one GPU per rank")), flush=True)
    eng.close()
    group.close()


def launch(world, scaling, steps, warmup, port, share):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    if share:
        env.update(DCSCN_SHARE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__), "--worker", scaling, "--steps", str(steps), "--warmup", str(warmup)]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or len(lines) != 1:
        raise RuntimeError("the %d-rank %s leg failed (%d):\n%s" % (world, scaling, p.returncode, (p.stdout + p.stderr)[-3000:]))
    print(lines[0], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--share-gpu-ranks", type=int, default=0, help="also run this many ranks on device 0 over gloo (plumbing cost only)")
    ap.add_argument("--port", type=int, default=29671)
    ap.add_argument("--worker", choices=("strong", "weak"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(a.worker, a.steps, a.warmup)
        return
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    gpus = torch.cuda.device_count()
    print(json.dumps(world_one(a.steps, a.warmup)), flush=True)
    port = a.port
    for world in (2, 4, 8):
        if gpus < world:
            print(json.dumps(dict(leg="world%d" % world, not_measured="the machine has %d GPU(s)" % gpus)), flush=True)
            continue
        for scaling in ("strong", "weak"):
            launch(world, scaling, a.steps, a.warmup, port, share=False)
            port += 1
    if a.share_gpu_ranks > 1:
        for scaling in ("strong", "weak"):
            launch(a.share_gpu_ranks, scaling, a.steps, a.warmup, port, share=True)
            port += 1


if __name__ == "__main__":
    main()
