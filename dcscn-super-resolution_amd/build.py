"""Builds libdcscn_hip.so (the C ABI of include/dcscn.h) in-tree with hipcc for gfx950.

hipcc cross-compiles without a GPU, so this runs in the build container; the resulting .so sits next
to this file and travels to the GPU box with the source tree.
"""

import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG_DIR, "csrc")
INCLUDE = os.path.join(os.path.dirname(PKG_DIR), "include")
LIB_NAME = "libdcscn_hip.so"
LIB_PATH = os.path.join(PKG_DIR, LIB_NAME)
HEADERS = [os.path.join(CSRC, h) for h in sorted(os.listdir(CSRC)) if h.endswith((".h", ".hpp"))] + [os.path.join(INCLUDE, "dcscn.h")]
ARCH = "gfx950"
# No packed-f32 VALU instructions (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32) in any kernel: beside ANOTHER process's MFMA work on
# the same SIMD their low-half results come back wrong in lanes 48-63 (tools/xproc_triage.hip: victim cin1p vs cin1s next to
# aggressor mfma).  They also issue worse next to MFMAs (MI355X_MICROARCH.md), so nothing is lost.  The feature flag is
# passed to the host compilation as well, which reports it as unknown and ignores it (filtered from the output below).
NO_PK_F32 = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
FLAGS = ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"] + NO_PK_F32
# -fno-slp-vectorize: see the comment at the top of conv_wino2.hip; the resource-usage remarks feed the spill gate of _run
NO_SLP = ["-fno-slp-vectorize"]
KERNEL = NO_SLP + ["-Rpass-analysis=kernel-resource-usage"]
NO_CONTRACT = ["-ffp-contract=off"]
# train.hip: the remarks alone (they change no code), so that the spill gate covers its MFMA kernels (train_kernels.hpp, train_tconv.hpp)
REMARKS = ["-Rpass-analysis=kernel-resource-usage"]
# source: (extra flags, must not spill).  Must not spill: kernels that sit at the VGPR limit by design (192 accumulators + operands) -- a
# register spill inside their K loop also breaks the hand-counted vmcnt accounting of the LDS-DMA pipeline, so a build that spills is
# rejected, not shipped
SOURCE_TABLE = {
    "api.hip": ([], False), "graph.hip": ([], False), "pack.hip": ([], False), "exec.hip": ([], False), "kernels.hip": ([], False),
    "resample.hip": ([], False), "ensemble.hip": ([], False), "color.hip": (NO_CONTRACT, False), "metrics.hip": (NO_CONTRACT, False),
    "conv_k1.hip": ([], False), "conv_k3.hip": ([], False), "conv_k5.hip": ([], False), "conv_k7.hip": ([], False),
    "conv_wino2.hip": (KERNEL, True), "conv_nin.hip": (KERNEL, True), "feat_stream.hip": (KERNEL, True),
    "conv_nin_h.hip": (KERNEL, True), "conv_nin_h_w8.hip": (KERNEL, True), "conv3_h.hip": (KERNEL, True), "conv3_h8.hip": (KERNEL, True),
    "conv5_h.hip": (KERNEL, True), "conv3_h_p16.hip": (KERNEL, True), "conv3_h8_p16.hip": (KERNEL, True),
    "conv3_h_fast16.hip": (KERNEL, True), "conv3_h8_fast16.hip": (KERNEL, True), "conv_nin_h_fast16.hip": (KERNEL, True),
    "conv5_h_fast16.hip": (KERNEL, True), "feat_stream_redo.hip": (NO_SLP, False), "feat3_stream.hip": (KERNEL, True),
    "feat3_stream_fast16.hip": (KERNEL, True), "feat_stream_fast16.hip": (KERNEL, True),
    "train.hip": (REMARKS, True), "train_data.hip": ([], False), "train_h.hip": (KERNEL, True),
    "train_wgrad_h.hip": (KERNEL, True), "summary.hip": (NO_CONTRACT, False),
}
SOURCES = list(SOURCE_TABLE)
EXTRA_FLAGS = {src: flags for src, (flags, _) in SOURCE_TABLE.items()}
NO_SCRATCH = tuple(src for src, (_, no_spill) in SOURCE_TABLE.items() if no_spill)


def hipcc_path():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.isfile(cand):
            return cand
    raise RuntimeError("hipcc not found; the DCSCN HIP extension cannot be built")


def _stale(target, deps):
    if not os.path.isfile(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _run(cmd):
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    proc.stdout = "\n".join(ln for ln in proc.stdout.splitlines() if "'-packed-fp32-ops' is not a recognized feature" not in ln)
    if proc.returncode != 0:
        raise RuntimeError("command failed (%d): %s\n%s" % (proc.returncode, " ".join(cmd), proc.stdout))
    if any(cmd[-3].endswith(n) for n in NO_SCRATCH if len(cmd) >= 3):
        import re
        bad = [ln for ln in proc.stdout.splitlines() if re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill): [1-9]", ln)]
        if bad:
            os.remove(cmd[-1])
            raise RuntimeError("register spill in a kernel that must not spill (%s):\n%s" % (cmd[-3], "\n".join(bad[:6])))
        return ""
    return proc.stdout


def build(force=False, verbose=False):
    """Compile every HIP source for gfx950 and link libdcscn_hip.so. Returns the library path."""
    hipcc = hipcc_path()
    obj_dir = os.path.join(PKG_DIR, "build")
    os.makedirs(obj_dir, exist_ok=True)
    jobs = []
    objs = []
    for src in SOURCES:
        src_path = os.path.join(CSRC, src)
        obj = os.path.join(obj_dir, os.path.splitext(src)[0] + ".o")
        objs.append(obj)
        if force or _stale(obj, [src_path, os.path.abspath(__file__)] + HEADERS):       # (a change of the flag lists in this file rebuilds everything)
            jobs.append([hipcc] + FLAGS + EXTRA_FLAGS.get(src, []) + ["-I", INCLUDE, "-c", src_path, "-o", obj])
    if jobs:
        with ThreadPoolExecutor(max_workers=len(jobs)) as pool:
            for out in pool.map(_run, jobs):
                if verbose and out.strip():
                    print(out, file=sys.stderr)
    if jobs or force or _stale(LIB_PATH, objs):
        out = _run([hipcc, "--offload-arch=" + ARCH, "-shared", "-fPIC"] + objs + ["-o", LIB_PATH])
        if verbose and out.strip():
            print(out, file=sys.stderr)
    return LIB_PATH


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
