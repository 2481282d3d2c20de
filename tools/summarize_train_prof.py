"""Group the kernel statistics of a `rocprofv3 --kernel-trace --stats` run of tools/train_bench.py by training phase.

    python tools/summarize_train_prof.py <rocprofv3 output dir> <steps profiled (warm-up + timed)>

Phases: forward (tconv_gemm<0>, tact_fwd, td2s), dgrad (tconv_gemm<1>, tpack_dgrad), wgrad (tconv_wgrad, treduce_wgrad,
tcol_*, tact_bwd), loss (tloss, tsumsq, tstats), optimizer (topt, tpowers).  td2s runs in both directions and is counted
with the forward; tact_bwd (the activator and dropout backward) is counted with the weight gradient it feeds.  With option
"train_split16" the eligible layers' convs are tconv_gemm_h<0> (forward) and tconv_gemm_h<1> (dgrad); what the option adds beside
them -- tabsmax_part, texp_final, tpack_h -- is the phase "scale_pack".  With option "train_split16_wgrad" the eligible layers' weight
gradients are tconv_wgrad_h<taps> (phase wgrad, like tconv_wgrad), and its exponent reductions count with "scale_pack".  "conv_kernels" lists the conv launches by kernel.
Separable nets (option "train_separable"): tdw_fwd, tdw_dgrad and tdw_wgrad count with the forward, dgrad and wgrad phases; a separable
layer's dd = dz . P^T runs on tconv_gemm<0> and so counts with the forward.
Transposed-conv nets (option "train_transposed"): tup_fwd, tup_dgrad and tup_wgrad (layer Up-TCNN) count with the forward, dgrad and wgrad
phases and are listed with the conv launches.
"""
import csv
import glob
import json
import os
import sys

PHASES = [("dgrad", ("tconv_gemmILi1E", "tconv_gemm<1>", "tconv_gemm_hILi1E", "tconv_gemm_h<1>", "tpack_dgrad", "tdw_dgrad", "tup_dgrad")),
          ("forward", ("tconv_gemmILi0E", "tconv_gemm<0>", "tconv_gemm_hILi0E", "tconv_gemm_h<0>", "tact_fwd", "td2s", "tdw_fwd", "tup_fwd")),
          ("scale_pack", ("tabsmax_part", "texp_final", "tpack_h")),
          ("wgrad", ("tconv_wgrad", "tdw_wgrad", "tup_wgrad", "treduce_wgrad", "tcol_partial", "tcol_final", "tact_bwd")),
          ("loss", ("tloss", "tsumsq", "tstats")), ("optimizer", ("topt", "tpowers"))]


def main():
    root, steps = sys.argv[1], int(sys.argv[2])
    files = glob.glob(os.path.join(root, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        sys.exit("no *kernel_stats.csv under %s" % root)
    ms = {p: 0.0 for p, _ in PHASES}
    other = 0.0
    convs = {}
    for f in files:
        with open(f) as fh:
            for row in csv.DictReader(fh):
                name, total_ns = row["Name"], float(row["TotalDurationNs"])
                if "tconv_" in name or "tup_" in name:
                    convs[name] = round(convs.get(name, 0.0) + total_ns / 1e6 / steps, 4)
                for phase, keys in PHASES:
                    if any(k in name for k in keys):
                        ms[phase] += total_ns / 1e6
                        break
                else:
                    other += total_ns / 1e6
    per_step = {p: round(v / steps, 4) for p, v in ms.items()}
    per_step["not_training"] = round(other / steps, 4)
    per_step["kernel_sum"] = round(sum(ms.values()) / steps, 4)
    print(json.dumps({"ms_per_step_by_phase": per_step, "conv_kernels": convs, "steps": steps, "files": [os.path.relpath(f, root) for f in files]}))


if __name__ == "__main__":
    main()
