"""Summarise rocprofv3 --pmc passes over tools/run_search.py for a matrix-core top-2 kernel, per build (development aid).

    python tools/mx_counters.py [--kernel NAME] [--mfma-per-group K] LABEL=DIR[,DIR...] [LABEL=DIR[,DIR...] ...] > profiles/<name>.json

NAME: a substring of the kernel's name (default bf_top2_mx_kernel; bf_top2_mx32_kernel for the 32x32x64 kernel,
bf_mx32_image_top2_kernel for the same fed from the prepared image, bf_mx_image_kernel for the image's own launch).  K: the MFMAs
of a group-equivalent of 16 rows x 64 queries x 256 bits (default 8; 4 for the 32x32x64 kernel).

Each DIR is the output directory of one pass (`rocprofv3 --pmc <set> --output-format csv -d DIR -- python3
tools/run_search.py 65536x65536 20`, --pmc alone, SLAM_LIB choosing the build).  Per counter: the mean over the launches of
the sum over the dispatch's rows, and a few ratios the design document quotes."""
import csv
import glob
import json
import os
import sys
from collections import defaultdict

def opt(name, default):
    if name in sys.argv:
        i = sys.argv.index(name)
        v = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        return type(default)(v)
    return default


KERNEL, PER_GROUP = opt("--kernel", "bf_top2_mx_kernel"), opt("--mfma-per-group", 8)
out = {"kernel": KERNEL, "mfma_per_group": PER_GROUP, "per_launch": {}, "derived": {}}
for spec in sys.argv[1:]:
    label, dirs = spec.split("=")
    per = {}
    for d in dirs.split(","):
        for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            acc = defaultdict(float)
            with open(f, newline="") as fh:
                for row in csv.DictReader(fh):
                    if KERNEL in row["Kernel_Name"]:
                        acc[(row["Counter_Name"], row["Dispatch_Id"])] += float(row["Counter_Value"])
            vals = defaultdict(list)
            for (name, _), v in acc.items():
                vals[name].append(v)
            for name, v in vals.items():
                per[name] = {"value": sum(v) / len(v), "launches": len(v)}
    out["per_launch"][label] = per
    g = lambda n: per[n]["value"] if n in per else None
    dv = {}
    if g("SQ_WAVE_CYCLES"):
        for n in ("SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_VALU"):
            if g(n) is not None:
                dv[n + "_share_of_wave_cycles"] = g(n) / g("SQ_WAVE_CYCLES")
    if g("SQ_VALU_MFMA_BUSY_CYCLES") and g("SQ_VALU_MFMA_COEXEC_CYCLES") is not None:
        dv["coexec_share_of_mfma_busy"] = g("SQ_VALU_MFMA_COEXEC_CYCLES") / g("SQ_VALU_MFMA_BUSY_CYCLES")
    if g("SQ_INSTS_MFMA"):
        groups = g("SQ_INSTS_MFMA") / PER_GROUP
        if g("SQ_BUSY_CYCLES"):
            dv["SQ_BUSY_CYCLES_per_group_and_simd"] = g("SQ_BUSY_CYCLES") / groups      # see profiles/README.md for the scale
        for n in ("SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_LDS"):
            if g(n) is not None:
                dv[n + "_per_group"] = g(n) / groups      # SQ_INSTS_VALU counts the MFMAs too
    out["derived"][label] = dv
print(json.dumps(out, indent=1))
