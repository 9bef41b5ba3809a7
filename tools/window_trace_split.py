"""Per-call split of the window search from a rocprofv3 kernel trace of tools/window_time.py: the calls are cut at
win_bounds_kernel / win_decode_kernel and grouped by the decode grid (N rounded up to 256); per group the median span of a
call (first start to last end), the median busy time (sum of kernel durations) and each kernel's median duration.

    rocprofv3 --kernel-trace --stats -d OUT -o win -- python tools/window_time.py --rounds 1
    python tools/window_trace_split.py OUT/win_results.db"""
import collections
import re
import sqlite3
import sys

import numpy as np


def main(db):
    rows = sqlite3.connect(db).execute("select name, start, end, grid_x from kernels order by start").fetchall()
    calls, cur = [], None
    for name, s, e, gx in rows:
        short = re.sub(r"\(.*", "", name).replace("void ", "")
        if "win_bounds_kernel" in short:
            cur = []
        if cur is not None:
            cur.append((short, s, e, gx))
            if "win_decode_kernel" in short:
                calls.append(cur)
                cur = None
    groups = collections.defaultdict(list)
    for c in calls:
        groups[c[-1][3]].append(c)
    for n, cs in groups.items():
        span = np.median([(c[-1][2] - c[0][1]) / 1e3 for c in cs])
        busy = np.median([sum(e - s for _, s, e, _ in c) / 1e3 for c in cs])
        print(f"N <= {n}: {len(cs)} calls, span {span:.1f} us, kernels {busy:.1f} us, {len(cs[0])} launches")
        per = collections.defaultdict(list)
        for c in cs:
            seen = collections.Counter()
            for k, s, e, _ in c:
                seen[k] += 1
                per[(k, seen[k])].append((e - s) / 1e3)
        for (k, _), v in per.items():
            print(f"    {k:32s} {np.median(v):8.1f} us")


if __name__ == "__main__":
    main(sys.argv[1])
