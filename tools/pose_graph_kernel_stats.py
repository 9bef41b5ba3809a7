#!/usr/bin/env python3
"""Durations of the SE(3) pose-graph kernels (csrc/graph_lm.h instantiated with pg_se3: glm_hmul_kernel<pg_se3, 1>, ...) from
kernel traces of tools/pose_graph_time.py, one trace per graph:

    for s in sphere loop_closure large; do
        rocprofv3 --kernel-trace -d trace_$s -o pg -- python tools/pose_graph_time.py --scenes $s --no-reference
    done
    python tools/pose_graph_kernel_stats.py sphere=trace_sphere loop_closure=trace_loop_closure large=trace_large \\
        > profiles/pose_graph_kernel_stats.txt

Reads the `kernels` view of the trace databases (*_results.db) and prints, per graph and kernel: calls, average / min / max
duration in microseconds.  The kernels are told apart by the traits type in their name: `pg_` matches pg_se3.  A first argument
--prefix=s3g reads the Sim(3) instantiations (s3g_sim3) from tools/sim3_graph_time.py's children instead
(rocprofv3 --kernel-trace -d DIR -o s3g -- python tools/sim3_graph_time.py --child hmul large).  glm_hmul_kernel<M, 0> is the
product alone (the calls of slam_*_hmul_f64 the timing scripts make); glm_hmul_kernel<M, 1> and the two CG vector kernels include
the launches that return at once after convergence."""
import glob
import os
import sqlite3
import sys


def main():
    args, prefix = sys.argv[1:], "pg"
    if args and args[0].startswith("--prefix="):
        prefix, args = args[0][9:], args[1:]
    script = "tools/pose_graph_time.py --scenes NAME --no-reference" if prefix == "pg" else "tools/sim3_graph_time.py --child FIGURE NAME"
    print(f"# durations of the glm_*<{prefix}_...> kernels (rocprofv3 --kernel-trace of {script})")
    print("# calls, average / min / max in us, kernel")
    for arg in args:
        label, _, where = arg.partition("=")
        dbs = sorted(glob.glob(os.path.join(where, "**", "*_results.db"), recursive=True))
        if not dbs:
            raise SystemExit(f"no *_results.db under {where}")
        db = sqlite3.connect(dbs[-1])
        print(f"\n== {label}")
        rows = db.execute("select name, count(*), avg(duration), min(duration), max(duration) from kernels "
                          f"where name like '%{prefix}\\_%' escape '\\' group by name order by sum(duration) desc")
        for name, calls, avg, lo, hi in rows:
            print(f"{calls:7d} {avg / 1e3:9.2f} {lo / 1e3:9.2f} {hi / 1e3:9.2f}  {name.split('(')[0].replace('void ', '')}")


if __name__ == "__main__":
    main()
