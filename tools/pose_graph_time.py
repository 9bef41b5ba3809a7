#!/usr/bin/env python3
"""Times of the pose-graph optimisation on the GPU, with the numpy/scipy reference of the tests beside them.

    python tools/pose_graph_time.py [--scenes sphere loop_closure large] [--no-reference] > profiles/pose_graph_time.log

Per scene: the whole 15-iteration run (slam_pg_optimize_host_f64, upload and download included), per LM trial (whole run /
trials) and per CG iteration (slope of slam_pg_pcg_f64 between 64 and 576 forced iterations: three launches, one product).
The product kernel's own duration is not separable from outside the library: tools/pose_graph_kernel_stats.py reads it
(pg_hmul_kernel<0>) from kernel traces of this script, one per graph.  HIP events on the context's stream, warm-up calls,
median of 7.  The reference is
tests/pose_graph_ref.py with scipy's sparse direct solve (SuperLU, one thread) on the same host, wall clock, one run.
No time here is a pass/fail criterion."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "slam-experiments_amd"), os.path.join(ROOT, "tests"), ROOT]

import numpy as np  # noqa: E402

import pose_graph_ref as R  # noqa: E402
import slamhip  # noqa: E402
from slamhip import pose_graph as pg  # noqa: E402


def median_ms(ctx, fn, reps=7, warm=2):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        ctx.sync()
        ctx.timer_start()
        fn()
        out.append(ctx.timer_stop())
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["sphere", "loop_closure", "large"])
    ap.add_argument("--no-reference", action="store_true")
    args = ap.parse_args()
    ctx = slamhip.default_context()
    makers = dict(R.SMALL_SCENES, large=R.large)
    print(f"# pose-graph optimisation, {slamhip.load().slam_version().decode()}; host threads: OMP_NUM_THREADS="
          f"{os.environ.get('OMP_NUM_THREADS', 'unset')}, reference = numpy + scipy spsolve (SuperLU, single-threaded)")
    for name in args.scenes:
        s = makers[name]()
        plan = pg.plan(s.V, s.E)
        print(f"\n== {name}: {s.V} poses, {s.E} edges; plan {plan}")
        P, st = pg.optimize_pose_graph(s.init, s.edges, s.meas, s.info, s.fixed, ctx=ctx)
        whole = median_ms(ctx, lambda: pg.optimize_pose_graph(s.init, s.edges, s.meas, s.info, s.fixed, ctx=ctx), warm=1)
        print(f"whole run (15 iterations): median {whole[0]:.3f} ms (min {whole[1]:.3f}, max {whole[2]:.3f}); stats {st}")
        print(f"per LM trial: {whole[0] / max(st['trials'], 1):.3f} ms ({st['trials']} trials, {st['cg_iterations']} CG iterations in all)")
        # CG iteration: device buffers, forced iteration counts (a tolerance that is never met)
        c, b, Hd, W, _ = pg.pose_graph_linearize(s.init, s.edges, s.meas, s.info, ctx=ctx)
        ptr, adj = pg.vertex_lists(s.V, s.edges)
        bufs = [ctx.upload(a) for a in (s.edges, ptr, adj, s.fixed, Hd, W, b)]
        de, dp, da, df, dH, dW, db = bufs
        dx = ctx.malloc(s.V * 48)
        hs = np.zeros(4)
        lam = 1e-6 * float(np.abs(Hd).max())

        def cg(n):
            slamhip._lib.check(ctx.lib.slam_pg_pcg_f64(ctx.handle, s.V, s.E, de.ptr, dp.ptr, da.ptr, df.ptr, dH.ptr, dW.ptr, db.ptr, lam, 1e-300,
                                                       n, dx.ptr, hs.ctypes.data))

        t64, t576 = median_ms(ctx, lambda: cg(64)), median_ms(ctx, lambda: cg(576))
        per_cg = (t576[0] - t64[0]) / 512
        print(f"slam_pg_pcg_f64 with 64 / 576 forced iterations: {t64[0]:.3f} / {t576[0]:.3f} ms -> {1e3 * per_cg:.2f} us per CG iteration "
              f"(3 launches; product traffic {576 * s.E / 1e6:.1f} MB -> {576 * s.E / max(per_cg, 1e-9) / 1e6:.1f} GB/s if the product were all of it)")
        dy = ctx.malloc(s.V * 48)
        one = median_ms(ctx, lambda: slamhip._lib.check(ctx.lib.slam_pg_hmul_f64(ctx.handle, s.V, s.E, de.ptr, dp.ptr, da.ptr, df.ptr, dH.ptr, dW.ptr,
                                                                                  lam, dx.ptr, dy.ptr)))
        print(f"slam_pg_hmul_f64 (checks + packing + one product + one read-back of the status): {one[0]:.3f} ms")
        for buf in bufs + [dx, dy]:
            buf.free()
        if not args.no_reference and name != "large":
            t = time.perf_counter()
            Pd, sd = R.optimize(s.init, s.edges, s.meas, s.info, s.fixed, solver="direct")
            dt = time.perf_counter() - t
            print(f"reference (direct solve), same host: {1e3 * dt:.1f} ms for {sd['trials']} trials = {1e3 * dt / sd['trials']:.1f} ms per trial; "
                  f"chi2 {sd['chi2_final']:.6f} against {st['chi2_final']:.6f} here; GPU/CPU = {whole[0] / (1e3 * dt):.4f}")
        elif name == "large":
            print("reference: not run at this size (its sparse factorisation takes minutes per trial)")


if __name__ == "__main__":
    main()
