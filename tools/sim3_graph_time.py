#!/usr/bin/env python3
"""Times of the Sim(3) pose-graph optimisation on the GPU.

    python tools/sim3_graph_time.py [--scenes drift_loop large] [--alt-lib PATH LABEL] > profiles/sim3_graph_time.log

One child process per figure (a fresh context, a fresh workspace), HIP events on the context's stream around warm calls,
median of 7.  Per scene: the whole 15-iteration run (slam_s3g_optimize_host_f64, upload and download included), per LM trial
(whole run / trials), per CG iteration (slope of slam_s3g_pcg_f64 between 64 and 576 forced iterations: three launches, one
product) and one slam_s3g_hmul_f64 call (checks + packing + one product + the status read-back; the product kernel's own
duration comes from a kernel trace of the hmul child: tools/pose_graph_kernel_stats.py --prefix=s3g).  On `large` also
slam_pg_optimize_host_f64 and the SE(3) CG slope on the same graph with every scale 1, in the same session, as context.
--alt-lib times the CG slope and the whole run of another build of the library on `large` (the slot-layout A/B).
No time here is a pass/fail criterion."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "slam-experiments_amd"), os.path.join(ROOT, "tests"), ROOT]


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


def child(figure, scene, lib):
    import numpy as np

    import slamhip
    from slamhip import _lib

    if lib:
        _lib.LIB_PATH = lib
    import pose_graph_ref as P
    import sim3_graph_ref as R
    from slamhip import pose_graph as pg
    from slamhip import sim3_graph as sg

    ctx = slamhip.default_context()
    se3 = figure.startswith("se3_")
    if se3:
        s = P.large() if scene == "large" else None
        n, lin, call, opt = 6, pg.pose_graph_linearize, ctx.lib.slam_pg_pcg_f64, pg.optimize_pose_graph
    else:
        s = R.large() if scene == "large" else R.SMALL_SCENES[scene]()
        n, lin, call, opt = 7, sg.sim3_graph_linearize, ctx.lib.slam_s3g_pcg_f64, sg.optimize_sim3_graph
    out = dict(figure=figure, scene=scene, V=s.V, E=s.E)
    if figure in ("whole", "se3_whole"):
        _, st = opt(s.init, s.edges, s.meas, s.info, s.fixed, ctx=ctx)
        t = median_ms(ctx, lambda: opt(s.init, s.edges, s.meas, s.info, s.fixed, ctx=ctx), warm=1)
        out.update(ms=t, stats={k: float(v) for k, v in st.items()}, plan=(pg if se3 else sg).plan(s.V, s.E))
    else:
        _, b, Hd, W, _ = lin(s.init, s.edges, s.meas, s.info, ctx=ctx)
        ptr, adj = pg.vertex_lists(s.V, s.edges)
        bufs = [ctx.upload(a) for a in (s.edges, ptr, adj, s.fixed, Hd, W, b)]
        de, dp, da, df, dH, dW, db = bufs
        dx, dy = ctx.malloc(s.V * 8 * n), ctx.malloc(s.V * 8 * n)
        hs = np.zeros(4)
        lam = 1e-6 * float(np.abs(Hd).max())
        if figure in ("cg", "se3_cg"):
            cg = lambda k: _lib.check(call(ctx.handle, s.V, s.E, de.ptr, dp.ptr, da.ptr, df.ptr, dH.ptr, dW.ptr, db.ptr, lam, 1e-300, k, dx.ptr,
                                           hs.ctypes.data))
            t64, t576 = median_ms(ctx, lambda: cg(64)), median_ms(ctx, lambda: cg(576))
            out.update(ms64=t64, ms576=t576, us_per_iteration=1e3 * (t576[0] - t64[0]) / 512)
        else:
            out.update(ms=median_ms(ctx, lambda: _lib.check(ctx.lib.slam_s3g_hmul_f64(ctx.handle, s.V, s.E, de.ptr, dp.ptr, da.ptr, df.ptr, dH.ptr,
                                                                                       dW.ptr, lam, dx.ptr, dy.ptr))))
    print("RESULT " + json.dumps(out), flush=True)


def figure(name, scene, lib=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", name, scene] + (["--lib", lib] if lib else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"{name} on {scene} failed ({r.returncode}):\n{r.stderr[-3000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def report(scene, label, lib, with_hmul=True):
    w = figure("whole", scene, lib)
    st = w["stats"]
    print(f"[{label}] plan {w['plan']}")
    print(f"[{label}] whole run (15 iterations): median {w['ms'][0]:.3f} ms (min {w['ms'][1]:.3f}, max {w['ms'][2]:.3f}); chi2 "
          f"{st['chi2_initial']:.6g} -> {st['chi2_final']:.6g}, {int(st['iterations'])} iterations, {int(st['trials'])} trials, "
          f"{int(st['cg_iterations'])} CG iterations, status {int(st['status'])}")
    print(f"[{label}] per LM trial: {w['ms'][0] / max(st['trials'], 1):.3f} ms")
    c = figure("cg", scene, lib)
    slot = w["plan"]["slot_row_doubles"] * 7 * 8
    traffic = 2 * c["E"] * slot
    print(f"[{label}] slam_s3g_pcg_f64 with 64 / 576 forced iterations: {c['ms64'][0]:.3f} / {c['ms576'][0]:.3f} ms -> "
          f"{c['us_per_iteration']:.2f} us per CG iteration (3 launches, one product; the product reads {traffic / 1e6:.1f} MB of slots -> "
          f"{traffic / max(c['us_per_iteration'], 1e-9) / 1e3:.1f} GB/s if the product were all of it)")
    if with_hmul:
        h = figure("hmul", scene, lib)
        print(f"[{label}] slam_s3g_hmul_f64 (checks + packing + one product + one read-back of the status): {h['ms'][0]:.3f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["drift_loop", "large"])
    ap.add_argument("--alt-lib", nargs=2, metavar=("PATH", "LABEL"))
    ap.add_argument("--child", nargs=2)
    ap.add_argument("--lib")
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1], args.lib)
    print("# Sim(3) pose-graph optimisation; HIP events, warm calls, median of 7, one process per figure")
    for scene in args.scenes:
        print(f"\n== {scene}")
        report(scene, "this build", None)
        if scene == "large":
            if args.alt_lib:
                report(scene, args.alt_lib[1], os.path.abspath(args.alt_lib[0]), with_hmul=False)
            w, c = figure("se3_whole", scene), figure("se3_cg", scene)
            st = w["stats"]
            print(f"[SE(3), slam_pg_*, the same graph with every scale 1] whole run: median {w['ms'][0]:.3f} ms; {int(st['iterations'])} iterations, "
                  f"{int(st['trials'])} trials, {int(st['cg_iterations'])} CG iterations -> {w['ms'][0] / max(st['trials'], 1):.3f} ms per trial; "
                  f"{c['us_per_iteration']:.2f} us per CG iteration ({576 * c['E'] / max(c['us_per_iteration'], 1e-9) / 1e3:.1f} GB/s of 6x6 slots)")


if __name__ == "__main__":
    main()
