"""Time of the Sim(3) refinement (slam_sim3_optimize_f64), from HIP events (slam_timer_start/stop) around back-to-back calls
on device-resident arrays, after a warm launch; the median and the spread (min - max) of 7 rounds are reported.

    python tools/sim3_opt_time.py [--rounds R] > profiles/sim3_opt_time.log

  * batch      1 / 16 / 256 / 4096 candidates x 200 pairs (1 px noise, 30 % planted outliers, the start moved by about
               0.005 rad / 0.01 m / 0.02 in log scale), per call and per candidate, with the mean accepted steps (d_stats) and
               the mean trials and linearisations per candidate (counted by the host twin on the first 16 candidates);
  * host       beside each: one host core on the same candidates - the numpy statement (tests/sim3_opt_ref.py) and the host
               build of the kernel file's own routines (tests/sim3_opt_twin.py, plain C++ at -O2), both on the first 16
               candidates at most, per candidate;
  * context    slam_sim3_ransac_f64 (H = 256) + slam_sim3_refit_f64 on the same shapes in the same session;
  * paths      one candidate of 512 pairs (kept in LDS) against one of 600 (the same code on the global arrays).
The values are a record, not a gate."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "slam-experiments_amd"), os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)

import slamhip  # noqa: E402
import sim3_opt_ref as ref  # noqa: E402
import sim3_opt_twin as tw  # noqa: E402

K = ref.EUROC
ARGS = (10.0, 5, 10, 5, 10, 0)
HOST = 16


def opt(name, default):
    if name in sys.argv:
        i = sys.argv.index(name)
        v = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        return type(default)(v)
    return default


def spread(v):
    return f"{np.median(v) * 1e3:10.1f} us  [{min(v) * 1e3:9.1f} - {max(v) * 1e3:9.1f}]"


def main():
    rounds = opt("--rounds", 7)
    ctx = slamhip.default_context()
    lib, h = ctx.lib, ctx.handle
    rng = np.random.default_rng(4242)

    def timed(fn):
        ctx.timer_start()
        fn()
        return ctx.timer_stop()

    def run(call):
        timed(call)
        return [timed(call) for _ in range(rounds)]

    def problem(B, n):
        base = [ref.make_scene(rng, n, 1.2, 1.0, 0.3) for _ in range(min(B, 64))]
        starts = [ref.moved(rng, s["model"]) for s in base]
        sc = [base[b % len(base)] for b in range(B)]                    # (beyond 64 the scenes repeat: the device cannot tell)
        cat = lambda k: np.concatenate([s[k] for s in sc])
        return sc, np.stack([starts[b % len(base)] for b in range(B)]), cat

    def device(B, n, label):
        sc, starts, cat = problem(B, n)
        M = B * n
        off = np.arange(B + 1, dtype=np.int32) * n
        bufs = [ctx.upload(a) for a in (cat("X1"), cat("X2"), cat("px1"), cat("px2"), off, starts)]
        d1, d2, dp1, dp2, do, dz = bufs
        outs = [ctx.malloc(B * 104), ctx.malloc(M), ctx.malloc(M * 16), ctx.malloc(B * 16), ctx.malloc(B * 104), ctx.malloc(B * 8)]
        dT, dm, dc, ds, dT2, ds2 = outs

        def call():
            assert lib.slam_sim3_optimize_f64(h, B, do.ptr, d1.ptr, d2.ptr, dp1.ptr, dp2.ptr, M, None, dz.ptr, *K, *ARGS, dT.ptr, dm.ptr, dc.ptr,
                                              ds.ptr) == 0

        def ransac():
            assert lib.slam_sim3_ransac_f64(h, B, do.ptr, d1.ptr, d2.ptr, M, None, *K, 256, 9.210, 0, 0, dT.ptr, dm.ptr, ds.ptr) == 0
            assert lib.slam_sim3_refit_f64(h, B, do.ptr, d1.ptr, d2.ptr, M, dm.ptr, 0, dT2.ptr, ds2.ptr) == 0

        v = run(call)
        st = ds.download(np.int32, (B, 4))
        k = min(B, HOST)
        t0 = time.perf_counter()
        work = np.array([tw.optimize(s["X1"], s["X2"], s["px1"], s["px2"], m, K, with_work=True)[4] for s, m in zip(sc[:k], starts[:k])])
        t1 = time.perf_counter()
        for s, m in zip(sc[:k], starts[:k]):
            ref.optimize(s, m)
        t2 = time.perf_counter()
        print(f"{label} B = {B:5d} x {n:3d}: {spread(v)}  {np.median(v) * 1e3 / B:9.2f} us / candidate | inliers {st[:, 0].mean():6.1f} steps "
              f"{st[:, 1].mean():5.1f} trials {work[:, 0].mean():5.1f} linearisations {work[:, 1].mean():5.1f} | one host core: C++ "
              f"{(t1 - t0) / k * 1e6:8.1f} us, numpy {(t2 - t1) / k * 1e6:9.1f} us / candidate")
        if label == "batch":
            v = run(ransac)
            print(f"context B = {B:5d} x {n:3d}: {spread(v)}  {np.median(v) * 1e3 / B:9.2f} us / candidate  (slam_sim3_ransac_f64 H = 256 + slam_sim3_refit_f64)")
        for o in bufs + outs:
            o.free()

    print(slamhip.load().slam_version().decode())
    tw.lib()
    for B in (1, 16, 256, 4096):
        device(B, 200, "batch")
    device(1, 512, "lds   ")
    device(1, 600, "global")


if __name__ == "__main__":
    main()
