"""Time of the radius search (slam_bf_radius_u256) against the top-2 search on the VALU engine (slam_bf_set_engine(1)) on the
same inputs, interleaved in ONE process; the median and the spread (min - max) over the rounds are reported.  Inputs: queries
from default_rng(228), train rows from default_rng(229), all on the device.

    python tools/radius_time.py [--rounds R] [--radii 64,96,104] [NxM ...]

Per shape and radius, three numbers:
  * count   the count kernel alone (HIP events around it: slam_prof_enable / slam_prof_read);
  * call    the whole call with the matches written (count, scan, read-back of the total, emit, sort: wall clock per call, the
            stream drained at the end; the capacity already fits, so it is one call);
  * top2    slam_bf_knn2_u256 on the VALU engine (HIP events around back-to-back searches).
Also the frame-sized host call at 200 x 200 (radius_match_arrays: upload, search, download) against knn_match_arrays(k=2).
The split per kernel comes from a separate run under rocprofv3 --kernel-trace --stats."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "slam-experiments_amd"), ROOT):
    sys.path.insert(0, p)

import slamhip  # noqa: E402

REPS = {4096 * 4096: 40, 8192 * 65536: 8, 65536 * 65536: 3}


def opt(name, default):
    if name in sys.argv:
        i = sys.argv.index(name)
        v = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        return type(default)(v)
    return default


def spread(v):
    return f"{np.median(v) * 1e3:9.1f} us  [{min(v) * 1e3:8.1f} - {max(v) * 1e3:8.1f}]"


def time_shape(ctx, n, m, radii, rounds):
    q = np.random.default_rng(228).integers(0, 256, (n, 32), dtype=np.uint8)
    t = np.random.default_rng(229).integers(0, 256, (m, 32), dtype=np.uint8)
    dq, dt = slamhip.DeviceDescriptors(ctx, q), slamhip.DeviceDescriptors(ctx, t)
    idx2, dist2 = ctx.malloc(n * 8), ctx.malloc(n * 8)
    off = ctx.malloc((n + 1) * 8)
    lib, h = ctx.lib, ctx.handle
    totals = {r: slamhip.radius_device(ctx, dq.buf, n, dt.buf, m, r, off, 0, None, None) for r in radii}
    cap = max(max(totals.values()), 1)
    ridx, rdist = ctx.malloc(cap * 4), ctx.malloc(cap * 4)
    reps = REPS.get(n * m, max(1, int(2e10 // (n * m))))

    def top2():
        ctx.timer_start()
        for _ in range(reps):
            assert lib.slam_bf_knn2_u256(h, dq.buf.ptr, n, dt.buf.ptr, m, 0, idx2.ptr, dist2.ptr) == 0, lib.slam_last_error()
        return ctx.timer_stop() / reps

    def radius(r):
        ctx.sync()
        ctx.prof_enable(True)
        t0 = time.perf_counter()
        for _ in range(reps):
            assert slamhip.radius_device(ctx, dq.buf, n, dt.buf, m, r, off, cap, ridx, rdist) == totals[r]
        ctx.sync()
        wall = (time.perf_counter() - t0) * 1e3 / reps
        launches, ms = ctx.prof_read()
        ctx.prof_enable(False)
        assert launches == reps
        return ms / reps, wall

    ctx.set_engine(1)
    try:
        for _ in range(2):                                          # warm-up: allocations, code objects, clocks
            top2()
            for r in radii:
                radius(r)
        t2 = []
        cnt = {r: [] for r in radii}
        call = {r: [] for r in radii}
        for _ in range(rounds):
            t2.append(top2())
            for r in radii:
                c, w = radius(r)
                cnt[r].append(c)
                call[r].append(w)
    finally:
        ctx.set_engine(0)
    assert ctx.state_dirty() == 0
    base = float(np.median(t2))
    print(f"{n:>6} x {m:<7} top2 (VALU)  {spread(t2)}", flush=True)
    for r in radii:
        frac = totals[r] / (float(n) * m)
        print(f"{n:>6} x {m:<7} r={r:<5g} count {spread(cnt[r])}  x top2 {np.median(cnt[r]) / base:5.2f}   "
              f"call {spread(call[r])}  x top2 {np.median(call[r]) / base:5.2f}   matches {totals[r]} ({frac:.2e} of pairs)",
              flush=True)
    for o in (idx2, dist2, off, ridx, rdist, dq, dt):
        o.free()


def time_host(ctx, r, calls=200):
    q = np.random.default_rng(228).integers(0, 256, (200, 32), dtype=np.uint8)
    t = np.random.default_rng(229).integers(0, 256, (200, 32), dtype=np.uint8)
    res = {}
    for name, fn in (("radius", lambda: slamhip.radius_match_arrays(q, t, r, ctx=ctx)),
                     ("top2", lambda: slamhip.knn_match_arrays(q, t, 2, ctx=ctx))):
        for _ in range(20):
            fn()
        dt = []
        for _ in range(calls):
            t0 = time.perf_counter()
            fn()
            dt.append((time.perf_counter() - t0) * 1e3)              # ms, as the device times above
        res[name] = dt
    print(f"host call 200 x 200 r={r:g}: radius_match_arrays {spread(res['radius'])}, knn_match_arrays(k=2) {spread(res['top2'])}",
          flush=True)


def main():
    rounds = opt("--rounds", 7)
    radii = [float(v) for v in opt("--radii", "64,96,104").split(",")]
    shapes = [tuple(int(v) for v in a.split("x")) for a in sys.argv[1:]] or [(65536, 65536), (8192, 65536)]
    ctx = slamhip.default_context()
    print(f"libslamhip {slamhip.load().slam_version().decode()}, {rounds} rounds, median [min - max] per call", flush=True)
    for n, m in shapes:
        time_shape(ctx, n, m, radii, rounds)
    for r in (64.0, 96.0):
        time_host(ctx, r)


if __name__ == "__main__":
    main()
