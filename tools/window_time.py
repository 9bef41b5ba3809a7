"""Time of the window-constrained top-2 search (slam_bf_window_knn_u256) against the dense top-2 search (slam_bf_knn2_u256)
on the same rows, interleaved in ONE process; the median and the spread (min - max) over the rounds are reported.  Rows from
default_rng(228) (queries) and default_rng(229) (train), positions uniform on a square plane from default_rng(230).

    python tools/window_time.py [--rounds R] [NxM:plane:radius ...]

Per device shape (default 65536x65536:4096:16 and 1048576x1048576:8192:24), three numbers, all from HIP events around
back-to-back calls on device-resident rows:
  * window   the whole windowed search (bounds, binning, scans, search, decode);
  * top2     slam_bf_knn2_u256 with the shipped engine choice (matrix cores at these sizes);
  * valu     slam_bf_knn2_u256 on the VALU engine (slam_bf_set_engine(1)).
Then the frame-sized host call, 600 x 600 on a 640 x 480 plane at r = 32: window_match_arrays against knn_match_arrays(k=2),
wall clock per call (upload, search, download), interleaved call by call.  The split per kernel comes from a separate run
under rocprofv3 --kernel-trace --stats."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "slam-experiments_amd"), ROOT):
    sys.path.insert(0, p)

import slamhip  # noqa: E402


def opt(name, default):
    if name in sys.argv:
        i = sys.argv.index(name)
        v = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        return type(default)(v)
    return default


def spread(v):
    return f"{np.median(v) * 1e3:9.1f} us  [{min(v) * 1e3:8.1f} - {max(v) * 1e3:8.1f}]"


def rows(n, m, plane):
    q = np.random.default_rng(228).integers(0, 256, (n, 32), dtype=np.uint8)
    t = np.random.default_rng(229).integers(0, 256, (m, 32), dtype=np.uint8)
    g = np.random.default_rng(230)
    return q, t, g.uniform(0, plane, (n, 2)).astype(np.float32), g.uniform(0, plane, (m, 2)).astype(np.float32)


def time_shape(ctx, n, m, plane, radius, rounds):
    q, t, qxy, txy = rows(n, m, plane)
    dq, dt = slamhip.DeviceDescriptors(ctx, q), slamhip.DeviceDescriptors(ctx, t)
    dqxy, dtxy = ctx.malloc(n * 8).upload(qxy), ctx.malloc(m * 8).upload(txy)
    idx, dist = ctx.malloc(n * 8), ctx.malloc(n * 8)
    lib, h = ctx.lib, ctx.handle
    reps = max(1, min(20, int(4e10 // (n * m))))

    def window():
        ctx.timer_start()
        for _ in range(20):
            slamhip.window_knn_device(ctx, dq.buf, n, dt.buf, m, dqxy, dtxy, radius, 2, idx, dist)
        return ctx.timer_stop() / 20

    def top2(engine):
        ctx.set_engine(engine)
        try:
            ctx.timer_start()
            for _ in range(reps):
                assert lib.slam_bf_knn2_u256(h, dq.buf.ptr, n, dt.buf.ptr, m, 0, idx.ptr, dist.ptr) == 0, lib.slam_last_error()
            return ctx.timer_stop() / reps
        finally:
            ctx.set_engine(0)

    for _ in range(2):                                              # warm-up: allocations, code objects, clocks
        window()
        top2(0)
        top2(1)
    res = {"window": [], "top2": [], "valu": []}
    for _ in range(rounds):
        res["window"].append(window())
        res["top2"].append(top2(0))
        res["valu"].append(top2(1))
    slamhip.window_knn_device(ctx, dq.buf, n, dt.buf, m, dqxy, dtxy, radius, 2, idx, dist)
    found = (idx.download(np.int32, (n, 2))[:, 0] >= 0).mean()
    w = float(np.median(res["window"]))
    print(f"{n:>7} x {m:<7} plane {plane:g}^2 r={radius:g}: window {spread(res['window'])}   "
          f"top2 {spread(res['top2'])} (x{np.median(res['top2']) / w:6.1f})   "
          f"valu {spread(res['valu'])} (x{np.median(res['valu']) / w:6.1f})   queries with a neighbour {found:.3f}", flush=True)
    for o in (idx, dist, dqxy, dtxy, dq, dt):
        o.free()


def time_host(ctx, n=600, m=600, radius=32.0, calls=300):
    q, t, _, _ = rows(n, m, 1.0)
    g = np.random.default_rng(231)
    qxy = np.stack([g.uniform(0, 640, n), g.uniform(0, 480, n)], 1).astype(np.float32)
    txy = np.stack([g.uniform(0, 640, m), g.uniform(0, 480, m)], 1).astype(np.float32)
    fns = (("window", lambda: slamhip.window_match_arrays(q, t, qxy, txy, radius, 2, ctx=ctx)),
           ("top2", lambda: slamhip.knn_match_arrays(q, t, 2, ctx=ctx)))
    for _, fn in fns:
        for _ in range(30):
            fn()
    res = {name: [] for name, _ in fns}
    for _ in range(calls):                                          # interleaved call by call
        for name, fn in fns:
            t0 = time.perf_counter()
            fn()
            res[name].append((time.perf_counter() - t0) * 1e3)      # ms, as the device times above
    print(f"host call {n} x {m} (640 x 480, r={radius:g}): window_match_arrays {spread(res['window'])}, "
          f"knn_match_arrays(k=2) {spread(res['top2'])}", flush=True)


def main():
    rounds = opt("--rounds", 7)
    specs = sys.argv[1:] or ["65536x65536:4096:16", "1048576x1048576:8192:24"]
    ctx = slamhip.default_context()
    print(f"libslamhip {slamhip.load().slam_version().decode()}, {rounds} rounds, median [min - max] per call", flush=True)
    for s in specs:
        shape, plane, radius = s.split(":")
        n, m = (int(v) for v in shape.split("x"))
        time_shape(ctx, n, m, float(plane), float(radius), rounds)
    time_host(ctx)


if __name__ == "__main__":
    main()
