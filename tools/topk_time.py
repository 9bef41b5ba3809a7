"""Device time of the top-k search (slam_bf_knn_u256) at K = 4, 8, 16, 32 against the top-2 search (slam_bf_knn2_u256) on
the same inputs, interleaved in ONE process: per round, every variant runs `reps` back-to-back searches between two HIP
events; the median over the rounds is reported.  Inputs: queries from default_rng(228), train rows from default_rng(229).

    python tools/topk_time.py [--rounds R] [NxM ...]

Also reported: the frame-sized host call (200 x 200, k = 3 and k = 8, wall clock per call) and the 16-thread C oracle
(oracle.bf_knn_c, the CPU port of OpenCV's K-best insertion) at 4096 x 4096.  "floor" is the fraction of the 16-VALU-per-pair
bound of the whole chip (bench.py's VALU_LANES_PER_S and OPS_PER_PAIR)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "slam-experiments_amd"), ROOT):
    sys.path.insert(0, p)

from bench import OPS_PER_PAIR, VALU_LANES_PER_S  # noqa: E402
import slamhip  # noqa: E402
from oracle import oracle  # noqa: E402

REPS = {4096 * 4096: 40, 8192 * 65536: 8, 65536 * 65536: 3, 4096 * (1 << 20): 3}


def opt(name, default):
    if name in sys.argv:
        i = sys.argv.index(name)
        v = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        return type(default)(v)
    return default


def time_shape(ctx, n, m, rounds):
    q = np.random.default_rng(228).integers(0, 256, (n, 32), dtype=np.uint8)
    t = np.random.default_rng(229).integers(0, 256, (m, 32), dtype=np.uint8)
    dq, dt = slamhip.DeviceDescriptors(ctx, q), slamhip.DeviceDescriptors(ctx, t)
    idx, dist = ctx.malloc(n * 32 * 4), ctx.malloc(n * 32 * 4)
    lib, h = ctx.lib, ctx.handle
    variants = [("top2", lambda: lib.slam_bf_knn2_u256(h, dq.buf.ptr, n, dt.buf.ptr, m, 0, idx.ptr, dist.ptr))]
    for k in (4, 8, 16, 32):
        variants.append((f"k={k}", lambda k=k: lib.slam_bf_knn_u256(h, dq.buf.ptr, n, dt.buf.ptr, m, 0, k, idx.ptr, dist.ptr)))
    reps = REPS.get(n * m, max(1, int(2e10 // (n * m))))
    for _, fn in variants:                                          # warm-up: allocations, code objects, clocks
        for _ in range(3):
            assert fn() == 0, lib.slam_last_error()
    ctx.sync()
    times = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            ctx.timer_start()
            for _ in range(reps):
                assert fn() == 0, lib.slam_last_error()
            times[name].append(ctx.timer_stop() / reps)
    assert ctx.state_dirty() == 0
    for o in (idx, dist, dq, dt):
        o.free()
    pairs = float(n) * m
    base = float(np.median(times["top2"]))
    for name, _ in variants:
        ms = float(np.median(times[name]))
        print(f"{n:>6} x {m:<8} {name:<5} {ms * 1e3:10.1f} us  (min {min(times[name]) * 1e3:9.1f})  "
              f"{pairs / (ms * 1e-3) / 1e12:6.2f} Tpairs/s  floor {pairs * OPS_PER_PAIR / VALU_LANES_PER_S / (ms * 1e-3):5.3f}  "
              f"x top2 {ms / base:5.2f}", flush=True)


def time_host(ctx, k, calls=200):
    rng = np.random.default_rng(228)
    q, t = rng.integers(0, 256, (200, 32), dtype=np.uint8), np.random.default_rng(229).integers(0, 256, (200, 32), dtype=np.uint8)
    for _ in range(20):
        slamhip.topk_match_arrays(q, t, k, ctx=ctx)
    dt = []
    for _ in range(calls):
        t0 = time.perf_counter()
        slamhip.topk_match_arrays(q, t, k, ctx=ctx)
        dt.append(time.perf_counter() - t0)
    print(f"host call 200 x 200 k={k}: median {np.median(dt) * 1e6:.1f} us, p10 {np.percentile(dt, 10) * 1e6:.1f} us "
          f"(topk_match_arrays: upload, search, download, one synchronisation)", flush=True)


def main():
    rounds = opt("--rounds", 5)
    shapes = [tuple(int(v) for v in a.split("x")) for a in sys.argv[1:]] or \
        [(4096, 4096), (8192, 65536), (65536, 65536), (4096, 1 << 20)]
    ctx = slamhip.default_context()
    print(f"libslamhip {slamhip.load().slam_version().decode()}, {rounds} rounds, median per call", flush=True)
    for n, m in shapes:
        time_shape(ctx, n, m, rounds)
    for k in (3, 8):
        time_host(ctx, k)
    q = np.random.default_rng(228).integers(0, 256, (4096, 32), dtype=np.uint8)
    t = np.random.default_rng(229).integers(0, 256, (4096, 32), dtype=np.uint8)
    oracle.bf_knn_c(q, t, 8, threads=16)
    dt = []
    for _ in range(5):
        t0 = time.perf_counter()
        oracle.bf_knn_c(q, t, 8, threads=16)
        dt.append(time.perf_counter() - t0)
    print(f"CPU oracle port (oracle.bf_knn_c, 16 threads, {oracle.bf_simd()}) 4096 x 4096 k=8: median {np.median(dt) * 1e3:.2f} ms",
          flush=True)


if __name__ == "__main__":
    main()
