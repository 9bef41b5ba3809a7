"""Time of the two-view geometry calls (slam_tv_*), all from HIP events (slam_timer_start/stop) around back-to-back calls on
device-resident arrays, after warm-up; the median and the spread (min - max) over the rounds are reported.

    python tools/two_view_time.py [--rounds R]

  * solver    slam_tv_fivepoint_f64 alone at S = 256 / 4096 / 65536 samples, us per call and ns per sample;
  * pair      slam_tv_essential_ransac_f64 on one pair of 200 matches, H = 256;
  * batch     the same on 16 / 256 / 4096 pairs of 200 matches, per call and per pair, and with slam_tv_recover_pose_f64 behind it;
  * points    slam_tv_triangulate_f64 on 2^20 points.
Scenes: 0.5 px noise, 30 % outliers, EuRoC intrinsics, generated from default_rng(228) the way tests/two_view_ref.py does
(restated here: the tool does not import the tests)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "slam-experiments_amd"), ROOT):
    sys.path.insert(0, p)

import slamhip  # noqa: E402

K = (458.654, 457.296, 367.215, 248.375)


def opt(name, default):
    if name in sys.argv:
        i = sys.argv.index(name)
        v = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        return type(default)(v)
    return default


def spread(v):
    return f"{np.median(v) * 1e3:10.1f} us  [{min(v) * 1e3:9.1f} - {max(v) * 1e3:9.1f}]"


def scenes(rng, B, n, noise=0.5, outliers=0.3):
    """B frame pairs of n matches each: (px1 [B,n,2], px2 [B,n,2]); rotation 1 - 20 degrees, unit baseline, depth 2 - 20."""
    fx, fy, cx, cy = K
    ax = rng.normal(size=(B, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    ang = np.radians(rng.uniform(1, 20, B))
    Kx = np.zeros((B, 3, 3))
    Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0], Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -ax[:, 2], ax[:, 1], ax[:, 2], -ax[:, 0], -ax[:, 1], ax[:, 0]
    R = np.eye(3) + np.sin(ang)[:, None, None] * Kx + (1 - np.cos(ang))[:, None, None] * (Kx @ Kx)
    t = rng.normal(size=(B, 3))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    u, v, z = rng.uniform(100, 652, (B, n)), rng.uniform(60, 420, (B, n)), rng.uniform(2, 20, (B, n))
    X = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], -1)
    Q = X @ np.swapaxes(R, 1, 2) + t[:, None, :]
    Q[..., 2] = np.maximum(Q[..., 2], 0.5)
    px1 = np.stack([u, v], -1) + rng.normal(0, noise, (B, n, 2))
    px2 = np.stack([fx * Q[..., 0] / Q[..., 2] + cx, fy * Q[..., 1] / Q[..., 2] + cy], -1) + rng.normal(0, noise, (B, n, 2))
    bad = rng.uniform(size=(B, n)) < outliers
    px2[bad] = np.stack([rng.uniform(0, 752, bad.sum()), rng.uniform(0, 480, bad.sum())], -1)
    return px1, px2


def timed(ctx, fn, reps):
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def measure(ctx, fn, reps, rounds):
    for _ in range(2):
        timed(ctx, fn, reps)
    return [timed(ctx, fn, reps) for _ in range(rounds)]


def main():
    rounds = opt("--rounds", 7)
    ctx = slamhip.default_context()
    lib, h = ctx.lib, ctx.handle
    rng = np.random.default_rng(228)
    print(f"libslamhip {slamhip.load().slam_version().decode()}, {rounds} rounds, median [min - max] per call", flush=True)

    for S in (256, 4096, 65536):
        px1, px2 = scenes(rng, S, 5, 0.0, 0.0)
        x1 = np.stack([(px1[..., 0] - K[2]) / K[0], (px1[..., 1] - K[3]) / K[1]], -1)
        x2 = np.stack([(px2[..., 0] - K[2]) / K[0], (px2[..., 1] - K[3]) / K[1]], -1)
        d1, d2, dE, dn = ctx.upload(x1), ctx.upload(x2), ctx.malloc(S * 720), ctx.malloc(S * 4)

        def solver():
            assert lib.slam_tv_fivepoint_f64(h, S, d1.ptr, d2.ptr, dE.ptr, dn.ptr) == 0, lib.slam_last_error()

        v = measure(ctx, solver, 10, rounds)
        roots = dn.download(np.int32, (S,)).mean()
        print(f"solver  S = {S:6d}: {spread(v)}   {np.median(v) * 1e6 / S:8.1f} ns per sample   {roots:.2f} real roots per sample", flush=True)
        for o in (d1, d2, dE, dn):
            o.free()

    for B in (1, 16, 256, 4096):
        n = 200
        px1, px2 = scenes(rng, B, n)
        off = (np.arange(B + 1) * n).astype(np.int32)
        d1, d2, do = ctx.upload(px1.reshape(-1, 2)), ctx.upload(px2.reshape(-1, 2)), ctx.upload(off)
        dE, dm, ds = ctx.malloc(B * 72), ctx.malloc(B * n), ctx.malloc(B * 16)
        dp, dg, dq = ctx.malloc(B * 96), ctx.malloc(B * n), ctx.malloc(B * 8)

        def ransac():
            assert lib.slam_tv_essential_ransac_f64(h, B, do.ptr, d1.ptr, d2.ptr, B * n, *K, 256, 1.0, 0, dE.ptr, dm.ptr, ds.ptr) == 0, lib.slam_last_error()

        def both():
            ransac()
            assert lib.slam_tv_recover_pose_f64(h, B, do.ptr, d1.ptr, d2.ptr, B * n, *K, dE.ptr, None, 50.0, dp.ptr, dg.ptr, dq.ptr) == 0, lib.slam_last_error()

        reps = 10 if B <= 256 else 2
        v, w = measure(ctx, ransac, reps, rounds), measure(ctx, both, reps, rounds)
        st = ds.download(np.int32, (B, 4))
        name = "pair " if B == 1 else "batch"
        print(f"{name}   B = {B:6d} x {n} matches, H = 256: ransac {spread(v)} ({np.median(v) * 1e3 / B:8.2f} us per pair)   "
              f"+ recover_pose {spread(w)}   mean inliers {st[:, 0].mean():.1f}, models scored per pair {st[:, 3].mean():.0f}", flush=True)
        for o in (d1, d2, do, dE, dm, ds, dp, dg, dq):
            o.free()

    N = 1 << 20
    px1, px2 = scenes(rng, 1, N, 0.5, 0.0)
    x1 = np.stack([(px1[0, :, 0] - K[2]) / K[0], (px1[0, :, 1] - K[3]) / K[1]], -1)
    x2 = np.stack([(px2[0, :, 0] - K[2]) / K[0], (px2[0, :, 1] - K[3]) / K[1]], -1)
    P1 = np.eye(4)[:3].reshape(12)
    P2 = np.array([1, 0, 0, 1.0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64)
    dP1, dP2, d1, d2, dX, dw = ctx.upload(P1), ctx.upload(P2), ctx.upload(x1), ctx.upload(x2), ctx.malloc(N * 24), ctx.malloc(N * 8)

    def tri():
        assert lib.slam_tv_triangulate_f64(h, N, dP1.ptr, dP2.ptr, d1.ptr, d2.ptr, dX.ptr, dw.ptr) == 0, lib.slam_last_error()

    v = measure(ctx, tri, 10, rounds)
    print(f"points  N = {N}: {spread(v)}   {N * 64 / np.median(v) / 1e6:.1f} GB/s of the 64 B a point moves", flush=True)


if __name__ == "__main__":
    main()
