"""Time of the Sim(3) calls (slam_sim3_*), all from HIP events (slam_timer_start/stop) around back-to-back calls on
device-resident arrays, after warm-up; the median and the spread (min - max) over the rounds are reported.

    python tools/sim3_time.py [--rounds R]

  * solver     slam_sim3_threepoint_f64 alone at S = 256 / 65536 samples, us per call and ns per sample;
  * candidate  slam_sim3_ransac_f64 on one candidate of 200 correspondences, H = 256;
  * batch      the same on 16 / 256 / 4096 candidates of 200 correspondences, per call and per candidate;
  * refit      slam_sim3_refit_f64 on the RANSAC masks of the 256 x 200 batch, and on one trajectory of 10^5 points;
  * context    slam_pnp_ransac_f64 on the same shape (256 x 200, H = 256) in the same session.
Scenes: pixels uniform in a 752 x 480 image at depths 2 - 20, a similarity of scale 1.2, rotation 1 - 20 degrees and a
translation of 0.5, noise 0.001 of the depth on every coordinate, 30 % outliers, EuRoC intrinsics, from default_rng(3107)
the way tests/sim3_ref.py does (restated here: the tool does not import the tests).  The values are a record, not a gate."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "slam-experiments_amd"), ROOT):
    sys.path.insert(0, p)

import slamhip  # noqa: E402

K = (458.654, 457.296, 367.215, 248.375)
CHI2 = 9.210


def opt(name, default):
    if name in sys.argv:
        i = sys.argv.index(name)
        v = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        return type(default)(v)
    return default


def spread(v):
    return f"{np.median(v) * 1e3:10.1f} us  [{min(v) * 1e3:9.1f} - {max(v) * 1e3:9.1f}]"


def rotations(rng, B):
    ax = rng.normal(size=(B, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    ang = np.radians(rng.uniform(1, 20, B))
    Kx = np.zeros((B, 3, 3))
    Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0], Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -ax[:, 2], ax[:, 1], ax[:, 2], -ax[:, 0], -ax[:, 1], ax[:, 0]
    return np.eye(3) + np.sin(ang)[:, None, None] * Kx + (1 - np.cos(ang))[:, None, None] * (Kx @ Kx)


def cloud(rng, B, n):
    fx, fy, cx, cy = K
    u, v, z = rng.uniform(0, 752, (B, n)), rng.uniform(0, 480, (B, n)), rng.uniform(2, 20, (B, n))
    return np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], -1)


def scenes(rng, B, n, scale=1.2, noise=0.001, outliers=0.3):
    """B candidates of n correspondences each: (X1 [B,n,3], X2 [B,n,3])."""
    R = rotations(rng, B)
    t = rng.normal(size=(B, 3))
    t *= 0.5 / np.linalg.norm(t, axis=1, keepdims=True)
    X1 = cloud(rng, B, n)
    X2 = scale * (X1 @ np.swapaxes(R, 1, 2)) + t[:, None, :]
    X1 = X1 + rng.normal(0, noise, X1.shape) * X1[..., 2:]
    X2 = X2 + rng.normal(0, noise, X2.shape) * X2[..., 2:]
    bad = rng.uniform(size=(B, n)) < outliers
    X2[bad] = scale * cloud(rng, B, n)[bad]
    return np.ascontiguousarray(X1), np.ascontiguousarray(X2)


def main():
    rounds = opt("--rounds", 7)
    ctx = slamhip.default_context()
    lib, h = ctx.lib, ctx.handle
    rng = np.random.default_rng(3107)

    def timed(fn):
        ctx.timer_start()
        fn()
        return ctx.timer_stop()

    def run(call):
        timed(call)
        return [timed(call) for _ in range(rounds)]

    print(slamhip.load().slam_version().decode())
    for S in (256, 65536):
        X1, X2 = scenes(rng, S, 3, noise=0.0, outliers=0.0)
        d1, d2, dm, dk = ctx.upload(X1), ctx.upload(X2), ctx.malloc(S * 104), ctx.malloc(S * 4)

        def call():
            assert lib.slam_sim3_threepoint_f64(h, S, d1.ptr, d2.ptr, 0, dm.ptr, dk.ptr) == 0

        v = run(call)
        print(f"solver     S = {S:6d}: {spread(v)}  {np.median(v) * 1e6 / S:8.1f} ns / sample, models {dk.download(np.int32, (S,)).mean():.3f}")
        for o in (d1, d2, dm, dk):
            o.free()
    for B in (1, 16, 256, 4096):
        X1, X2 = scenes(rng, B, 200)
        off = np.arange(B + 1, dtype=np.int32) * 200
        d1, d2, do = ctx.upload(X1.reshape(-1, 3)), ctx.upload(X2.reshape(-1, 3)), ctx.upload(off)
        dT, dm, ds = ctx.malloc(B * 104), ctx.malloc(B * 200), ctx.malloc(B * 16)

        def call():
            assert lib.slam_sim3_ransac_f64(h, B, do.ptr, d1.ptr, d2.ptr, B * 200, None, *K, 256, CHI2, 0, 0, dT.ptr, dm.ptr, ds.ptr) == 0

        v = run(call)
        st = ds.download(np.int32, (B, 4))
        name = "candidate" if B == 1 else "batch    "
        print(f"{name}  B = {B:6d}: {spread(v)}  {np.median(v) * 1e3 / B:8.2f} us / candidate, mean inliers {st[:, 0].mean():.1f}, models {st[:, 3].mean():.0f}")
        if B == 256:
            dT2, ds2 = ctx.malloc(B * 104), ctx.malloc(B * 8)

            def refit():
                assert lib.slam_sim3_refit_f64(h, B, do.ptr, d1.ptr, d2.ptr, B * 200, dm.ptr, 0, dT2.ptr, ds2.ptr) == 0

            v = run(refit)
            rs = ds2.download(np.int32, (B, 2))
            print(f"refit      B = {B:6d}: {spread(v)}  {np.median(v) * 1e3 / B:8.2f} us / candidate, mean points {rs[:, 0].mean():.1f}, ok {rs[:, 1].mean():.3f}")
            P = X1.reshape(-1, 3)
            px = np.stack([K[0] * P[:, 0] / P[:, 2] + K[2], K[1] * P[:, 1] / P[:, 2] + K[3]], 1) + rng.normal(0, 0.5, (B * 200, 2))
            dp, dP = ctx.upload(px), ctx.malloc(B * 96)

            def pnp():
                assert lib.slam_pnp_ransac_f64(h, B, do.ptr, d1.ptr, dp.ptr, B * 200, *K, 256, 8.0, 0, dP.ptr, dm.ptr, ds.ptr) == 0

            v = run(pnp)
            print(f"context    B = {B:6d}: {spread(v)}  {np.median(v) * 1e3 / B:8.2f} us / candidate  (slam_pnp_ransac_f64, same shape: X1 against its own pixels)")
            for o in (dT2, ds2, dp, dP):
                o.free()
        for o in (d1, d2, do, dT, dm, ds):
            o.free()
    N = 100000
    k = np.arange(N)
    est = np.stack([2 * np.cos(0.001 * k), 2 * np.sin(0.001 * k), 1e-4 * k], 1) + np.cumsum(rng.normal(0, 0.01, (N, 3)), 0)
    gt = 0.37 * (est @ rotations(rng, 1)[0].T) + np.array([4.0, -2.0, 1.5]) + rng.normal(0, 0.01, (N, 3))
    d1, d2, do = ctx.upload(est), ctx.upload(gt), ctx.upload(np.array([0, N], np.int32))
    dT, ds = ctx.malloc(104), ctx.malloc(8)

    def traj():
        assert lib.slam_sim3_refit_f64(h, 1, do.ptr, d1.ptr, d2.ptr, N, None, 0, dT.ptr, ds.ptr) == 0

    v = run(traj)
    m = dT.download(np.float64, (13,))
    print(f"trajectory N = {N:6d}: {spread(v)}  {np.median(v) * 1e6 / N:8.2f} ns / pose, scale {m[12]:.6f}, stats {ds.download(np.int32, (2,)).tolist()}")
    for o in (d1, d2, do, dT, ds):
        o.free()


if __name__ == "__main__":
    main()
