"""Time of the absolute-pose calls (slam_pnp_*), all from HIP events (slam_timer_start/stop) around back-to-back calls on
device-resident arrays, after warm-up; the median and the spread (min - max) over the rounds are reported.

    python tools/pnp_time.py [--rounds R]

  * solver     slam_pnp_p3p_f64 alone at S = 256 / 65536 samples, us per call and ns per sample;
  * candidate  slam_pnp_ransac_f64 on one candidate of 200 correspondences, H = 256;
  * batch      the same on 16 / 256 / 4096 candidates of 200 correspondences, per call and per candidate.
Scenes: 0.5 px noise, 30 % outliers, EuRoC intrinsics, generated from default_rng(228) the way tests/pnp_ref.py does
(restated here: the tool does not import the tests).  The values are a record, not a gate."""
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
    """B candidates of n correspondences each: (X [B,n,3], px [B,n,2]); rotation 1 - 20 degrees, unit translation, depth 2 - 20."""
    fx, fy, cx, cy = K
    ax = rng.normal(size=(B, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    ang = np.radians(rng.uniform(1, 20, B))
    Kx = np.zeros((B, 3, 3))
    Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0], Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -ax[:, 2], ax[:, 1], ax[:, 2], -ax[:, 0], -ax[:, 1], ax[:, 0]
    R = np.eye(3) + np.sin(ang)[:, None, None] * Kx + (1 - np.cos(ang))[:, None, None] * (Kx @ Kx)
    t = rng.normal(size=(B, 3))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    u, v, z = rng.uniform(0, 752, (B, n)), rng.uniform(0, 480, (B, n)), rng.uniform(2, 20, (B, n))
    Y = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], -1)
    X = (Y - t[:, None, :]) @ R                                   # R^T (Y - t), row-wise
    px = np.stack([u, v], -1) + rng.normal(0, noise, (B, n, 2))
    bad = rng.uniform(size=(B, n)) < outliers
    px[bad] = np.stack([rng.uniform(0, 752, bad.sum()), rng.uniform(0, 480, bad.sum())], -1)
    return np.ascontiguousarray(X), px


def main():
    rounds = opt("--rounds", 7)
    ctx = slamhip.default_context()
    lib, h = ctx.lib, ctx.handle
    rng = np.random.default_rng(228)

    def timed(fn):
        ctx.timer_start()
        fn()
        return ctx.timer_stop()

    print(slamhip.load().slam_version().decode())
    for S in (256, 65536):
        X, px = scenes(rng, S, 3, 0.0, 0.0)
        x = np.stack([(px[..., 0] - K[2]) / K[0], (px[..., 1] - K[3]) / K[1]], -1)
        dX, dx, dp, dn = ctx.upload(X), ctx.upload(x), ctx.malloc(S * 384), ctx.malloc(S * 4)

        def call():
            assert lib.slam_pnp_p3p_f64(h, S, dX.ptr, dx.ptr, dp.ptr, dn.ptr) == 0

        timed(call)
        v = [timed(call) for _ in range(rounds)]
        print(f"solver     S = {S:6d}: {spread(v)}  {np.median(v) * 1e6 / S:8.1f} ns / sample, mean solutions {dn.download(np.int32, (S,)).mean():.2f}")
        for o in (dX, dx, dp, dn):
            o.free()
    for B in (1, 16, 256, 4096):
        X, px = scenes(rng, B, 200)
        off = np.arange(B + 1, dtype=np.int32) * 200
        dX, dp, do = ctx.upload(X.reshape(-1, 3)), ctx.upload(px.reshape(-1, 2)), ctx.upload(off)
        dT, dm, ds = ctx.malloc(B * 96), ctx.malloc(B * 200), ctx.malloc(B * 16)

        def call():
            assert lib.slam_pnp_ransac_f64(h, B, do.ptr, dX.ptr, dp.ptr, B * 200, *K, 256, 8.0, 0, dT.ptr, dm.ptr, ds.ptr) == 0

        timed(call)
        v = [timed(call) for _ in range(rounds)]
        st = ds.download(np.int32, (B, 4))
        name = "candidate" if B == 1 else "batch    "
        print(f"{name}  B = {B:6d}: {spread(v)}  {np.median(v) * 1e3 / B:8.2f} us / candidate, mean inliers {st[:, 0].mean():.1f}, models {st[:, 3].mean():.0f}")
        for o in (dX, dp, do, dT, dm, ds):
            o.free()


if __name__ == "__main__":
    main()
