"""Time of the homography calls (slam_hg_*), all from HIP events (slam_timer_start/stop) around back-to-back calls on
device-resident arrays, after warm-up; the median and the spread (min - max) over the rounds are reported.

    python tools/homography_time.py [--rounds R] > profiles/homography_time.log

  * solver      slam_hg_fourpoint_f64 alone at S = 256 / 65536 samples, us per call and ns per sample;
  * pair        slam_hg_ransac_f64 on one pair of 200 matches, H = 256;
  * batch       the same on 16 / 256 / 4096 pairs of 200 matches, per call and per pair;
  * essential   slam_tv_essential_ransac_f64 on the same inputs in the same session (B = 1 / 256), for comparison;
  * decompose   slam_hg_decompose_f64 of the 256 winners on their inliers;
  * score       slam_hg_model_score_f64 of the 256 (H, E) pairs.
Scenes: a plane at depth 4 - 12 with a random normal, rotation 1 - 20 degrees, unit translation, 0.5 px noise, 30 % outliers,
EuRoC intrinsics, from default_rng(228) (restated here: the tool does not import the tests).  The values are a record, not a gate."""
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
    """B planar pairs of n matches each: (px1 [B,n,2], px2 [B,n,2])."""
    fx, fy, cx, cy = K
    ax = rng.normal(size=(B, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    ang = np.radians(rng.uniform(1, 20, B))
    Kx = np.zeros((B, 3, 3))
    Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0], Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -ax[:, 2], ax[:, 1], ax[:, 2], -ax[:, 0], -ax[:, 1], ax[:, 0]
    R = np.eye(3) + np.sin(ang)[:, None, None] * Kx + (1 - np.cos(ang))[:, None, None] * (Kx @ Kx)
    t = rng.normal(size=(B, 3))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    nrm = np.c_[rng.uniform(-0.5, 0.5, (B, 2)), np.ones(B)]
    d = rng.uniform(4, 12, B)
    u, v = rng.uniform(0, 752, (B, n)), rng.uniform(0, 480, (B, n))
    a, b = (u - cx) / fx, (v - cy) / fy
    z = d[:, None] / (nrm[:, None, 0] * a + nrm[:, None, 1] * b + nrm[:, None, 2])
    X = np.stack([a * z, b * z, z], -1)
    Y = np.einsum("bij,bnj->bni", R, X) + t[:, None, :]
    px1 = np.stack([u, v], -1) + rng.normal(0, noise, (B, n, 2))
    px2 = np.stack([fx * Y[..., 0] / Y[..., 2] + cx, fy * Y[..., 1] / Y[..., 2] + cy], -1) + rng.normal(0, noise, (B, n, 2))
    bad = rng.uniform(size=(B, n)) < outliers
    px2[bad] = np.stack([rng.uniform(0, 752, bad.sum()), rng.uniform(0, 480, bad.sum())], -1)
    return np.ascontiguousarray(px1), np.ascontiguousarray(px2)


def main():
    rounds = opt("--rounds", 7)
    ctx = slamhip.default_context()
    lib, h = ctx.lib, ctx.handle
    rng = np.random.default_rng(228)

    def timed(fn):
        ctx.timer_start()
        fn()
        return ctx.timer_stop()

    def measure(fn):
        timed(fn)
        return [timed(fn) for _ in range(rounds)]

    print(slamhip.load().slam_version().decode())
    for S in (256, 65536):
        p1, p2 = scenes(rng, S, 4, 0.0, 0.0)
        d1, d2, dH, dk = ctx.upload(p1), ctx.upload(p2), ctx.malloc(S * 72), ctx.malloc(S * 4)
        v = measure(lambda: lib.slam_hg_fourpoint_f64(h, S, d1.ptr, d2.ptr, dH.ptr, dk.ptr))
        print(f"solver     S = {S:6d}: {spread(v)}  {np.median(v) * 1e6 / S:8.2f} ns / sample, models {dk.download(np.int32, (S,)).mean():.3f}")
        for o in (d1, d2, dH, dk):
            o.free()
    for B in (1, 16, 256, 4096):
        px1, px2 = scenes(rng, B, 200)
        M = B * 200
        off = np.arange(B + 1, dtype=np.int32) * 200
        d1, d2, do = ctx.upload(px1.reshape(-1, 2)), ctx.upload(px2.reshape(-1, 2)), ctx.upload(off)
        dH, dm, ds = ctx.malloc(B * 72), ctx.malloc(M), ctx.malloc(B * 16)
        v = measure(lambda: lib.slam_hg_ransac_f64(h, B, do.ptr, d1.ptr, d2.ptr, M, 256, 3.0, 0, dH.ptr, dm.ptr, ds.ptr))
        st = ds.download(np.int32, (B, 4))
        name = "pair     " if B == 1 else "batch    "
        print(f"{name}  B = {B:6d}: {spread(v)}  {np.median(v) * 1e3 / B:8.2f} us / pair, mean inliers {st[:, 0].mean():.1f}, models {st[:, 3].mean():.0f}")
        if B in (1, 256):
            dE, dme, dse = ctx.malloc(B * 72), ctx.malloc(M), ctx.malloc(B * 16)
            v = measure(lambda: lib.slam_tv_essential_ransac_f64(h, B, do.ptr, d1.ptr, d2.ptr, M, *K, 256, 1.0, 0, dE.ptr, dme.ptr, dse.ptr))
            print(f"essential  B = {B:6d}: {spread(v)}  {np.median(v) * 1e3 / B:8.2f} us / pair (slam_tv_essential_ransac_f64, same matches)")
        if B == 256:
            dpa, dna, dc, dp, dsv, dg, dsd = (ctx.malloc(B * 384), ctx.malloc(B * 96), ctx.malloc(B * 16), ctx.malloc(B * 96), ctx.malloc(B * 24),
                                              ctx.malloc(M), ctx.malloc(B * 16))
            v = measure(lambda: lib.slam_hg_decompose_f64(h, B, do.ptr, d1.ptr, d2.ptr, M, *K, dH.ptr, dm.ptr, 50.0, dpa.ptr, dna.ptr, dc.ptr,
                                                          dp.ptr, dsv.ptr, dg.ptr, dsd.ptr))
            sd = dsd.download(np.int32, (B, 4))
            print(f"decompose  B = {B:6d}: {spread(v)}  {np.median(v) * 1e3 / B:8.2f} us / pair, mean best count {sd[:, 0].mean():.1f}")
            dsc, dr = ctx.malloc(B * 16), ctx.malloc(B * 8)
            v = measure(lambda: lib.slam_hg_model_score_f64(h, B, do.ptr, d1.ptr, d2.ptr, M, *K, dH.ptr, dE.ptr, 1.0, dsc.ptr, dr.ptr))
            print(f"score      B = {B:6d}: {spread(v)}  {np.median(v) * 1e3 / B:8.2f} us / pair, mean R_H {dr.download(np.float64, (B,)).mean():.3f}")
            for o in (dpa, dna, dc, dp, dsv, dg, dsd, dsc, dr):
                o.free()
        if B in (1, 256):
            for o in (dE, dme, dse):
                o.free()
        for o in (d1, d2, do, dH, dm, ds):
            o.free()


if __name__ == "__main__":
    main()
