"""numpy statement of the lens-distortion calls (slam_cam_*, include/slamhip.h) on another route than csrc/cam_model.h: the
inverse by OpenCV's FIXED-POINT iteration run until the iterate stops changing (the library runs Newton steps), the map in
vectorised f64 numpy, the remap as the header's integer formula on whole arrays, and a 50-digit mpmath solve of the inverse."""
from __future__ import annotations

import numpy as np

SENTINEL = -2 ** 31


def distort_n(case, x, y):
    """normalised (x, y) -> distorted normalised (xd, yd), arrays."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if case.model == "pinhole":
        return x.copy(), y.copy()
    if case.model == "radtan":
        k1, k2, p1, p2, k3 = case.coeffs
        r2 = x * x + y * y
        rad = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
        return x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x), y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    k1, k2, k3, k4 = case.coeffs
    r = np.hypot(x, y)
    th = np.arctan(r)
    thd = th * (1 + k1 * th ** 2 + k2 * th ** 4 + k3 * th ** 6 + k4 * th ** 8)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(r == 0, 1.0, thd / r)
    return x * s, y * s


def distort(case, px):
    """pinhole pixels [n,2] -> raw pixels [n,2]."""
    fx, fy, cx, cy = case.K
    px = np.asarray(px, np.float64).reshape(-1, 2)
    xd, yd = distort_n(case, (px[:, 0] - cx) / fx, (px[:, 1] - cy) / fy)
    return np.stack([fx * xd + cx, fy * yd + cy], -1)


def undistort_fixed_point(case, px, max_iterations: int = 5000):
    """raw pixels [n,2] -> (pinhole pixels [n,2], normalised [n,2]) by cv2.undistortPoints' iteration x <- (x0 - tangential(x)) /
    radial(x) (cv2.fisheye: theta <- rd / poly(theta)), run until no iterate changes any more (or repeats its value of two
    steps ago: a two-cycle of neighbouring doubles).  Meaningful only where the model is monotonic."""
    fx, fy, cx, cy = case.K
    px = np.asarray(px, np.float64).reshape(-1, 2)
    x0, y0 = (px[:, 0] - cx) / fx, (px[:, 1] - cy) / fy
    if case.model == "pinhole":
        x, y = x0, y0
    elif case.model == "radtan":
        k1, k2, p1, p2, k3 = case.coeffs
        x, y = x0.copy(), y0.copy()
        before = (None, None)
        for _ in range(max_iterations):
            r2 = x * x + y * y
            rad = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
            nx = (x0 - (2 * p1 * x * y + p2 * (r2 + 2 * x * x))) / rad
            ny = (y0 - (p1 * (r2 + 2 * y * y) + 2 * p2 * x * y)) / rad
            same = np.array_equal(nx, x) and np.array_equal(ny, y)
            cycle = before[0] is not None and np.array_equal(nx, before[0]) and np.array_equal(ny, before[1])
            before = (x, y)
            x, y = nx, ny
            if same or cycle:
                break
    else:
        k1, k2, k3, k4 = case.coeffs
        rd = np.hypot(x0, y0)
        th, before = rd.copy(), None
        for _ in range(max_iterations):
            t2 = th * th
            nt = rd / (1 + k1 * t2 + k2 * t2 ** 2 + k3 * t2 ** 3 + k4 * t2 ** 4)
            same, cycle = np.array_equal(nt, th), before is not None and np.array_equal(nt, before)
            before, th = th, nt
            if same or cycle:
                break
        with np.errstate(invalid="ignore", divide="ignore"):
            s = np.where(rd == 0, 1.0, np.tan(th) / rd)
        x, y = x0 * s, y0 * s
    return np.stack([fx * x + cx, fy * y + cy], -1), np.stack([x, y], -1)


def undistort_mp(case, px, digits: int = 50):
    """The inverse of each raw pixel solved in ``digits``-digit arithmetic (mpmath Newton from the fixed-point answer), rounded
    to f64: pinhole pixels [n,2]."""
    import mpmath as mp

    fx, fy, cx, cy = [mp.mpf(v) for v in case.K]
    start = undistort_fixed_point(case, px)[1]
    out = []
    with mp.workdps(digits):
        for (u, v), (sx, sy) in zip(np.asarray(px, np.float64).reshape(-1, 2), start):
            x0, y0 = (mp.mpf(float(u)) - cx) / fx, (mp.mpf(float(v)) - cy) / fy
            if case.model == "pinhole":
                x, y = x0, y0
            elif case.model == "radtan":
                k1, k2, p1, p2, k3 = [mp.mpf(c) for c in case.coeffs]

                def f(x, y):
                    r2 = x * x + y * y
                    rad = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
                    return (x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x) - x0, y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y - y0)

                x, y = mp.findroot(f, (mp.mpf(float(sx)), mp.mpf(float(sy))), tol=mp.mpf(10) ** (-2 * digits + 10), maxsteps=100)
            else:
                k = [mp.mpf(c) for c in case.coeffs]
                rd = mp.sqrt(x0 * x0 + y0 * y0)
                if rd == 0:
                    x, y = x0, y0
                else:
                    th = mp.findroot(lambda t: t * (1 + k[0] * t ** 2 + k[1] * t ** 4 + k[2] * t ** 6 + k[3] * t ** 8) - rd, rd,
                                     tol=mp.mpf(10) ** (-2 * digits + 10), maxsteps=100)
                    x, y = x0 * mp.tan(th) / rd, y0 * mp.tan(th) / rd
            out.append([float(fx * x + cx), float(fy * y + cy)])
    return np.asarray(out, np.float64).reshape(-1, 2)


def rectify_map(case, size_out, new_K, R=None):
    """slam_cam_rectify_map in f64 numpy: (map int32 [H,W,2], exact f64 [H,W,2] = 32 * (u, v) before rounding, NaN at sentinels)."""
    W, H = size_out
    nfx, nfy, ncx, ncy = new_K
    R = np.eye(3) if R is None else np.asarray(R, np.float64).reshape(3, 3)
    j, i = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    ray = np.stack([(j - ncx) / nfx, (i - ncy) / nfy, np.ones_like(j)], -1) @ R              # row vector times R = R^T ray
    Z = ray[..., 2]
    front = Z > 0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        xd, yd = distort_n(case, ray[..., 0] / Z, ray[..., 1] / Z)
        s = 32.0 * np.stack([case.K[0] * xd + case.K[2], case.K[1] * yd + case.K[3]], -1)
        ok = front & (np.abs(s) < 2.0 ** 30).all(-1)                                            # (NaN and inf fail)
    m = np.full((H, W, 2), SENTINEL, np.int64)
    m[ok] = np.rint(s[ok]).astype(np.int64)
    return m.astype(np.int32), np.where(ok[..., None], s, np.nan)


def remap(src, mp, border: int = 0):
    """slam_cam_remap_u8: src u8 [B,Hs,Ws] (or [Hs,Ws]), mp int32 [Hd,Wd,2] -> (dst u8 [B,Hd,Wd], mask u8 [B,Hd,Wd])."""
    src = np.asarray(src, np.uint8)
    single = src.ndim == 2
    src = src[None] if single else src
    B, Hs, Ws = src.shape
    U, V = mp[..., 0].astype(np.int64), mp[..., 1].astype(np.int64)
    sent = (U == SENTINEL) | (V == SENTINEL)
    x0, a, y0, b = U >> 5, U & 31, V >> 5, V & 31
    total = np.zeros((B,) + U.shape, np.int64)
    valid = np.ones(U.shape, bool)
    for dx, dy, w in ((0, 0, (32 - a) * (32 - b)), (1, 0, a * (32 - b)), (0, 1, (32 - a) * b), (1, 1, a * b)):
        xx, yy = x0 + dx, y0 + dy
        inside = (xx >= 0) & (xx < Ws) & (yy >= 0) & (yy < Hs)
        tap = np.where(inside, src[:, np.clip(yy, 0, Hs - 1), np.clip(xx, 0, Ws - 1)].astype(np.int64), border)
        total += w * tap
        valid &= inside | (w == 0)
    dst = np.where(sent, border, (total + 512) >> 10).astype(np.uint8)
    mask = np.broadcast_to(np.where(valid & ~sent, 255, 0).astype(np.uint8), dst.shape).copy()
    return (dst[0], mask[0]) if single else (dst, mask)
