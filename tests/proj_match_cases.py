"""Inputs the projection-search tests share: the gate edge points with the status each must get, stated from the
arithmetic and not from any implementation, a job writer for tests/proj_match_twin.cpp, and a synthetic map seen by a camera."""
import struct

import numpy as np

import proj_match_ref as R

CAMERA = (256.0, 256.0, 320.0, 240.0)
BOUNDS = (0.0, 640.0, 0.0, 480.0)
SIZE = (640, 480)
NAN, INF = float("nan"), float("inf")
H3 = 0.8660254037844386             # a normal (0, H3, 0.5) seen along +z: dot = z / 2 exactly, cos^2 = 1/4 exactly


def edge_points():
    """(xyz, range, normal, expected status, expected lp) under the identity pose, camera centre 0, CAMERA, BOUNDS, scale 2.0
    over 4 levels (scale2 = 1, 4, 16, 64: every product below is exact).  u = 256 X / Z + 320 with Z a power of two."""
    ok_r, up = (1.0, 4096.0), (0.0, 0.0, 1.0)
    rows = [
        # xyz, (dmin2, dmax2), normal, status, lp
        ((0.0, 0.0, 4.0), ok_r, up, 0, 3),                  # d2 = 16: 16, 64, 256 < 4096 -> lp = 3 = n_levels - 1 (clamped at the top)
        ((0.0, 0.0, 0.0), ok_r, up, 1, -1),                 # zc = 0
        ((0.0, 0.0, -2.0), ok_r, up, 1, -1),                # behind
        ((0.0, 0.0, NAN), ok_r, up, 1, -1),                 # a NaN fails zc > 0
        ((NAN, 0.0, 2.0), ok_r, up, 1, -1),                 # A20 * X = 0 * NaN: zc is NaN
        ((0.0, 0.0, INF), ok_r, up, 2, -1),                 # zc = inf passes; xc = 0 * inf = NaN, so u fails the bounds
        ((INF, 0.0, INF), ok_r, up, 1, -1),                 # zc = 0 * inf + inf = NaN
        ((0.0, 0.0, 2.0 ** 600), ok_r, up, 3, -1),          # u = cx, d2 overflows to inf > dmax2
        ((-2.5, 0.0, 2.0), ok_r, up, 0, 3),                 # u = 0 = min_x is kept
        ((2.5, 0.0, 2.0), ok_r, up, 2, -1),                 # u = 640 = max_x is not
        ((0.0, -1.875, 2.0), ok_r, up, 0, 3),               # v = 0 = min_y
        ((0.0, 1.875, 2.0), ok_r, up, 2, -1),               # v = 480 = max_y
        ((0.0, 0.0, 4.0), (16.0, 64.0), up, 0, 1),          # d2 = dmin2 is in range; 16 < 64, 64 < 64 fails -> lp = 1
        ((0.0, 0.0, 4.0), (4.0, 16.0), up, 0, 0),           # d2 = dmax2 is in range; 16 < 16 fails -> lp = 0 (clamped at the bottom)
        ((0.0, 0.0, 4.0), (np.nextafter(16.0, 17.0), 64.0), up, 3, -1),
        ((0.0, 0.0, 4.0), (4.0, np.nextafter(16.0, 15.0)), up, 3, -1),
        ((0.0, 0.0, 4.0), (1.0, 256.0), up, 0, 2),          # 16, 64 < 256, 256 < 256 fails
        ((0.0, 0.0, 4.0), ok_r, (1.0, 0.0, 0.0), 4, -1),    # dot = 0
        ((0.0, 0.0, 4.0), ok_r, (0.0, H3, 0.5), 0, 3),      # dot^2 = 4 = cos2_limit * 16: at the limit, kept
        ((0.0, 0.0, 4.0), ok_r, (0.0, H3, np.nextafter(0.5, 0.0)), 4, -1),
        ((0.0, 0.0, 4.0), ok_r, (0.0, 0.0, -1.0), 4, -1),   # seen from behind its normal
        ((0.0, 0.0, 4.0), ok_r, (NAN, 0.0, 1.0), 4, -1),    # a NaN fails dot > 0
    ]
    xyz = np.array([r[0] for r in rows], np.float64)
    rng = np.array([r[1] for r in rows], np.float64)
    nrm = np.array([r[2] for r in rows], np.float64)
    return xyz, rng, nrm, np.array([r[3] for r in rows], np.int32), np.array([r[4] for r in rows], np.int32)


def random_pose(rng, angle=0.3, shift=0.5):
    """A rigid world -> camera pose [3,4] with no zero or one among its entries."""
    w = rng.normal(0, angle, 3)
    t = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / t
    Rm = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)
    return np.c_[Rm, rng.normal(0, shift, 3)]


def twin_job(xyz, A, Ow, th, camera, bounds, scale, scale2, rng=None, normal=None, level=None, cos2_limit=0.25) -> bytes:
    n = len(xyz)
    s, s2 = np.zeros(16), np.zeros(16)
    s[:len(scale)], s2[:len(scale2)] = scale, scale2
    flags = (1 if rng is not None else 0) | (2 if normal is not None else 0) | (4 if level is not None else 0)
    job = struct.pack("qqq", n, flags, len(scale))
    job += np.concatenate([np.asarray(camera, np.float64), np.asarray(bounds, np.float64), [cos2_limit, th], np.asarray(A, np.float64).reshape(12),
                           np.asarray(Ow, np.float64).reshape(3), s, s2]).astype(np.float64).tobytes()
    job += np.ascontiguousarray(xyz, np.float64).tobytes()
    for a, dt in ((rng, np.float64), (normal, np.float64), (level, np.int32)):
        if a is not None:
            job += np.ascontiguousarray(a, dt).tobytes()
    return job


def parse_twin(text, n):
    rows = [line.split() for line in text.strip().splitlines()]
    assert len(rows) == n, (len(rows), n)
    status = np.array([int(r[0]) for r in rows], np.int32)
    u = np.array([int(r[1], 16) for r in rows], np.uint64).view(np.float64)
    v = np.array([int(r[2], 16) for r in rows], np.uint64).view(np.float64)
    return status, u, v, np.array([int(r[3]) for r in rows], np.int32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def flip_bits(rng, desc, k):
    """``desc`` with k random bits flipped per row."""
    out = desc.copy()
    for i in range(len(out)):
        for b in rng.choice(256, k, replace=False):
            out[i, b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def make_scene(seed, n_points, n_clutter=0, n_levels=8, scale=1.2, size=SIZE, camera=CAMERA, flips=12):
    """A map of ``n_points`` points in front of a camera at ``pose`` and the frame that sees them: one feature per visible
    point at its projection (rounded to f32), on the level its distance predicts, its descriptor the point's with ``flips``
    bits flipped, plus ``n_clutter`` random features.  Returns (points dict, frame dict, pose [3,4], row_of_point int [n])."""
    rng = np.random.default_rng(seed)
    s, s2 = R.scale_tables(n_levels, scale)
    pose = random_pose(rng, 0.1, 0.2)
    fx, fy, cx, cy = camera
    u, v = rng.uniform(20, size[0] - 20, n_points), rng.uniform(20, size[1] - 20, n_points)
    z = rng.uniform(2.0, 12.0, n_points)
    cam = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    xyz = (cam - pose[:, 3]) @ pose[:, :3]                       # R^T (x - t)
    centre = -pose[:, :3].T @ pose[:, 3]
    d = np.linalg.norm(cam, axis=1)
    level = rng.integers(0, n_levels, n_points)                  # the level the point is seen at in this frame
    dmax = d * s[level] * (1.0 - rng.uniform(0.02, 0.8, n_points) * (1.0 - 1.0 / scale))     # s[level-1] d < dmax < s[level] d: lp = level
    dmax = np.where(level == 0, d * 1.01, dmax)                  # level 0 is seen at the far end of the range: lp = 1, and lp - 1 = 0
    dmin = dmax / s[-1] * 0.8
    normal = xyz - centre[None, :]                               # the mean viewing direction: from the camera to the point
    normal /= np.linalg.norm(normal, axis=1)[:, None]
    desc = rng.integers(0, 256, (n_points, 32), dtype=np.uint8)
    bins = rng.integers(0, 32, n_points)
    points = dict(xyz=xyz, desc=desc, range=np.stack([dmin * dmin, dmax * dmax], 1), normal=normal, level=level.astype(np.int32), bins=bins)
    f_desc = np.concatenate([flip_bits(rng, desc, flips), rng.integers(0, 256, (n_clutter, 32), dtype=np.uint8)])
    f_xy = np.concatenate([np.stack([u, v], 1) + rng.normal(0, 0.3, (n_points, 2)),
                           np.stack([rng.uniform(0, size[0], n_clutter), rng.uniform(0, size[1], n_clutter)], 1)]).astype(np.float32)
    f_level = np.concatenate([level, rng.integers(0, n_levels, n_clutter)]).astype(np.int32)
    f_bins = np.concatenate([(bins - 3) % 32, rng.integers(0, 32, n_clutter)])
    perm = rng.permutation(n_points + n_clutter)
    frame = dict(desc=np.ascontiguousarray(f_desc[perm]), xy=np.ascontiguousarray(f_xy[perm]), level=f_level[perm], bins=f_bins[perm])
    row_of_point = np.argsort(perm)[:n_points]
    return points, frame, pose, row_of_point
