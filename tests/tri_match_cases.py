"""Scenes and hand-built cases shared by the CPU and GPU tests of the epipolar search: a synthetic two-keyframe
scene with a real baseline, random pairs under a rectified-stereo F for the shape tests, the exact edge set of the gates, and
one match for every status of the triangulation step."""
import numpy as np

import tri_match_ref as R

CAMERA = (256.0, 256.0, 320.0, 240.0)
SIZE = (640, 480)
SCALE, SIGMA2 = R.scale_tables(8, 1.2)
F_RECT = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])    # lines y2 = y1: den = 1, num = y2 - y1
NO_EPIPOLE = np.array([np.nan, np.nan])


def rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def pose(R_, centre):
    """world -> camera [3,4] of a camera at ``centre`` with rotation R_."""
    return np.c_[R_, -R_ @ np.asarray(centre, np.float64)]


def flip_bits(rng, desc, k):
    """``desc`` u8 [n,32] with k[i] distinct random bits of row i flipped."""
    out = desc.copy()
    for i, ki in enumerate(k):
        for b in rng.choice(256, int(ki), replace=False):
            out[i, b >> 3] ^= np.uint8(1 << (b & 7))
    return out


POSES = (pose(rot([0, 1, 0], 1.0), [0.0, 0.0, 0.0]), pose(rot([0.1, 1, 0], -3.0), [0.6, 0.05, 0.02]),
         pose(rot([0, 1, 0.1], -1.0), [0.3, -0.04, 0.1]))


def make_scene(seed, n_common, n_rows, n_nodes=12, noise=0.2, poses=POSES):
    """Two keyframes of ``n_rows`` rows seeing ``n_common`` common points (depths 2 to 8), the rest clutter; a third frame that
    sees the common points too.  Returns (s1, s2, frame3, truth) with truth = dict(rows1, rows2, X): the rows of the common
    points in the two keyframes and their world positions."""
    rng = np.random.default_rng(seed)
    T1, T2, T3 = poses
    X = np.zeros((0, 3))
    while len(X) < n_common:                             # points inside all three images with a margin
        px = np.stack([rng.uniform(40, 600, 4 * n_common), rng.uniform(40, 440, 4 * n_common)], 1)
        z = rng.uniform(2.0, 8.0, 4 * n_common)
        c = np.stack([(px[:, 0] - CAMERA[2]) / CAMERA[0] * z, (px[:, 1] - CAMERA[3]) / CAMERA[1] * z, z], 1)
        W = (c - T1[:, 3]) @ T1[:, :3]
        ok = np.ones(len(W), bool)
        for T in (T2, T3):
            p, d = R.project(T, W, CAMERA)
            ok &= (d > 0.5) & (p[:, 0] > 20) & (p[:, 0] < 620) & (p[:, 1] > 20) & (p[:, 1] < 460)
        X = np.concatenate([X, W[ok]])[:n_common]
    base = rng.integers(0, 256, (n_common, 32), dtype=np.uint8)
    node = rng.integers(0, n_nodes, n_common)
    level = rng.integers(0, 4, n_common)
    bins = rng.integers(0, 32, n_common)
    sides = []
    for T in (T1, T2, T3):
        n_extra = n_rows - n_common
        xy = np.concatenate([R.project(T, X, CAMERA)[0] + rng.normal(0, noise, (n_common, 2)),
                             np.stack([rng.uniform(0, 640, n_extra), rng.uniform(0, 480, n_extra)], 1)]).astype(np.float32)
        s = dict(desc=np.concatenate([flip_bits(rng, base, rng.integers(0, 10, n_common)), rng.integers(0, 256, (n_extra, 32), dtype=np.uint8)]),
                 nodes=np.concatenate([node, rng.integers(0, n_nodes, n_extra)]).astype(np.int32), xy=xy,
                 level=np.concatenate([level, rng.integers(0, 4, n_extra)]).astype(np.int32),
                 bins=np.concatenate([bins, rng.integers(0, 32, n_extra)]).astype(np.uint8))
        perm = rng.permutation(n_rows)
        s = {k: np.ascontiguousarray(v[perm]) for k, v in s.items()}
        s["row_of_point"] = np.argsort(perm)[:n_common]
        sides.append(s)
    truth = dict(rows1=sides[0].pop("row_of_point"), rows2=sides[1].pop("row_of_point"), rows3=sides[2].pop("row_of_point"), X=X)
    return sides[0], sides[1], sides[2], truth


def random_pair(seed, n1, n2, n_nodes=6, masked=True, taken=True, bins=False, pool=None):
    """Two images for the shape tests under F_RECT: y on a lattice of spacing 3 (a neighbouring lattice row passes the line gate
    from level 2 up only: sqrt(3.84 * 1.2^(2 l)) = 1.96, 2.35, 2.82, 3.39 px), descriptors a few bits from a small pool."""
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 256, (max(2, 2 * n_nodes), 32), dtype=np.uint8) if pool is None else pool

    def side(n):
        s = dict(desc=flip_bits(rng, pool[rng.integers(0, len(pool), n)], rng.integers(0, 34, n)) if n else np.zeros((0, 32), np.uint8),
                 nodes=rng.integers(-1 if masked else 0, n_nodes, n).astype(np.int32),
                 xy=np.stack([rng.integers(0, 640, n), 3 * rng.integers(0, 6, n)], 1).astype(np.float32).reshape(n, 2),
                 level=rng.integers(0, 4, n).astype(np.int32))
        if taken:
            s["taken"] = (rng.random(n) < 0.1).astype(np.uint8)
        if bins:
            s["bins"] = rng.integers(0, 4, n).astype(np.uint8)
        return s
    return side(n1), side(n2)


POOL = np.random.default_rng(1).integers(0, 256, (8, 32), dtype=np.uint8)     # one pool for images made by separate calls
EPIPOLE_RECT = np.array([320.0, 6.0])                    # inside the lattice: the epipole gate removes rows near it


def edge_gates():
    """The exact edge set: integer pixels, integer F, chi2 * sigma2 a power of two (chi2 = 4, sigma2 = 1, 4).  Returns
    (xy1, xy2, level2, scale, sigma2, chi2, [(F, epipole, expected on_line [n1, n2] or None)])."""
    below = np.nextafter(np.float32(102.0), np.float32(0.0))
    xy1 = np.array([[0.0, 0.0], [10.0, 100.0]], np.float32)
    xy2 = np.array([[5.0, 100.0], [7.0, 102.0], [7.0, below], [9.0, 98.0], [3.0, 104.0], [3.0, np.nextafter(np.float32(104.0), np.float32(0.0))]],
                   np.float32)
    level2 = np.array([0, 0, 0, 0, 1, 1], np.int32)
    scale, sigma2 = np.array([1.0, 2.0]), np.array([1.0, 4.0])
    line = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 1.0, -100.0]])        # every side-1 pixel: the line y2 = 100, den = 1
    # level 0: |num| < 2, level 1: |num| < 4; equality is rejected, the next float below passes
    want = np.array([[True, False, True, False, False, True]] * 2)
    nan_f, inf_f, zero_den = line.copy(), line.copy(), np.zeros((3, 3))
    nan_f[2, 1] = np.nan
    inf_f[2, 0] = np.inf
    zero_den[2, 2] = 1.0                                                           # a = b = 0, c = 1
    none = np.zeros((2, 6), bool)
    cases = [(line, NO_EPIPOLE, want), (2.0 * line, NO_EPIPOLE, want), (np.zeros((3, 3)), NO_EPIPOLE, none), (zero_den, NO_EPIPOLE, none),
             (nan_f, NO_EPIPOLE, none), (inf_f, NO_EPIPOLE, none), (line, np.array([7.0, 92.0]), want), (line, np.array([np.nan, 100.0]), want)]
    return xy1, xy2, level2, scale, sigma2, 4.0, cases


def status_cases():
    """One hand-built match for every status 2 to 8 (and one created point).  Camera 1 at the origin; camera 2 one unit to the
    right (A), ten units ahead (B), or at an infinite offset (C).  Returns a list of (T1, T2, p1, p2, l1, l2, status)."""
    I = np.eye(3)
    T1, A, Bk = pose(I, [0, 0, 0]), pose(I, [1, 0, 0]), pose(I, [0, 0, 10])
    C = np.c_[I, [-np.inf, 0.0, 0.0]]
    return [
        (T1, A, (352.0, 240.0), (288.0, 240.0), 0, 0, 0),          # X = (0.5, 0, 4) exactly
        (T1, A, (320.0, 240.0), (319.744, 240.0), 0, 0, 2),        # X = (0, 0, 1000): the rays are 0.06 degrees apart
        (T1, C, (352.0, 240.0), (288.0, 240.0), 0, 0, 3),          # the rays pass the parallax test, the DLT has no finite answer
        (T1, A, (300.0, 240.0), (340.0, 240.0), 0, 0, 4),          # diverging rays: they meet behind both cameras
        (T1, Bk, (352.0, 240.0), (298.6667, 240.0), 0, 0, 5),      # X = (0.5, 0, 4) lies behind the camera ten units ahead
        (T1, A, (352.0, 243.0), (288.0, 237.0), 0, 0, 6),          # 6 px of vertical disparity: 3 px of error in each image
        (T1, A, (352.0, 243.0), (288.0, 237.0), 3, 0, 7),          # ... which level 3 of image 1 tolerates (9 <= 5.991 * 2.99)
        (T1, A, (352.0, 240.0), (288.0, 240.0), 0, 5, 8),          # equal distances, five levels apart
    ]
