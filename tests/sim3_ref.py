"""numpy statement of the Sim(3) calls (slam_sim3_* of include/slamhip.h), written from the definitions.

Imports neither the product nor the twin.  The closed form here takes another route than the kernel: the kernel takes the
rotation from the largest eigenvector of Horn's 4x4 quaternion matrix by cyclic Jacobi; this file is Umeyama's (1991)
solution, the SVD of the 3x3 cross-covariance from ``np.linalg.svd`` with the determinant fix, plain numpy sums.  An
agreement of the two is not an agreement of one piece of code with itself.

Conventions (as the header): X1, X2 [n,3] the two copies of the map points, each in its own camera frame; the model is
(s, R, t) with X2 = s R X1 + t (flat [13]: row-major [R | t], then s).

Also the scene generator of the tests: EuRoC intrinsics, 752 x 480 image; X1 from pixels uniform in the image and a depth
range, a rotation of 1 - 20 degrees about a random axis, a translation of length 0.5, a scale; X2 = s R X1 + t plus noise."""
from __future__ import annotations

import numpy as np

import ransac_draws

EUROC = (458.654, 457.296, 367.215, 248.375)      # fx, fy, cx, cy
IMAGE = (752, 480)
CHI2 = 9.210
SEED = 3107
MASK64 = ransac_draws.MASK64
splitmix = ransac_draws.splitmix
FLAT = 1e-20
BIG = 1e200
MIN_ANGLE_DEG = 5.0
REFIT_SIZES = (3, 4, 63, 64, 65, 255, 256, 257, 1000)


# ---------------------------------------------------------------- models
def pack(s, R, t):
    return np.concatenate([np.concatenate([R, np.reshape(t, (3, 1))], 1).reshape(12), [s]])


def split(model):
    m = np.asarray(model)
    T = m[..., :12].reshape(m.shape[:-1] + (3, 4))
    return m[..., 12], T[..., :3], T[..., 3]


IDENTITY = pack(1.0, np.eye(3), np.zeros(3))


def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    W = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * W + (1 - np.cos(angle)) * W @ W


def apply(model, X):
    s, R, t = split(model)
    return s * (np.asarray(X) @ R.T) + t


# ---------------------------------------------------------------- the closed form (Umeyama, SVD)
def umeyama(X1, X2, fix_scale=False):
    """(s, R, t, sv) minimising sum |X2 - (s R X1 + t)|^2 over proper rotations; sv = singular values of the covariance."""
    X1, X2 = np.asarray(X1, np.float64), np.asarray(X2, np.float64)
    c1, c2 = X1.mean(0), X2.mean(0)
    A, B = X1 - c1, X2 - c2
    U, d, Vt = np.linalg.svd(B.T @ A)
    D = np.array([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    R = U @ np.diag(D) @ Vt
    s = 1.0 if fix_scale else float((d * D).sum() / (A * A).sum())
    return s, R, c2 - s * (R @ c1), d


def triangle_ok(P):
    """The header's rule for one triple [3,3]: neither repeated nor collinear (sin^2 of the angle at the first point)."""
    e12, e13, e23 = P[1] - P[0], P[2] - P[0], P[2] - P[1]
    n = np.cross(e12, e13)
    return bool(n @ n > FLAT * ((e12 @ e12) * (e13 @ e13)) and e23 @ e23 > 0)


def threepoint_one(P1, P2, fix_scale=False):
    """model [13] or None."""
    with np.errstate(all="ignore"):
        if not ((P1 * P1).sum() + (P2 * P2).sum() < BIG):
            return None
        if not (triangle_ok(P1) and triangle_ok(P2)):
            return None
        s, R, t, _ = umeyama(P1, P2, fix_scale)
        m = pack(s, R, t)
        return m if (np.isfinite(m).all() and s > 0) else None


def threepoint(X1, X2, fix_scale=False):
    X1, X2 = np.asarray(X1, np.float64).reshape(-1, 3, 3), np.asarray(X2, np.float64).reshape(-1, 3, 3)
    model, ok = np.tile(IDENTITY, (len(X1), 1)), np.zeros(len(X1), np.int32)
    for i in range(len(X1)):
        m = threepoint_one(X1[i], X2[i], fix_scale)
        if m is not None:
            model[i], ok[i] = m, 1
    return model, ok


def refit(X1, X2, mask=None, fix_scale=False):
    """The least-squares fit over the selected correspondences, plain numpy: (model [13], used)."""
    X1, X2 = np.asarray(X1, np.float64).reshape(-1, 3), np.asarray(X2, np.float64).reshape(-1, 3)
    if mask is not None:
        X1, X2 = X1[np.asarray(mask, bool)], X2[np.asarray(mask, bool)]
    s, R, t, _ = umeyama(X1, X2, fix_scale)
    return pack(s, R, t), len(X1)


# ---------------------------------------------------------------- draws, score, RANSAC (the header's statements)
def draw_sample(seed, h, n):
    """Three distinct indices of hypothesis h among n correspondences."""
    return ransac_draws.draw_sample(seed, h, n, 3)


def score(model, X1, X2, K, chi2=CHI2, sigma2=None):
    """The header's inlier rule, operation by operation: bool [n]."""
    s, R, t = split(np.asarray(model, np.float64))
    X1, X2 = np.asarray(X1, np.float64).reshape(-1, 3), np.asarray(X2, np.float64).reshape(-1, 3)
    fx, fy, cx, cy = K
    sg = np.ones((len(X1), 2)) if sigma2 is None else np.asarray(sigma2, np.float64).reshape(-1, 2)
    with np.errstate(all="ignore"):
        u1, v1 = fx * (X1[:, 0] / X1[:, 2]) + cx, fy * (X1[:, 1] / X1[:, 2]) + cy
        u2, v2 = fx * (X2[:, 0] / X2[:, 2]) + cx, fy * (X2[:, 1] / X2[:, 2]) + cy
        front = (X1[:, 2] > 0) & (X2[:, 2] > 0)
        g1, g2 = np.where(front, chi2 * sg[:, 0], 0.0), np.where(front, chi2 * sg[:, 1], 0.0)
        A = s * R
        c = [((A[i, 0] * X1[:, 0] + A[i, 1] * X1[:, 1]) + A[i, 2] * X1[:, 2]) + t[i] for i in range(3)]
        du2, dv2 = (fx * (c[0] / c[2]) + cx) - u2, (fy * (c[1] / c[2]) + cy) - v2
        y = [X2[:, i] - t[i] for i in range(3)]
        w = [(R[0, i] * y[0] + R[1, i] * y[1]) + R[2, i] * y[2] for i in range(3)]
        du1, dv1 = (fx * (w[0] / w[2]) + cx) - u1, (fy * (w[1] / w[2]) + cy) - v1
        return (c[2] > 0) & (w[2] > 0) & ((du2 * du2 + dv2 * dv2) < g2) & ((du1 * du1 + dv1 * dv1) < g1)


def ransac(X1, X2, K, H, chi2=CHI2, seed=0, sigma2=None, fix_scale=False):
    """slam_sim3_ransac_f64 for one candidate with the numpy solver: (model [13], mask bool [n], stats [4])."""
    X1, X2 = np.asarray(X1, np.float64).reshape(-1, 3), np.asarray(X2, np.float64).reshape(-1, 3)
    n = len(X1)
    none = (IDENTITY.copy(), np.zeros(n, bool), np.array([0, -1, -1, 0], np.int32))
    if n < 3:
        return none
    best, models = None, 0
    for h in range(H):
        idx = draw_sample(seed, h, n)
        m = threepoint_one(X1[idx], X2[idx], fix_scale)
        if m is None:
            continue
        models += 1
        cnt = int(score(m, X1, X2, K, chi2, sigma2).sum())
        if best is None or cnt > best[0]:
            best = (cnt, h, m)
    if best is None:
        return none
    return best[2], score(best[2], X1, X2, K, chi2, sigma2), np.array([best[0], best[1], 0, models], np.int32)


# ---------------------------------------------------------------- scenes
def random_similarity(rng, scale):
    R = rodrigues(rng.normal(size=3), np.deg2rad(rng.uniform(1.0, 20.0)))
    t = rng.normal(size=3)
    return float(scale), R, 0.5 * t / np.linalg.norm(t)


def cloud(rng, n, depth=(2.0, 20.0), K=EUROC):
    """n points in front of camera 1: pixels uniform in the image, depth uniform in the range."""
    u, v, z = rng.uniform(0, IMAGE[0], n), rng.uniform(0, IMAGE[1], n), rng.uniform(depth[0], depth[1], n)
    return np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], 1)


def make_scene(rng, n, scale=1.0, noise=0.0, outlier_share=0.0, depth=(2.0, 20.0), mirror=False, planar=False, K=EUROC):
    """dict(X1, X2 [n,3], model [13] the planted similarity, true_inlier bool [n]).  ``noise``: sigma of the Gaussian added
    to every coordinate of both sets, in units of each set's own scale per unit of depth (0.001: half a pixel at EuRoC's
    focal length); ``planar``: depths within 1e-3 of one plane; ``mirror``: X2 is the similarity of the MIRROR image of X1
    (x -> -x), which no proper rotation reproduces; an outlier's X2 is another random point in front of camera 2."""
    s, R, t = random_similarity(rng, scale)
    X1 = cloud(rng, n, depth, K)
    if planar:
        X1 = X1 / X1[:, 2:] * (8.0 + 1e-3 * rng.normal(size=(n, 1)))
    src = X1 * np.array([-1.0, 1.0, 1.0]) if mirror else X1
    X2 = s * (src @ R.T) + t
    if noise:
        X1 = X1 + rng.normal(0, noise, X1.shape) * X1[:, 2:]
        X2 = X2 + rng.normal(0, noise, X2.shape) * X2[:, 2:]
    out = rng.random(n) < outlier_share if outlier_share else np.zeros(n, bool)
    X2 = np.where(out[:, None], s * cloud(rng, n, depth, K), X2)
    return dict(X1=np.ascontiguousarray(X1), X2=np.ascontiguousarray(X2), model=pack(s, R, t), true_inlier=~out, K=K)


def integer_scene(rng, n):
    """Integer coordinates in both sets: X1 rounded at depths 100 - 1000, X2 the rounded similarity of it."""
    s, R, t = random_similarity(rng, 2.0)
    X1 = np.round(cloud(rng, n, (100.0, 1000.0)))
    X2 = np.round(s * (X1 @ R.T) + 50.0 * t)
    return dict(X1=X1, X2=X2, model=pack(s, R, 50.0 * t), true_inlier=np.ones(n, bool), K=EUROC)


def family_scenes():
    """name -> scene, 200 correspondences each; 'planted' families have a planted similarity that RANSAC must recover."""
    rng = np.random.default_rng(SEED + 1)
    fam = {}
    fam["general"] = make_scene(rng, 200, 1.3, 0.001)
    fam["near_planar"] = make_scene(rng, 200, 0.8, 0.001, planar=True)
    fam["distant"] = make_scene(rng, 200, 1.2, 0.001, depth=(200.0, 2000.0))
    for sc in (0.1, 1.0, 10.0):
        fam[f"scale_{sc:g}"] = make_scene(rng, 200, sc, 0.001)
    fam["mirror"] = make_scene(rng, 200, 1.1, 0.0, mirror=True)
    for share in (0.0, 0.3, 0.5):
        fam[f"outliers_{int(share * 100)}"] = make_scene(rng, 200, 1.5, 0.001, share)
    fam["integer"] = integer_scene(rng, 200)
    return fam


def min_angle_deg(P):
    """The smallest angle of a triangle [3,3]."""
    best = 180.0
    for i in range(3):
        a, b = P[(i + 1) % 3] - P[i], P[(i + 2) % 3] - P[i]
        c = (a @ b) / np.sqrt((a @ a) * (b @ b))
        best = min(best, float(np.degrees(np.arccos(np.clip(c, -1, 1)))))
    return best


def solver_samples(S=2000, seed=SEED):
    """S minimal samples, each with its own similarity (scale log-uniform in 0.1 - 10): (X1 [S,3,3], X2 [S,3,3], model [S,13]).
    A triangle whose smallest angle is under 5 degrees in either set is redrawn HERE; no sample is left out afterwards."""
    rng = np.random.default_rng(seed)
    X1, X2, models = np.zeros((S, 3, 3)), np.zeros((S, 3, 3)), np.zeros((S, 13))
    for i in range(S):
        while True:
            sc = make_scene(rng, 3, 10.0 ** rng.uniform(-1, 1))
            if min(min_angle_deg(sc["X1"]), min_angle_deg(sc["X2"])) >= MIN_ANGLE_DEG:
                break
        X1[i], X2[i], models[i] = sc["X1"], sc["X2"], sc["model"]
    return X1, X2, models


def family_samples(name, S=200):
    """Minimal samples drawn (with the RANSAC generator, seed 1) from a family scene; a triple with a planted outlier in it, or
    a triangle under 5 degrees, is redrawn."""
    sc = family_scenes()[name]
    n, X1, X2, h = len(sc["X1"]), [], [], 0
    while len(X1) < S:
        idx = draw_sample(1, h, n)
        h += 1
        if sc["true_inlier"][idx].all() and min(min_angle_deg(sc["X1"][idx]), min_angle_deg(sc["X2"][idx])) >= MIN_ANGLE_DEG:
            X1.append(sc["X1"][idx]); X2.append(sc["X2"][idx])
    return np.array(X1), np.array(X2), sc["model"]


def model_quantities(model, truth=None):
    """Worst values over models [S,13]: |R^T R - I| (Frobenius), |det R - 1|; against truth [S,13] or [13]: |s / s_true - 1|,
    |R - R_true| (Frobenius), |t - t_true| / (1 + |t_true|)."""
    s, R, t = split(np.asarray(model).reshape(-1, 13))
    q = dict(orthonormal=float(np.linalg.norm(np.swapaxes(R, 1, 2) @ R - np.eye(3), axis=(1, 2)).max()),
             det=float(np.abs(np.linalg.det(R) - 1).max()))
    if truth is not None:
        st, Rt, tt = split(np.broadcast_to(np.asarray(truth), np.asarray(model).reshape(-1, 13).shape))
        q["scale"] = float(np.abs(s / st - 1).max())
        q["rotation"] = float(np.linalg.norm(R - Rt, axis=(1, 2)).max())
        q["translation"] = float((np.linalg.norm(t - tt, axis=1) / (1 + np.linalg.norm(tt, axis=1))).max())
    return q


def refit_cloud(n, offset=0.0, seed=SEED):
    """A noisy cloud of n correspondences for the refit tests, both sets shifted by ``offset`` along every axis (1e4: a
    one-pass covariance loses eight digits there): dict(X1, X2, model)."""
    rng = np.random.default_rng(seed + 7 * n + (1 if offset else 0))
    sc = make_scene(rng, n, 1.7, 0.001)
    s, R, t = split(sc["model"])
    X1, X2 = sc["X1"] + offset, sc["X2"] + offset
    # the planted similarity in the shifted coordinates: X2' = s R (X1' - o) + t + o
    o = np.full(3, offset)
    return dict(X1=X1, X2=X2, model=pack(s, R, t + o - s * (R @ o)))


# ---------------------------------------------------------------- the refit in extended precision (the yardstick's truth)
def refit_longdouble(X1, X2, fix_scale=False):
    """The least-squares similarity with every sum and Horn's eigenproblem (cyclic Jacobi, 16 sweeps) in ``np.longdouble``
    (64-bit mantissa on x86-64: three digits beyond f64), rounded to f64 at the end: what numpy's and the twin's f64 results
    on a NOISY cloud are measured against, since the planted similarity is not the least-squares one there."""
    L = np.longdouble
    A, B = np.asarray(X1, L).reshape(-1, 3), np.asarray(X2, L).reshape(-1, 3)
    c1, c2 = A.sum(0) / L(len(A)), B.sum(0) / L(len(B))
    A, B = A - c1, B - c2
    S = A.T @ B                                           # Horn's S_ab = sum x1_a x2_b
    N = np.zeros((4, 4), L)
    N[0, 0] = S[0, 0] + S[1, 1] + S[2, 2]; N[1, 1] = S[0, 0] - S[1, 1] - S[2, 2]
    N[2, 2] = -S[0, 0] + S[1, 1] - S[2, 2]; N[3, 3] = -S[0, 0] - S[1, 1] + S[2, 2]
    N[0, 1] = S[1, 2] - S[2, 1]; N[0, 2] = S[2, 0] - S[0, 2]; N[0, 3] = S[0, 1] - S[1, 0]
    N[1, 2] = S[0, 1] + S[1, 0]; N[1, 3] = S[2, 0] + S[0, 2]; N[2, 3] = S[1, 2] + S[2, 1]
    N = N + np.triu(N, 1).T
    V = np.eye(4, dtype=L)
    for _ in range(16):
        for p in range(3):
            for q in range(p + 1, 4):
                if N[p, q] == 0:
                    continue
                th = (N[q, q] - N[p, p]) / (2 * N[p, q])
                t = (L(-1) if th < 0 else L(1)) / (abs(th) + np.sqrt(th * th + 1))
                c = 1 / np.sqrt(t * t + 1)
                J = np.eye(4, dtype=L)
                J[p, p] = J[q, q] = c; J[p, q] = t * c; J[q, p] = -t * c
                N, V = J.T @ N @ J, V @ J
    w, x, y, z = V[:, int(np.argmax(np.diag(N)))]
    n = np.sqrt(w * w + x * x + y * y + z * z)
    w, x, y, z = w / n, x / n, y / n, z / n
    R = np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]], L)
    s = L(1) if fix_scale else (R * S.T).sum() / (A * A).sum()
    t = c2 - s * (R @ c1)
    return pack(float(s), R.astype(np.float64), t.astype(np.float64))


# ---------------------------------------------------------------- exactly-stated cases
def exact_similarity(q, scale, t):
    """The similarity of an INTEGER quaternion q = (w, x, y, z), a Fraction scale and an integer translation, as Fractions:
    (s, R [3][3], t [3], N = |q|^2).  R = (integer matrix) / N, so s R X + t is exact in f64 for X a multiple of N / s."""
    from fractions import Fraction as F
    w, x, y, z = q
    N = w * w + x * x + y * y + z * z
    Ri = [[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
          [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
          [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]]
    return F(scale), [[F(v, N) for v in row] for row in Ri], [F(v) for v in t], N


def exact_cases():
    """List of dict(X1, X2 integer-valued f64 [n,3], s, R, t as Fractions): triples and clouds of 40 mapped by rational
    similarities (integer quaternion, scale 2 and 1/2, integer translation); X2 is computed in Fractions and is exact."""
    from fractions import Fraction as F
    rng = np.random.default_rng(SEED + 50)
    cases = []
    for q in ((1, 2, 2, 4), (3, 1, -1, 2), (5, -2, 1, 1), (2, 3, 6, 0)):
        for scale in (F(2), F(1, 2)):
            for n in (3, 40):
                t = [int(v) for v in rng.integers(-50, 51, 3)]
                s, R, tf, N = exact_similarity(q, scale, t)
                while True:
                    P = rng.integers(-20, 21, (n, 3))
                    if n > 3 or min_angle_deg(P.astype(np.float64)) >= MIN_ANGLE_DEG:
                        break
                X1 = [[int(v) * 2 * N for v in row] for row in P]
                X2 = [[s * sum(R[i][j] * row[j] for j in range(3)) + tf[i] for i in range(3)] for row in X1]
                assert all(v.denominator == 1 for row in X2 for v in row)
                cases.append(dict(X1=np.array(X1, np.float64), X2=np.array([[int(v) for v in row] for row in X2], np.float64),
                                  s=s, R=R, t=tf, n=n))
    return cases


def exact_errors(model, case):
    """(|s - s_exact|, max |R - R_exact|, max |t - t_exact| / (1 + max |t_exact|)) of a f64 model against the case's Fractions, the differences
    taken in Fractions (exact) and rounded once."""
    from fractions import Fraction as F
    s, R, t = split(np.asarray(model, np.float64))
    es = abs(float(F(float(s)) - case["s"]))
    eR = max(abs(float(F(float(R[i, j])) - case["R"][i][j])) for i in range(3) for j in range(3))
    tmax = max(abs(float(v)) for v in case["t"])
    et = max(abs(float(F(float(t[i])) - case["t"][i])) for i in range(3)) / (1 + tmax)
    return es, eR, et


def trajectory(n=200, seed=SEED + 60):
    """A 200-pose path (a random walk of 0.1 steps on a slow helix) and the planted similarity of it:
    dict(est [n,3], gt [n,3] = s R est + t, model)."""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    est = np.stack([2 * np.cos(0.05 * k), 2 * np.sin(0.05 * k), 0.01 * k], 1) + np.cumsum(rng.normal(0, 0.1, (n, 3)), 0)
    s, R, t = 0.37, rodrigues(rng.normal(size=3), 2.1), np.array([4.0, -2.0, 1.5])
    return dict(est=est, gt=s * (est @ R.T) + t, model=pack(s, R, t))
