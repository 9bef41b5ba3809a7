"""numpy statement of the two-view geometry calls (slam_tv_* of include/slamhip.h), written from the definitions.

Imports neither the product nor the oracle.  The five-point solver here takes the action-matrix route (Stewenius: SVD null
space, the ten cubic constraints as a 10x20 system, ``np.linalg.solve`` for the reduced block, eigenvectors of the 10x10
matrix of "multiply by z"); the kernel takes the other one (Householder null space, Gauss-Jordan with row pivoting, a
degree-10 polynomial in z whose real roots are bracketed through its derivatives), so an agreement of the two is not an
agreement of one piece of code with itself.

Conventions (as the header): points 1 = source / last frame, points 2 = query / current frame, normalised
x = ((u - cx) / fx, (v - cy) / fy, 1), x2^T E x1 = 0, X2 = R X1 + t, |t| = 1.

Also the scene generator of the tests: EuRoC intrinsics, 752 x 480 image, rotation of 1 - 20 degrees about a random axis,
unit baseline, points at depth 2 - 20 in front of both cameras, optional pixel noise and uniform outliers."""
from __future__ import annotations

import numpy as np

EUROC = (458.654, 457.296, 367.215, 248.375)      # fx, fy, cx, cy
IMAGE = (752, 480)
MIN_ROTATION_DEG, MAX_ROTATION_DEG = 1.0, 20.0
MIN_DEPTH, MAX_DEPTH = 2.0, 20.0

# ---------------------------------------------------------------- polynomials in (x, y, z), total degree <= 3
_MONO = [(i, j, k) for d in range(4) for i in range(d, -1, -1) for j in range(d - i, -1, -1) for k in [d - i - j]]
_BY_DEG = {d: [m for m in _MONO if sum(m) <= d] for d in range(4)}
# Stewenius' column order: the ten cubic monomials, then the basis of the quotient ring
_COLS = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3),
         (2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]


def _pmul(a, b, da, db):
    """Product of polynomial batches a, b [S,4,4,4] of total degree da, db (da + db <= 3)."""
    out = np.zeros_like(a)
    for (i, j, k) in _BY_DEG[da]:
        for (p, q, r) in _BY_DEG[db]:
            out[:, i + p, j + q, k + r] += a[:, i, j, k] * b[:, p, q, r]
    return out


def null_space(x1, x2):
    """Orthonormal basis [S,4,9] of the null space of the 5x9 epipolar system (rows kron(x2, x1)), by SVD."""
    x1 = np.asarray(x1, np.float64).reshape(-1, 5, 2)
    x2 = np.asarray(x2, np.float64).reshape(-1, 5, 2)
    h1 = np.concatenate([x1, np.ones(x1.shape[:2] + (1,))], -1)
    h2 = np.concatenate([x2, np.ones(x2.shape[:2] + (1,))], -1)
    A = (h2[:, :, :, None] * h1[:, :, None, :]).reshape(-1, 5, 9)           # row = x2_i * x1_j at 3i + j
    return np.linalg.svd(A)[2][:, 5:, :]


def fivepoint(x1, x2):
    """All real essential matrices through five correspondences, per sample.

    x1, x2 [S,5,2] normalised.  Returns (E [S,10,9], nroots [S], z [S,10]): E with Frobenius norm 1 in ascending order
    of the root variable z (this function's own z: the coefficient of the third null-space vector over the fourth),
    unused slots zero / NaN."""
    N = null_space(x1, x2)
    S = N.shape[0]
    Ep = np.zeros((S, 3, 3, 4, 4, 4))                                        # E = x N0 + y N1 + z N2 + N3, entrywise
    for c, m in enumerate([(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]):
        Ep[(slice(None), slice(None), slice(None)) + m] = N[:, c].reshape(S, 3, 3)
    rows = []
    det = np.zeros((S, 4, 4, 4))
    for (a, b, c, s) in [(0, 1, 2, 1), (0, 2, 1, -1), (1, 2, 0, 1), (1, 0, 2, -1), (2, 0, 1, 1), (2, 1, 0, -1)]:
        det += s * _pmul(_pmul(Ep[:, 0, a], Ep[:, 1, b], 1, 1), Ep[:, 2, c], 2, 1)
    rows.append(det)
    EEt = np.zeros((S, 3, 3, 4, 4, 4))
    for i in range(3):
        for j in range(3):
            for k in range(3):
                EEt[:, i, j] += _pmul(Ep[:, i, k], Ep[:, j, k], 1, 1)
    tr = EEt[:, 0, 0] + EEt[:, 1, 1] + EEt[:, 2, 2]
    for i in range(3):
        EEt[:, i, i] -= 0.5 * tr
    for i in range(3):
        for j in range(3):
            r = np.zeros((S, 4, 4, 4))
            for k in range(3):
                r += _pmul(EEt[:, i, k], Ep[:, k, j], 2, 1)
            rows.append(r)
    M = np.stack([np.stack([r[(slice(None),) + m] for m in _COLS], -1) for r in rows], 1)   # [S,10,20]
    E = np.zeros((S, 10, 9))
    zs = np.full((S, 10), np.nan)
    nroots = np.zeros(S, np.int32)
    try:
        B = np.linalg.solve(M[:, :, :10], M[:, :, 10:])
        singular = np.zeros(S, bool)
    except np.linalg.LinAlgError:
        B = np.zeros((S, 10, 10))
        singular = np.zeros(S, bool)
        for s in range(S):
            try:
                B[s] = np.linalg.solve(M[s, :, :10], M[s, :, 10:])
            except np.linalg.LinAlgError:
                singular[s] = True
    singular |= ~np.isfinite(B).all((1, 2))
    B[singular] = 0.0
    Act = np.zeros((S, 10, 10))
    for i, r in enumerate([2, 4, 5, 7, 8, 9]):                               # z * (x^2, xy, xz, y^2, yz, z^2) are cubics
        Act[:, i] = -B[:, r]
    for i, c in [(6, 2), (7, 4), (8, 5), (9, 8)]:                            # z * (x, y, z, 1) = (xz, yz, z^2, z)
        Act[:, i, c] = 1.0
    w, V = np.linalg.eig(Act)
    for s in range(S):
        if singular[s]:
            continue
        real = np.flatnonzero(w[s].imag == 0)
        real = real[np.argsort(w[s].real[real], kind="stable")]
        n = 0
        for r in real:
            v = V[s, :, r].real
            if v[9] == 0 or not np.isfinite(v).all():
                continue
            xyz1 = np.array([v[6] / v[9], v[7] / v[9], v[8] / v[9], 1.0])
            e = xyz1 @ N[s]
            nrm = np.linalg.norm(e)
            if not np.isfinite(nrm) or nrm == 0:
                continue
            E[s, n] = e / nrm
            zs[s, n] = w[s].real[r]
            n += 1
        nroots[s] = n
    return E, nroots, zs


# ---------------------------------------------------------------- scoring
def normalise(px, K):
    fx, fy, cx, cy = K
    px = np.asarray(px, np.float64).reshape(-1, 2)
    return np.stack([(px[:, 0] - cx) / fx, (px[:, 1] - cy) / fy], 1)


def sampson_sq(E, x1, x2):
    """Squared Sampson distance of x2^T E x1 = 0 in normalised coordinates, operation by operation as the header states it."""
    E = np.asarray(E, np.float64).reshape(9)
    a, b = x1[:, 0], x1[:, 1]
    c, d = x2[:, 0], x2[:, 1]
    l0 = E[0] * a + E[1] * b + E[2]                     # E x1
    l1 = E[3] * a + E[4] * b + E[5]
    l2 = E[6] * a + E[7] * b + E[8]
    m0 = E[0] * c + E[3] * d + E[6]                     # E^T x2
    m1 = E[1] * c + E[4] * d + E[7]
    r = c * l0 + d * l1 + l2
    with np.errstate(divide="ignore", invalid="ignore"):
        return r * r / (l0 * l0 + l1 * l1 + m0 * m0 + m1 * m1)


def threshold_sq(threshold_px, K):
    t = threshold_px / ((K[0] + K[1]) / 2)
    return t * t


# ---------------------------------------------------------------- the draw generator (header comment of slam_tv_essential_ransac_f64)
_M64 = (1 << 64) - 1


def _splitmix(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def draw_word(seed, h, d):
    return _splitmix(_splitmix((seed & _M64) ^ ((h * 0xD1B54A32D192ED03) & _M64)) ^ ((d * 0x8CB92BA72F3D8DD7) & _M64))


def draw_sample(seed, b, h, n):
    """The five distinct match indices of hypothesis h of a pair of n >= 5 matches.  The pair index b is accepted and
    deliberately unused: a pair's draws, and so its result, do not depend on where in a batch it stands."""
    out, d = [], 0
    while len(out) < 5:
        i = ((draw_word(seed, h, d) >> 32) * n) >> 32
        d += 1
        if i not in out:
            out.append(int(i))
    return out


# ---------------------------------------------------------------- RANSAC, pose, triangulation
def ransac(px1, px2, K, hypotheses=256, threshold=1.0, seed=0, b=0, band=0.0):
    """(E [9], mask, stats [4]) as slam_tv_essential_ransac_f64 defines them, with this module's solver."""
    x1, x2 = normalise(px1, K), normalise(px2, K)
    n = len(x1)
    if n < 5:
        return np.zeros(9), np.zeros(n, bool), np.array([0, -1, -1, 0])
    idx = np.array([draw_sample(seed, b, h, n) for h in range(hypotheses)])
    E, nr, _ = fivepoint(x1[idx], x2[idx])
    t2 = threshold_sq(threshold, K)
    best = (-1, -1, -1)
    models = 0
    for h in range(hypotheses):
        for r in range(nr[h]):
            models += 1
            cnt = int((sampson_sq(E[h, r], x1, x2) < t2).sum())
            if cnt > best[0]:
                best = (cnt, h, r)
    if best[1] < 0:
        return np.zeros(9), np.zeros(n, bool), np.array([0, -1, -1, models])
    Eb = E[best[1], best[2]]
    return Eb, sampson_sq(Eb, x1, x2) < t2, np.array([best[0], best[1], best[2], models])


def decompose(E):
    """(R1, R2, t): E = U diag(s1, s2, 0) V^T with det U = det V = +1 (the third columns carry no weight, so they take the
    sign that makes it so), R1 = U W V^T, R2 = U W^T V^T, t = the unit left null vector of E with its largest component
    (first of equals) positive."""
    U, _, Vt = np.linalg.svd(np.asarray(E, np.float64).reshape(3, 3))
    if np.linalg.det(U) < 0:
        U[:, 2] = -U[:, 2]
    if np.linalg.det(Vt) < 0:
        Vt[2] = -Vt[2]
    W = np.array([[0.0, 1, 0], [-1, 0, 0], [0, 0, 1]])
    t = U[:, 2].copy()
    if t[np.argmax(np.abs(t))] < 0:
        t = -t
    return U @ W @ Vt, U @ W.T @ Vt, t


def triangulate(P1, P2, x1, x2):
    """(X [N,3], w [N]): right singular vector of the smallest singular value of the 4x4 DLT matrix, |v| = 1, v[3] >= 0."""
    P1, P2 = np.asarray(P1, np.float64).reshape(3, 4), np.asarray(P2, np.float64).reshape(3, 4)
    x1, x2 = np.asarray(x1, np.float64).reshape(-1, 2), np.asarray(x2, np.float64).reshape(-1, 2)
    A = dlt_matrix(P1, P2, x1, x2)
    v = np.linalg.svd(A)[2][:, 3, :] if len(A) else np.zeros((0, 4))
    v = v * np.where(v[:, 3:4] < 0, -1.0, 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return v[:, :3] / v[:, 3:4], v[:, 3]


def dlt_matrix(P1, P2, x1, x2):
    return np.stack([x1[:, 0:1] * P1[2] - P1[0], x1[:, 1:2] * P1[2] - P1[1],
                     x2[:, 0:1] * P2[2] - P2[0], x2[:, 1:2] * P2[2] - P2[1]], 1)


def triangulate_eig(P1, P2, x1, x2):
    """The same through the eigenvectors of A^T A (the kernel's route), for the tolerance of the triangulation test."""
    A = dlt_matrix(np.asarray(P1, np.float64).reshape(3, 4), np.asarray(P2, np.float64).reshape(3, 4), x1, x2)
    v = np.linalg.eigh(np.swapaxes(A, 1, 2) @ A)[1][:, :, 0]
    v = v * np.where(v[:, 3:4] < 0, -1.0, 1.0)
    return v[:, :3] / v[:, 3:4], v[:, 3]


def recover_pose(E, px1, px2, K, inlier=None, distance_thresh=50.0):
    """(R, t, mask, stats [2]) as slam_tv_recover_pose_f64: most points with depth in (0, distance_thresh) in both
    cameras among the candidates (R1,t), (R2,t), (R1,-t), (R2,-t), ties to the lower index."""
    x1, x2 = normalise(px1, K), normalise(px2, K)
    inlier = np.ones(len(x1), bool) if inlier is None else np.asarray(inlier, bool)
    if not np.any(np.asarray(E)):
        return np.eye(3), np.zeros(3), np.zeros(len(x1), bool), np.array([0, -1])
    R1, R2, t = decompose(E)
    P1 = np.hstack([np.eye(3), np.zeros((3, 1))])
    best = None
    for c, (R, tt) in enumerate([(R1, t), (R2, t), (R1, -t), (R2, -t)]):
        P2 = np.hstack([R, tt[:, None]])
        X, _ = triangulate(P1, P2, x1, x2)
        z1 = X[:, 2]
        z2 = X @ R[2] + tt[2]
        with np.errstate(invalid="ignore"):
            good = inlier & (z1 > 0) & (z1 < distance_thresh) & (z2 > 0) & (z2 < distance_thresh)
        if best is None or good.sum() > best[0]:
            best = (int(good.sum()), c, R, tt, good)
    return best[2], best[3], best[4], np.array([best[0], best[1]])


def essential_from_pose(R, t):
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E = tx @ R
    return (E / np.linalg.norm(E)).reshape(9)


def rotation_angle_deg(Ra, Rb):
    return float(np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1))))


def direction_angle_deg(a, b):
    return float(np.degrees(np.arccos(np.clip(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)), -1, 1))))


# ---------------------------------------------------------------- scenes
def _rodrigues(axis, angle):
    a = axis / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def make_scene(rng, n, noise_px=0.0, outlier_share=0.0, K=EUROC):
    """One frame pair: dict with px1, px2 [n,2], R, t (X2 = R X1 + t, |t| = 1), E (Frobenius 1), X [n,3] in frame 1,
    true_inlier [n].  Points are drawn in camera 1 (uniform pixel, depth 2 - 20) and kept when they land inside the
    image of camera 2 at depth 2 - 20 as well; outliers replace px2 by a uniform pixel."""
    fx, fy, cx, cy = K
    R = _rodrigues(rng.normal(size=3), np.radians(rng.uniform(MIN_ROTATION_DEG, MAX_ROTATION_DEG)))
    t = rng.normal(size=3)
    t /= np.linalg.norm(t)
    X = np.zeros((0, 3))
    while len(X) < n:
        m = 4 * n
        u, v = rng.uniform(0, IMAGE[0], m), rng.uniform(0, IMAGE[1], m)
        z = rng.uniform(MIN_DEPTH, MAX_DEPTH, m)
        P = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
        Q = P @ R.T + t
        u2, v2 = fx * Q[:, 0] / Q[:, 2] + cx, fy * Q[:, 1] / Q[:, 2] + cy
        ok = (Q[:, 2] > MIN_DEPTH) & (Q[:, 2] < MAX_DEPTH) & (u2 >= 0) & (u2 < IMAGE[0]) & (v2 >= 0) & (v2 < IMAGE[1])
        X = np.concatenate([X, P[ok]])
    X = X[:n]
    Q = X @ R.T + t
    px1 = np.stack([fx * X[:, 0] / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy], 1)
    px2 = np.stack([fx * Q[:, 0] / Q[:, 2] + cx, fy * Q[:, 1] / Q[:, 2] + cy], 1)
    if noise_px > 0:
        px1 = px1 + rng.normal(0, noise_px, px1.shape)
        px2 = px2 + rng.normal(0, noise_px, px2.shape)
    true_inlier = np.ones(n, bool)
    n_out = int(round(outlier_share * n))
    if n_out:
        bad = rng.choice(n, n_out, replace=False)
        px2[bad] = np.stack([rng.uniform(0, IMAGE[0], n_out), rng.uniform(0, IMAGE[1], n_out)], 1)
        true_inlier[bad] = False
    return dict(px1=px1, px2=px2, R=R, t=t, E=essential_from_pose(R, t), X=X, true_inlier=true_inlier)


def make_samples(seed, S, noise_px=0.0, K=EUROC):
    """S five-point samples, each from a scene of its own: (x1 [S,5,2], x2 [S,5,2] normalised, E_gt [S,9])."""
    rng = np.random.default_rng(seed)
    x1, x2, Eg = np.zeros((S, 5, 2)), np.zeros((S, 5, 2)), np.zeros((S, 9))
    for s in range(S):
        sc = make_scene(rng, 5, noise_px, 0.0, K)
        x1[s], x2[s], Eg[s] = normalise(sc["px1"], K), normalise(sc["px2"], K), sc["E"]
    return x1, x2, Eg


def solver_quantities(E, nroots, x1, x2, E_gt=None):
    """Worst values over all returned roots of a batch: |x2^T E x1| on the sample's five points, the trace constraint's
    norm, |det E|, | |E|_F - 1 |; and per sample the completeness error min over roots of min(|E - E_gt|, |E + E_gt|)."""
    S = len(nroots)
    epi = cubic = det = fro = 0.0
    comp = np.full(S, np.inf)
    h1 = np.concatenate([x1, np.ones((S, 5, 1))], -1)
    h2 = np.concatenate([x2, np.ones((S, 5, 1))], -1)
    for s in range(S):
        for r in range(nroots[s]):
            M = E[s, r].reshape(3, 3)
            epi = max(epi, float(np.abs(np.einsum("ni,ij,nj->n", h2[s], M, h1[s])).max()))
            G = M @ M.T
            cubic = max(cubic, float(np.linalg.norm(2 * G @ M - np.trace(G) * M)))
            det = max(det, abs(float(np.linalg.det(M))))
            fro = max(fro, abs(float(np.linalg.norm(M)) - 1))
            if E_gt is not None:
                comp[s] = min(comp[s], np.linalg.norm(E[s, r] - E_gt[s]), np.linalg.norm(E[s, r] + E_gt[s]))
    return dict(epipolar=epi, cubic=cubic, det=det, frobenius=fro), comp
