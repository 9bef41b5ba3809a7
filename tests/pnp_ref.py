"""numpy statement of the absolute-pose calls (slam_pnp_* of include/slamhip.h), written from the definitions.

Imports neither the product nor the twin.  The P3P solver here takes another route than the kernel: the kernel eliminates
u = s2 / s1 (linear in one difference of the law-of-cosines equations), finds the real roots of a quartic in v = s3 / s1 by
bracketing through its derivatives, polishes the depths on the equations and builds R from two Gram-Schmidt frames; this file
eliminates v instead (the two quadratics in v whose coefficients are polynomials in u, their resultant a quartic in u), takes
the roots from ``np.polynomial.polynomial.polyroots`` (companion-matrix eigenvalues), does not polish and aligns the two
triangles by Kabsch's SVD.  An agreement of the two is not an agreement of one piece of code with itself.

Conventions (as the header): world points X, pixels px, normalised x = ((u - cx) / fx, (v - cy) / fy), pose [R|t] with
X_cam = R X + t.

Also the scene generator of the tests: EuRoC intrinsics, 752 x 480 image, rotation of 1 - 20 degrees about a random axis, a
unit-length random translation, pixels uniform in the image, depth uniform in 2 - 20, world points R^T (Y - t)."""
from __future__ import annotations

import numpy as np
from numpy.polynomial import polynomial as P

import ransac_draws

EUROC = (458.654, 457.296, 367.215, 248.375)      # fx, fy, cx, cy
IMAGE = (752, 480)
MIN_ROTATION_DEG, MAX_ROTATION_DEG = 1.0, 20.0
MIN_DEPTH, MAX_DEPTH = 2.0, 20.0
SEED = 228
MASK64 = ransac_draws.MASK64
splitmix = ransac_draws.splitmix


# ---------------------------------------------------------------- scenes
def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    W = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * W + (1 - np.cos(angle)) * W @ W


def random_pose(rng):
    R = rodrigues(rng.normal(size=3), np.deg2rad(rng.uniform(MIN_ROTATION_DEG, MAX_ROTATION_DEG)))
    t = rng.normal(size=3)
    return R, t / np.linalg.norm(t)


def normalise(px, K=EUROC):
    px = np.asarray(px, np.float64)
    return np.stack([(px[..., 0] - K[2]) / K[0], (px[..., 1] - K[3]) / K[1]], -1)


def make_scene(rng, n, noise=0.0, outlier_share=0.0, K=EUROC):
    """n correspondences of one camera: dict(X [n,3], px [n,2], R, t, true_inlier bool [n])."""
    R, t = random_pose(rng)
    px = np.stack([rng.uniform(0, IMAGE[0], n), rng.uniform(0, IMAGE[1], n)], 1)
    depth = rng.uniform(MIN_DEPTH, MAX_DEPTH, n)
    x = normalise(px, K)
    Y = np.concatenate([x, np.ones((n, 1))], 1) * depth[:, None]
    X = (Y - t) @ R                                    # R^T (Y - t), row-wise
    px = px + rng.normal(0, noise, px.shape) if noise else px
    out = rng.random(n) < outlier_share if outlier_share else np.zeros(n, bool)
    px = np.where(out[:, None], np.stack([rng.uniform(0, IMAGE[0], n), rng.uniform(0, IMAGE[1], n)], 1), px)
    return dict(X=np.ascontiguousarray(X), px=np.ascontiguousarray(px), R=R, t=t, true_inlier=~out)


def make_samples(S, seed=SEED, K=EUROC):
    """S minimal samples, each with its own pose: (X [S,3,3], x [S,3,2] normalised, R [S,3,3], t [S,3])."""
    rng = np.random.default_rng(seed)
    X, x, Rs, ts = np.zeros((S, 3, 3)), np.zeros((S, 3, 2)), np.zeros((S, 3, 3)), np.zeros((S, 3))
    for s in range(S):
        sc = make_scene(rng, 3, K=K)
        X[s], x[s], Rs[s], ts[s] = sc["X"], normalise(sc["px"], K), sc["R"], sc["t"]
    return X, x, Rs, ts


def end_to_end_scenes():
    """The nine scenes of the end-to-end tests: 200 correspondences, 0.5 px noise, 0 / 30 / 50 % outliers."""
    return [(share, make_scene(np.random.default_rng(SEED + 1 + i), 200, 0.5, share)) for i, share in enumerate((0.0, 0.3, 0.5) * 3)]


# ---------------------------------------------------------------- the minimal solver
def kabsch(X, Y):
    """[R|t] with Y ~ R X + t for point sets [k,3], by SVD."""
    Xc, Yc = X.mean(0), Y.mean(0)
    U, _, Vt = np.linalg.svd((X - Xc).T @ (Y - Yc))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    return R, Yc - R @ Xc


def p3p_one(X, x):
    """All poses of one sample: (list of (R, t), the four roots of the quartic as complex numbers or None)."""
    with np.errstate(all="ignore"):
        f = np.concatenate([x, np.ones((3, 1))], 1)
        f = f / np.linalg.norm(f, axis=1)[:, None]
        a2, b2, c2 = ((X[1] - X[2]) ** 2).sum(), ((X[0] - X[2]) ** 2).sum(), ((X[0] - X[1]) ** 2).sum()
        ca, cb, cg = f[1] @ f[2], f[0] @ f[2], f[0] @ f[1]
        if not np.isfinite([a2, b2, c2, ca, cb, cg]).all() or min(a2, b2, c2) <= 0:
            return [], None
        G = np.array([1.0, -2 * cg, 1.0])                                    # u^2 + 1 - 2 u cg = c2 / s1^2
        p1, p0 = np.array([0.0, -2 * ca]), P.polysub([0.0, 0.0, 1.0], a2 / c2 * G)      # v^2 + p1 v + p0 = 0
        q1, q0 = np.array([-2 * cb]), P.polysub([1.0], b2 / c2 * G)                     # v^2 + q1 v + q0 = 0
        d0, d1 = P.polysub(p0, q0), P.polysub(p1, q1)
        res = P.polyadd(P.polysub(P.polymul(d0, d0), P.polymul(P.polymul(p1, d0), d1)), P.polymul(p0, P.polymul(d1, d1)))
        res = np.concatenate([res, np.zeros(5 - len(res))])[:5]
        if not np.isfinite(res).all() or res[4] == 0:
            return [], None
        roots = np.asarray(P.polyroots(res), complex)
        sols = []
        for r in roots:
            if r.imag != 0 or not r.real > 0:
                continue
            u = r.real
            v = -P.polyval(u, d0) / P.polyval(u, d1)
            g = P.polyval(u, G)
            if not (v > 0 and g > 0 and np.isfinite(v)):
                continue
            s1 = np.sqrt(c2 / g)
            Y = f * np.array([s1, u * s1, v * s1])[:, None]
            R, t = kabsch(X, Y)
            if np.isfinite(R).all() and np.isfinite(t).all():
                sols.append((v, R, t))
        sols.sort(key=lambda e: e[0])
        return [(R, t) for _, R, t in sols], roots


def p3p(X, x):
    """(pose [S,4,3,4], nsol int32 [S], root_gap [S]): root_gap = the smallest distance between two roots of the quartic
    (inf where there is no quartic)."""
    X, x = np.asarray(X, np.float64).reshape(-1, 3, 3), np.asarray(x, np.float64).reshape(-1, 3, 2)
    S = len(X)
    pose, n, gap = np.zeros((S, 4, 3, 4)), np.zeros(S, np.int32), np.full(S, np.inf)
    for s in range(S):
        sols, roots = p3p_one(X[s], x[s])
        for k, (R, t) in enumerate(sols[:4]):
            pose[s, k, :, :3], pose[s, k, :, 3] = R, t
        n[s] = min(len(sols), 4)
        if roots is not None and len(roots) > 1:
            gap[s] = min(abs(roots[i] - roots[j]) for i in range(len(roots)) for j in range(i))
    return pose, n, gap


def solver_quantities(pose, nsol, X, x, R_true=None, t_true=None):
    """Worst values over the samples: reprojection of the three sample points (normalised units) by any returned solution,
    |R^T R - I| (Frobenius), |det R - 1|; and per sample the error of the best solution against the true pose
    (max of |R - R_true| Frobenius and |t - t_true|; inf where there is no solution)."""
    q = dict(reprojection=0.0, orthonormal=0.0, det=0.0)
    best = np.full(len(X), np.inf)
    for s in range(len(X)):
        for k in range(nsol[s]):
            R, t = pose[s, k, :, :3], pose[s, k, :, 3]
            Y = X[s] @ R.T + t
            q["reprojection"] = max(q["reprojection"], np.abs(Y[:, :2] / Y[:, 2:] - x[s]).max())
            q["orthonormal"] = max(q["orthonormal"], np.linalg.norm(R.T @ R - np.eye(3)))
            q["det"] = max(q["det"], abs(np.linalg.det(R) - 1))
            if R_true is not None:
                best[s] = min(best[s], max(np.linalg.norm(R - R_true[s]), np.linalg.norm(t - t_true[s])))
    return q, best


# ---------------------------------------------------------------- draws, score, RANSAC (the header's statements)
def draw_sample(seed, h, n):
    """Three distinct indices of hypothesis h among n correspondences."""
    return ransac_draws.draw_sample(seed, h, n, 3)


def score(T, X, px, K, threshold):
    """The header's inlier rule, operation by operation: bool [n]."""
    T = np.asarray(T, np.float64).reshape(3, 4)
    X, px = np.asarray(X, np.float64).reshape(-1, 3), np.asarray(px, np.float64).reshape(-1, 2)
    fx, fy, cx, cy = K
    with np.errstate(all="ignore"):
        c = [((T[i, 0] * X[:, 0] + T[i, 1] * X[:, 1]) + T[i, 2] * X[:, 2]) + T[i, 3] for i in range(3)]
        du = (fx * (c[0] / c[2]) + cx) - px[:, 0]
        dv = (fy * (c[1] / c[2]) + cy) - px[:, 1]
        return (c[2] > 0.0) & ((du * du + dv * dv) < threshold * threshold)


def ransac(X, px, K, H, threshold, seed, solver=None):
    """slam_pnp_ransac_f64 for one candidate with the numpy solver (or ``solver(X3, x3) -> list of (R, t)``):
    (pose [3,4], mask bool [n], stats [4])."""
    X, px = np.asarray(X, np.float64).reshape(-1, 3), np.asarray(px, np.float64).reshape(-1, 2)
    n = len(X)
    solver = solver or (lambda A, a: p3p_one(A, a)[0])
    ident = np.eye(4)[:3].copy()
    if n < 3:
        return ident, np.zeros(n, bool), np.array([0, -1, -1, 0], np.int32)
    best, models = None, 0
    for h in range(H):
        idx = draw_sample(seed, h, n)
        sols = solver(X[idx], normalise(px[idx], K))[:4]
        models += len(sols)
        for r, (R, t) in enumerate(sols):
            T = np.concatenate([R, t[:, None]], 1)
            cnt = int(score(T, X, px, K, threshold).sum())
            if best is None or cnt > best[0]:
                best = (cnt, h, r, T)
    if best is None:
        return ident, np.zeros(n, bool), np.array([0, -1, -1, 0], np.int32)
    return best[3], score(best[3], X, px, K, threshold), np.array([best[0], best[1], best[2], models], np.int32)


def rotation_angle_deg(R, R_true):
    c = (np.trace(R.T @ R_true) - 1) / 2
    return float(np.rad2deg(np.arccos(np.clip(c, -1, 1))))


def pose_errors(T, sc):
    """(rotation angle in degrees, |t - t_true|) of a 3x4 pose against the scene's truth."""
    T = np.asarray(T).reshape(3, 4)
    return rotation_angle_deg(T[:, :3], sc["R"]), float(np.linalg.norm(T[:, 3] - sc["t"]))


# ---------------------------------------------------------------- edge families (shared by the CPU and the GPU edge tests)
def _exact_scene(rng, n, K=EUROC, plane=False, behind=0):
    """Noise-free scene whose pixels are the projection itself; ``plane``: coplanar world points; ``behind``: that many
    points mirrored behind the camera (their pixels still are their projections)."""
    sc = make_scene(rng, n, K=K)
    R, t = sc["R"], sc["t"]
    Y = sc["X"] @ R.T + t
    if plane:
        x = Y[:, :2] / Y[:, 2:]
        Y = np.concatenate([x, np.ones((n, 1))], 1) * (5.0 / (1.0 + 0.3 * x[:, :1] - 0.2 * x[:, 1:]))
    Y[:behind] *= -1.0
    X = (Y - t) @ R
    Yc = X @ R.T + t
    px = np.stack([K[0] * (Yc[:, 0] / Yc[:, 2]) + K[2], K[1] * (Yc[:, 1] / Yc[:, 2]) + K[3]], 1)
    return dict(X=np.ascontiguousarray(X), px=np.ascontiguousarray(px), R=R, t=t)


def edge_families():
    """name -> dict(X, px, K, H, expect): expect 'none' (the stated no-model answer), 'all' (a model with every
    correspondence an inlier) or 'model' (a model; 'front' / 'bad' then name the correspondences that must / must not vote)."""
    rng = np.random.default_rng(SEED + 100)
    fam = {}
    base = _exact_scene(rng, 40)
    for n in (0, 1, 2):
        fam[f"n{n}"] = dict(X=base["X"][:n], px=base["px"][:n], expect="none")
    for n in (3, 4):
        fam[f"n{n}"] = dict(X=base["X"][:n], px=base["px"][:n], expect="all")
    fam["identical"] = dict(X=np.tile(base["X"][:1], (10, 1)), px=np.tile(base["px"][:1], (10, 1)), expect="none")
    line = base["X"][0] + np.arange(10)[:, None] * np.array([0.25, -0.5, 0.125])
    fam["collinear"] = dict(X=line, px=base["px"][:10], expect="none")
    pl = _exact_scene(rng, 40, plane=True)
    fam["coplanar"] = dict(X=pl["X"], px=pl["px"], expect="all")
    c = _exact_scene(rng, 40)
    c["X"][:4] = -(c["R"].T @ c["t"])                                   # the camera centre: its projection is 0 / 0
    with np.errstate(all="ignore"):
        Yc = c["X"] @ c["R"].T + c["t"]
        Yc[:4] = 0.0
        c["px"] = np.stack([EUROC[0] * (Yc[:, 0] / Yc[:, 2]) + EUROC[2], EUROC[1] * (Yc[:, 1] / Yc[:, 2]) + EUROC[3]], 1)
    fam["centre"] = dict(X=c["X"], px=c["px"], expect="model", bad=np.arange(4))
    bh = _exact_scene(rng, 40, behind=12)
    fam["behind"] = dict(X=bh["X"], px=bh["px"], expect="model", bad=np.arange(12), front=np.arange(12, 40))
    for name, val in (("nan", np.nan), ("inf", np.inf), ("huge", 1e150)):
        s = _exact_scene(rng, 40)
        s["X"][0, 0] = val; s["X"][1, 2] = -val; s["px"][2, 0] = val; s["px"][3, 1] = -val; s["X"][4] = val; s["px"][4] = val
        fam[name] = dict(X=s["X"], px=s["px"], expect="model", bad=np.arange(5), front=np.arange(5, 40))
    fam["all_nan"] = dict(X=np.full((10, 3), np.nan), px=np.full((10, 2), np.nan), expect="none")
    it = make_scene(rng, 60, 0.0, 0.2)
    fam["integer_px"] = dict(X=it["X"], px=np.floor(it["px"]), expect="model", threshold=1.0)
    Ka = (EUROC[0] * 10.0, EUROC[1] / 100.0, EUROC[2], EUROC[3])
    an = _exact_scene(rng, 40, K=Ka)
    fam["anisotropic"] = dict(X=an["X"], px=an["px"], K=Ka, expect="all")
    fam["h1"] = dict(X=base["X"], px=base["px"], H=1, expect="all")
    for f in fam.values():
        f.setdefault("K", EUROC); f.setdefault("H", 32); f.setdefault("threshold", 8.0)
        f["X"], f["px"] = np.ascontiguousarray(f["X"], np.float64).reshape(-1, 3), np.ascontiguousarray(f["px"], np.float64).reshape(-1, 2)
    return fam


def solver_edge_samples():
    """(X [S,3,3], x [S,3,2]) on which the minimal solver must return no solution."""
    rng = np.random.default_rng(SEED + 200)
    X, x, _, _ = make_samples(12, SEED + 200)
    X[0, 1] = X[0, 0]; x[0, 1] = x[0, 0]                               # a repeated correspondence
    X[1, 2] = X[1, 1]                                                   # a repeated world point
    x[2, 2] = x[2, 0]                                                   # a repeated image point
    X[3, 2] = X[3, 0] + 3.0 * (X[3, 1] - X[3, 0])                       # collinear world points
    X[4] = X[4, 0]; x[4] = x[4, 0]                                      # all identical
    X[5, 0, 1] = np.nan; x[6, 1, 0] = np.nan; X[7, 2, 2] = np.inf; x[8, 0, 1] = -np.inf; X[9, 1, 0] = 1e150; x[10, 2, 1] = 1e150
    x[11, 0] = np.nan                                                   # a point at the camera centre projects to 0 / 0
    return X, x


def check_candidate(fam, pose, mask, stats):
    """The contract every edge family is held to, whoever computed (pose, mask, stats)."""
    n = len(fam["X"])
    assert pose.shape == (3, 4) and np.isfinite(pose).all() and mask.shape == (n,)
    if fam["expect"] == "none":
        assert np.array_equal(pose, np.eye(4)[:3]) and not mask.any() and list(stats) == [0, -1, -1, 0]
        return
    assert 0 <= stats[1] < fam["H"] and 0 <= stats[2] < 4 and stats[3] >= 1, list(stats)
    assert stats[0] == mask.sum() and np.array_equal(mask, score(pose, fam["X"], fam["px"], fam["K"], fam["threshold"]))
    R = pose[:, :3]
    assert np.linalg.norm(R.T @ R - np.eye(3)) < 1e-13 and abs(np.linalg.det(R) - 1) < 1e-13
    if fam["expect"] == "all":
        assert mask.all()
    if "bad" in fam:
        assert not mask[fam["bad"]].any()
    if "front" in fam:
        assert mask[fam["front"]].all()
