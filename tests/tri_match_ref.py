"""numpy restatement of the epipolar node search and the new-map-point geometry of DESIGN.md 4m (ORBmatcher::
SearchForTriangulation, LocalMapping::CreateNewMapPoints).  Part A: the gates in f64 in the order the specification writes them
(numpy fuses nothing, so the doubles are the device's bit for bit), every side-1 row against every side-2 row with no grouped
index, then the one-to-one step and rotation histogram of 4k (``bow_match_ref``).  Part B on ANOTHER route: the null vector of
the DLT's 4x4 matrix by ``numpy.linalg.svd`` and plain vector algebra - what the device's Jacobi sweeps are compared against
within a tolerance."""
import numpy as np

import bow_match_ref as B
import proj_match_ref as PR

NONE_IDX, NONE_DIST = B.NONE_IDX, B.NONE_DIST
_BIG = np.int64(2**62)
scale_tables = PR.scale_tables


# ---- poses and cameras -----------------------------------------------------------------------------------------------------------

def centre(T):
    T = np.asarray(T, np.float64)[:3]
    return -T[:, :3].T @ T[:, 3]


def fundamental(T1, T2, camera):
    """F12 with x1^T F12 x2 = 0, from the definition: E12 = [t12]x R12 for x_c1 = R12 x_c2 + t12."""
    T1, T2 = np.asarray(T1, np.float64)[:3], np.asarray(T2, np.float64)[:3]
    fx, fy, cx, cy = camera
    R12 = T1[:, :3] @ T2[:, :3].T
    t12 = T1[:, 3] - R12 @ T2[:, 3]
    K = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
    Ki = np.linalg.inv(K)
    return Ki.T @ np.cross(np.eye(3), t12) @ R12 @ Ki        # row i of np.cross(I, t) is e_i x t: the rows of [t]x


def project(T, X, camera):
    """(pixels [n,2], depth [n]) of world points under T."""
    T, X = np.asarray(T, np.float64)[:3], np.asarray(X, np.float64).reshape(-1, 3)
    fx, fy, cx, cy = camera
    c = X @ T[:, :3].T + T[:, 3]
    return np.stack([fx * c[:, 0] / c[:, 2] + cx, fy * c[:, 1] / c[:, 2] + cy], 1), c[:, 2]


# ---- A: the gates ------------------------------------------------------------------------------------------------------------------

def epiline(F, xy1):
    """(a, b, c) f64 [n1] each: the line of every side-1 pixel in image 2, in the specification's order."""
    F = np.asarray(F, np.float64).reshape(9)
    x1, y1 = np.asarray(xy1, np.float32).reshape(-1, 2).astype(np.float64).T
    with np.errstate(all="ignore"):
        return (x1 * F[0] + y1 * F[3]) + F[6], (x1 * F[1] + y1 * F[4]) + F[7], (x1 * F[2] + y1 * F[5]) + F[8]


def gates(F, epipole, xy1, xy2, level2, scale, sigma2, chi2=3.84, epipole_r2=100.0):
    """(off_epipole bool [n2], on_line bool [n1, n2]) - gates 3 and 4 of the specification."""
    a, b, c = epiline(F, xy1)
    x2, y2 = np.asarray(xy2, np.float32).reshape(-1, 2).astype(np.float64).T
    scale, sigma2 = np.asarray(scale, np.float64), np.asarray(sigma2, np.float64)
    l = np.clip(np.asarray(level2, np.int64).reshape(-1), 0, len(scale) - 1)
    ex, ey = (np.float64(v) for v in epipole)
    with np.errstate(all="ignore"):
        dx, dy = ex - x2, ey - y2
        off = ~((dx * dx + dy * dy) < np.float64(epipole_r2) * scale[l])
        num = (a[:, None] * x2[None, :] + b[:, None] * y2[None, :]) + c[:, None]
        den = (a * a + b * b)[:, None]
        on = (den > 0) & (num * num < (np.float64(chi2) * sigma2[l])[None, :] * den)
    return off, on


def candidates(s1, s2, F, epipole, scale, sigma2, th_low=50, chi2=3.84, epipole_r2=100.0, rows=None):
    """(cand bool [n1, n2], hamming int64 [n1, n2]): conditions 1 to 4, for the side-1 rows ``rows`` (a slice; None: all).  A
    side is a dict desc, nodes, xy, level and optionally taken, bins."""
    rows = slice(None) if rows is None else rows
    nd1, nd2 = np.asarray(s1["nodes"], np.int64).reshape(-1)[rows], np.asarray(s2["nodes"], np.int64).reshape(-1)
    n1, n2 = len(nd1), len(nd2)
    free1 = np.ones(n1, bool) if s1.get("taken") is None else np.asarray(s1["taken"]).reshape(-1)[rows] == 0
    free2 = np.ones(n2, bool) if s2.get("taken") is None else np.asarray(s2["taken"]).reshape(-1) == 0
    d = PR.hamming(np.asarray(s1["desc"]).reshape(-1, 32)[rows], s2["desc"]) if n1 and n2 else np.zeros((n1, n2), np.int64)
    cand = (nd1[:, None] == nd2[None, :]) & (nd1[:, None] >= 0) & free1[:, None] & free2[None, :] & (d <= int(th_low))
    if n1 and n2:
        off, on = gates(F, epipole, np.asarray(s1["xy"]).reshape(-1, 2)[rows], s2["xy"], s2["level"], scale, sigma2, chi2, epipole_r2)
        cand &= off[None, :] & on
    return cand, d


def top2(cand, d):
    n1, n2 = cand.shape
    idx = np.full((n1, 2), NONE_IDX, np.int32)
    dist = np.full((n1, 2), NONE_DIST, np.int32)
    if n1 == 0 or n2 == 0:
        return idx, dist
    key = np.where(cand, d * (1 << 23) + np.arange(n2, dtype=np.int64)[None, :], _BIG)
    for k in range(2):
        j = key.argmin(1)
        best = key[np.arange(n1), j]
        has = best < _BIG
        idx[has, k] = j[has]
        dist[has, k] = best[has] >> 23
        key[np.arange(n1), j] = _BIG
    return idx, dist


def tables(s1, s2, F, epipole, scale, sigma2, th_low=50, chi2=3.84, epipole_r2=100.0):
    """(idx, dist) int32 [n1, 2] of one pair, in slabs of side-1 rows."""
    n1, n2 = len(np.asarray(s1["nodes"]).reshape(-1)), len(np.asarray(s2["nodes"]).reshape(-1))
    step = max(1, (1 << 20) // max(1, n2))
    parts = [top2(*candidates(s1, s2, F, epipole, scale, sigma2, th_low, chi2, epipole_r2, slice(s, min(n1, s + step))))
             for s in range(0, n1, step)]
    if not parts:
        return np.zeros((0, 2), np.int32), np.zeros((0, 2), np.int32)
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def search(s1, s2, F, epipole, scale, sigma2, th_low=50, chi2=3.84, epipole_r2=100.0):
    """One pair -> (matches12 int32 [n1], count, (idx, dist))."""
    idx, dist = tables(s1, s2, F, epipole, scale, sigma2, th_low, chi2, epipole_r2)
    m12 = B.one_to_one(idx, dist, idx[:, 0] >= 0, len(np.asarray(s2["nodes"]).reshape(-1)))
    if s1.get("bins") is not None and s2.get("bins") is not None:
        m12 = B.rotation_keep(m12, s1["bins"], s2["bins"])
    return m12, int((m12 >= 0).sum()), (idx, dist)


# ---- B: the geometry of one match, on the SVD route ----------------------------------------------------------------------------------

def triangulate_one(T1, T2, camera, scale, sigma2, p1, p2, l1, l2, cos_max=0.9998, chi2_px=5.991, ratio_factor=None, margins=None):
    """(status, X [3], normal [3], (dmin2, dmax2)) of one match; ``margins``: a list that receives, for every comparison made,
    the relative distance |lhs - rhs| / max(|lhs|, |rhs|) of the two sides."""
    T1, T2 = np.asarray(T1, np.float64)[:3], np.asarray(T2, np.float64)[:3]
    fx, fy, cx, cy = camera
    scale, sigma2 = np.asarray(scale, np.float64), np.asarray(sigma2, np.float64)
    L = len(scale)
    rf = 1.5 * (scale[1] if L > 1 else 1.0) if ratio_factor is None else ratio_factor
    l1, l2 = int(np.clip(l1, 0, L - 1)), int(np.clip(l2, 0, L - 1))
    nan3 = np.full(3, np.nan)

    def cmp(lhs, rhs):
        if margins is not None:
            margins.append(abs(lhs - rhs) / max(abs(lhs), abs(rhs), 1e-300))

    fail = lambda s: (s, nan3, nan3, (np.nan, np.nan))  # noqa: E731
    p1, p2 = np.asarray(p1, np.float32).astype(np.float64), np.asarray(p2, np.float32).astype(np.float64)
    xn1 = np.array([(p1[0] - cx) / fx, (p1[1] - cy) / fy, 1.0])
    xn2 = np.array([(p2[0] - cx) / fx, (p2[1] - cy) / fy, 1.0])
    r1, r2 = T1[:, :3].T @ xn1, T2[:, :3].T @ xn2
    cosv = r1 @ r2 / (np.linalg.norm(r1) * np.linalg.norm(r2))
    cmp(cosv, 0.0 if cosv <= 0 else cos_max)
    if not (cosv > 0 and cosv < cos_max):
        return fail(2)
    A = np.stack([xn1[0] * T1[2] - T1[0], xn1[1] * T1[2] - T1[1], xn2[0] * T2[2] - T2[0], xn2[1] * T2[2] - T2[1]])
    if not np.isfinite(A).all():
        return fail(3)
    v = np.linalg.svd(A)[2][3]
    if v[3] < 0:
        v = -v
    if not v[3] > 0 or not np.isfinite(v[:3] / v[3]).all():
        return fail(3)
    X = v[:3] / v[3]
    (u1, z1), (u2, z2) = project(T1, X, camera), project(T2, X, camera)
    cmp(z1[0], 0.0)
    if not z1[0] > 0:
        return fail(4)
    cmp(z2[0], 0.0)
    if not z2[0] > 0:
        return fail(5)
    e1, e2 = ((u1[0] - p1) ** 2).sum(), ((u2[0] - p2) ** 2).sum()
    cmp(e1, chi2_px * sigma2[l1])
    if e1 > chi2_px * sigma2[l1]:
        return fail(6)
    cmp(e2, chi2_px * sigma2[l2])
    if e2 > chi2_px * sigma2[l2]:
        return fail(7)
    O1, O2 = centre(T1), centre(T2)
    d1, d2 = np.linalg.norm(X - O1), np.linalg.norm(X - O2)
    if d1 == 0 or d2 == 0:
        return fail(8)
    rd, ro = d2 / d1, scale[l1] / scale[l2]
    cmp(rd * rf, ro)
    cmp(rd, ro * rf)
    if rd * rf < ro or rd > ro * rf:
        return fail(8)
    nr = (X - O1) / d1 + (X - O2) / d2
    dmax = d1 * scale[l1]
    dmin = dmax / scale[L - 1]
    return 0, X, nr / np.linalg.norm(nr), (dmin * dmin, dmax * dmax)


def triangulate(T1, T2, camera, scale, sigma2, xy1, xy2, level1, level2, matches12, margins=None, **kw):
    """All rows of one pair -> dict status int32 [n1], X, normal f64 [n1,3], dmin2, dmax2 f64 [n1]."""
    n1 = len(matches12)
    out = dict(status=np.ones(n1, np.int32), X=np.full((n1, 3), np.nan), normal=np.full((n1, 3), np.nan), dmin2=np.full(n1, np.nan),
               dmax2=np.full(n1, np.nan))
    n2 = len(np.asarray(level2).reshape(-1))
    for i, j in enumerate(np.asarray(matches12)):
        if not 0 <= j < n2:
            continue
        s, X, nr, (lo, hi) = triangulate_one(T1, T2, camera, scale, sigma2, xy1[i], xy2[j], level1[i], level2[j], margins=margins, **kw)
        out["status"][i], out["X"][i], out["normal"][i], out["dmin2"][i], out["dmax2"][i] = s, X, nr, lo, hi
    return out
