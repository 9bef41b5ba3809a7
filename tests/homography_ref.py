"""numpy statement of the homography calls (slam_hg_* of include/slamhip.h), written from the definitions by another route
than the kernel's: the four-point solver is ``np.linalg.svd`` of the 8x9 DLT matrix of Hartley-normalised points (the kernel:
a closed form in cofactors), the decomposition takes ``np.linalg.svd`` of ``K^-1 H K`` and Ma et al.'s matrices W U^T as
they stand (the kernel: Jacobi eigenvectors of Hn^T Hn and re-orthonormalised frames), the vote triangulates with
``two_view_ref.triangulate`` (SVD), and the scores are float sums beside the fixed-point rule.

Imports neither the product nor the oracle.  The scene families come from tests/two_view_ref.py; added here is only what is
missing there: planar scenes with pixel noise and outliers, and four-point samples."""
from __future__ import annotations

import numpy as np

import ransac_draws
import two_view_ref as ref

EUROC = ref.EUROC
FLAT = 1e-20
ROTATION_ONLY = 1e-9
CHI2_H, CHI2_E, FIXED = 5.991, 3.841, 1048576.0


# ---------------------------------------------------------------- the four-point solver
def _hartley(p):
    c = p.mean(0)
    d = np.sqrt(((p - c) ** 2).sum(1)).mean()
    s = np.sqrt(2.0) / d
    return (p - c) * s, np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])


def _triangle(p, i, j, k):
    """(twice the signed area, flat) of the triangle (p_i, p_j, p_k): flat if sin^2 of any angle is below FLAT."""
    u, v, w = p[j] - p[i], p[k] - p[i], p[k] - p[j]
    cr = u[0] * v[1] - u[1] * v[0]
    lu, lv, lw = u @ u, v @ v, w @ w
    flat = not (cr * cr > FLAT * lu * lv and cr * cr > FLAT * lu * lw and cr * cr > FLAT * lv * lw)
    return cr, flat


def sample_ok(p1, p2):
    """The header's no-model rules on one sample p1, p2 [4,2]: finite and below 1e100, no flat triangle, no triangle turned over."""
    p1, p2 = np.asarray(p1, np.float64), np.asarray(p2, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        if not ((p1 ** 2).sum() + (p2 ** 2).sum() < 1e200):
            return False
    n1, n2 = _hartley(p1)[0], _hartley(p2)[0]
    if not (np.isfinite(n1).all() and np.isfinite(n2).all()):
        return False
    for (i, j, k) in ((1, 2, 3), (2, 0, 3), (0, 1, 3), (0, 1, 2)):
        a, fa = _triangle(n1, i, j, k)
        b, fb = _triangle(n2, i, j, k)
        if fa or fb or not a * b > 0:
            return False
    return True


def fourpoint(p1, p2):
    """H [9] with p2 ~ H p1 through four correspondences p1, p2 [4,2]: Frobenius norm 1, positive projective weights at the
    sample.  Returns (H, ok, conditioning) with conditioning = s7 / s0 of the normalised 8x9 system (small: ill-conditioned)."""
    p1, p2 = np.asarray(p1, np.float64).reshape(4, 2), np.asarray(p2, np.float64).reshape(4, 2)
    if not sample_ok(p1, p2):
        return np.zeros(9), False, 0.0
    a, T1 = _hartley(p1)
    b, T2 = _hartley(p2)
    A = np.zeros((8, 9))
    for k in range(4):
        x, y, u, v = a[k, 0], a[k, 1], b[k, 0], b[k, 1]
        A[2 * k] = [-x, -y, -1, 0, 0, 0, u * x, u * y, u]
        A[2 * k + 1] = [0, 0, 0, -x, -y, -1, v * x, v * y, v]
    _, s, Vt = np.linalg.svd(A)
    H = np.linalg.inv(T2) @ Vt[8].reshape(3, 3) @ T1
    H = H / np.linalg.norm(H)
    w = np.c_[p1, np.ones(4)] @ H[2]
    if w.sum() < 0:
        H, w = -H, -w
    if not (w > 0).all():
        return np.zeros(9), False, float(s[7] / s[0])
    return H.reshape(9), True, float(s[7] / s[0])


def transfer(H, p):
    H = np.asarray(H, np.float64).reshape(3, 3)
    q = np.c_[p, np.ones(len(p))] @ H.T
    with np.errstate(divide="ignore", invalid="ignore"):
        return q[:, :2] / q[:, 2:3]


def homography_from_pose(R, t, plane, K=EUROC):
    """H in pixels of the plane (n, d) (n . X1 = d) under X2 = R X1 + t, Frobenius norm 1, positive weights."""
    n, d = plane
    fx, fy, cx, cy = K
    Km = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    H = Km @ (R + np.outer(t, n) / d) @ np.linalg.inv(Km)
    return (H / np.linalg.norm(H)).reshape(9)


def common_distance(Ha, Hb):
    """|Ha - Hb| after both are scaled to Frobenius norm 1 and Hb takes the sign nearer to Ha."""
    a, b = np.asarray(Ha).reshape(9), np.asarray(Hb).reshape(9)
    a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
    return float(min(np.linalg.norm(a - b), np.linalg.norm(a + b)))


# ---------------------------------------------------------------- scoring, sampling, RANSAC
def inlier_mask(H, px1, px2, threshold):
    """The header's formula, operation by operation."""
    h = np.asarray(H, np.float64).reshape(9)
    x, y, u, v = px1[:, 0], px1[:, 1], px2[:, 0], px2[:, 1]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        w = (h[6] * x + h[7] * y) + h[8]
        du = ((h[0] * x + h[1] * y) + h[2]) / w - u
        dv = ((h[3] * x + h[4] * y) + h[5]) / w - v
        return (w > 0) & (du * du + dv * dv < threshold * threshold)


def draw_sample(seed, h, n):
    """The four distinct match indices of hypothesis h of a pair of n >= 4 matches."""
    return ransac_draws.draw_sample(seed, h, n, 4)


def ransac(px1, px2, hypotheses=256, threshold=3.0, seed=0):
    """(H [9], mask, stats [4]) as slam_hg_ransac_f64 defines them, with this module's solver."""
    px1, px2 = np.asarray(px1, np.float64).reshape(-1, 2), np.asarray(px2, np.float64).reshape(-1, 2)
    n = len(px1)
    if n < 4:
        return np.zeros(9), np.zeros(n, bool), np.array([0, -1, -1, 0])
    best, models = (-1, -1, None), 0
    for h in range(hypotheses):
        idx = draw_sample(seed, h, n)
        H, ok, _ = fourpoint(px1[idx], px2[idx])
        if not ok:
            continue
        models += 1
        cnt = int(inlier_mask(H, px1, px2, threshold).sum())
        if cnt > best[0]:
            best = (cnt, h, H)
    if best[1] < 0:
        return np.zeros(9), np.zeros(n, bool), np.array([0, -1, -1, models])
    return best[2], inlier_mask(best[2], px1, px2, threshold), np.array([best[0], best[1], 0, models])


# ---------------------------------------------------------------- decomposition
def _fix_sign(a):
    return -a if a[np.argmax(np.abs(a))] < 0 else a


def normalised_homography(H, K):
    fx, fy, cx, cy = K
    Km = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    return np.linalg.inv(Km) @ np.asarray(H, np.float64).reshape(3, 3) @ Km


def decompose(H, K, px1, px2, inlier=None, distance_thresh=50.0, bound=ROTATION_ONLY):
    """dict(pose_all [4,3,4], normal_all [4,3], count [4], pose [3,4], sv [3], good [n], stats [4], spread) as
    slam_hg_decompose_f64 defines them."""
    x1, x2 = ref.normalise(px1, K), ref.normalise(px2, K)
    n = len(x1)
    sel = np.ones(n, bool) if inlier is None else np.asarray(inlier, bool)
    out = dict(pose_all=np.zeros((4, 3, 4)), normal_all=np.zeros((4, 3)), count=np.zeros(4, int), pose=np.eye(3, 4), sv=np.zeros(3),
               good=np.zeros(n, bool), stats=np.array([0, -1, 0, 0]), spread=np.nan)
    Hm = np.asarray(H, np.float64).reshape(3, 3)
    if not np.isfinite(Hm).all() or not np.any(Hm):
        return out
    Hn = normalised_homography(Hm, K)
    _, s, Vt = np.linalg.svd(Hn)
    if not (s[1] > 0):
        return out
    out["sv"], out["spread"] = s, (s[0] - s[2]) / s[1]
    Hs = Hn / s[1]
    r = np.einsum("ni,ij,nj->n", np.c_[x2, np.ones(n)], Hs, np.c_[x1, np.ones(n)])[sel]
    if (r < 0).sum() > (r > 0).sum():
        Hs = -Hs
    if out["spread"] < bound:
        U, _, Wt = np.linalg.svd(Hs)
        R = U @ np.diag([1, 1, np.linalg.det(U @ Wt)]) @ Wt
        out["pose"] = np.c_[R, np.zeros(3)]
        out["pose_all"][0] = out["pose"]
        out["stats"] = np.array([0, -2, 0, 1])
        return out
    v1, v3 = _fix_sign(Vt[0]), _fix_sign(Vt[2])
    v2 = np.cross(v3, v1)
    s1, s3 = s[0] / s[1], s[2] / s[1]
    a, b = np.sqrt(max(1 - s3 * s3, 0.0)), np.sqrt(max(s1 * s1 - 1, 0.0))
    for c, bs in enumerate((b, -b)):
        u = a * v1 + bs * v3
        u /= np.linalg.norm(u)
        nv = np.cross(v2, u)
        U = np.stack([v2, u, nv], 1)
        W = np.stack([Hs @ v2, Hs @ u, np.cross(Hs @ v2, Hs @ u)], 1)
        R = W @ U.T
        t = (Hs - R) @ nv
        t /= np.linalg.norm(t)
        if nv[np.argmax(np.abs(nv))] < 0:
            nv, t = -nv, -t
        for k, pm in enumerate((1.0, -1.0)):
            out["pose_all"][2 * c + k] = np.c_[R, pm * t]
            out["normal_all"][2 * c + k] = pm * nv
    P1 = np.eye(3, 4)
    goods = []
    for k in range(4):
        P2 = out["pose_all"][k]
        X, _ = ref.triangulate(P1, P2, x1, x2)
        z1, z2 = X[:, 2], X @ P2[2, :3] + P2[2, 3]
        with np.errstate(invalid="ignore"):
            goods.append(sel & (z1 > 0) & (z1 < distance_thresh) & (z2 > 0) & (z2 < distance_thresh))
        out["count"][k] = int(goods[k].sum())
    win = int(np.argmax(out["count"]))
    second = max(int(out["count"][k]) for k in range(4) if k != win)
    out.update(pose=out["pose_all"][win], good=goods[win], stats=np.array([out["count"][win], win, second, 4]))
    return out


# ---------------------------------------------------------------- model scores
def fundamental(E, K):
    fx, fy, cx, cy = K
    Ki = np.linalg.inv(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]]))
    return Ki.T @ np.asarray(E, np.float64).reshape(3, 3) @ Ki


def score_terms(H, E, K, px1, px2, sigma=1.0):
    """The four chi-square terms per match, [n,4]: transfer 1->2, transfer 2->1 (under the ADJUGATE of H, as the header),
    epipolar distance in image 2, in image 1 - NaN where undefined."""
    Hm = np.asarray(H, np.float64).reshape(3, 3)
    h = Hm.reshape(9)
    adj = np.array([h[4] * h[8] - h[5] * h[7], h[2] * h[7] - h[1] * h[8], h[1] * h[5] - h[2] * h[4],
                    h[5] * h[6] - h[3] * h[8], h[0] * h[8] - h[2] * h[6], h[2] * h[3] - h[0] * h[5],
                    h[3] * h[7] - h[4] * h[6], h[1] * h[6] - h[0] * h[7], h[0] * h[4] - h[1] * h[3]])
    F = fundamental(E, K)
    s2 = sigma * sigma
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t12 = ((transfer(Hm, px1) - px2) ** 2).sum(1) / s2
        t21 = ((transfer(adj, px2) - px1) ** 2).sum(1) / s2
        l = np.c_[px1, np.ones(len(px1))] @ F.T
        m = np.c_[px2, np.ones(len(px2))] @ F
        r = (np.c_[px2, np.ones(len(px2))] * l).sum(1)
        e2 = r * r / (l[:, 0] ** 2 + l[:, 1] ** 2) / s2
        e1 = r * r / (m[:, 0] ** 2 + m[:, 1] ** 2) / s2
    return np.stack([t12, t21, e2, e1], 1)


def _transfer_sq(m, x, y, u, v):
    w = (m[6] * x + m[7] * y) + m[8]
    du = ((m[0] * x + m[1] * y) + m[2]) / w - u
    dv = ((m[3] * x + m[4] * y) + m[5]) / w - v
    return du * du + dv * dv


def fixed_point_scores(H, E, K, px1, px2, sigma=1.0):
    """(S_H, S_E) as the header of slam_hg_model_score_f64 states them, elementwise in its operation order on numpy doubles
    (IEEE, nothing fused): the adjugate and F entry by entry, every term (int64)((5.991 - c) * 2^20) where c is below its
    gate, NaN terms nothing, summed as Python integers."""
    h = np.asarray(H, np.float64).reshape(9)
    e = np.asarray(E, np.float64).reshape(9)
    fx, fy, cx, cy = (np.float64(v) for v in K)
    a = [h[4] * h[8] - h[5] * h[7], h[2] * h[7] - h[1] * h[8], h[1] * h[5] - h[2] * h[4],
         h[5] * h[6] - h[3] * h[8], h[0] * h[8] - h[2] * h[6], h[2] * h[3] - h[0] * h[5],
         h[3] * h[7] - h[4] * h[6], h[1] * h[6] - h[0] * h[7], h[0] * h[4] - h[1] * h[3]]
    A, f = [None] * 9, [None] * 9
    for i in range(3):
        A[3 * i], A[3 * i + 1] = e[3 * i] / fx, e[3 * i + 1] / fy
        A[3 * i + 2] = e[3 * i + 2] - (cx * A[3 * i] + cy * A[3 * i + 1])
    for j in range(3):
        f[j], f[3 + j] = A[j] / fx, A[3 + j] / fy
        f[6 + j] = A[6 + j] - (cx * f[j] + cy * f[3 + j])
    px1, px2 = np.asarray(px1, np.float64).reshape(-1, 2), np.asarray(px2, np.float64).reshape(-1, 2)
    x, y, u, v = px1[:, 0], px1[:, 1], px2[:, 0], px2[:, 1]
    s2 = np.float64(sigma) * np.float64(sigma)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        l0, l1, l2 = (f[0] * x + f[1] * y) + f[2], (f[3] * x + f[4] * y) + f[5], (f[6] * x + f[7] * y) + f[8]
        m0, m1 = (f[0] * u + f[3] * v) + f[6], (f[1] * u + f[4] * v) + f[7]
        r = (u * l0 + v * l1) + l2
        r2 = r * r
        chi = [_transfer_sq(h, x, y, u, v) / s2, _transfer_sq(a, u, v, x, y) / s2, (r2 / (l0 * l0 + l1 * l1)) / s2, (r2 / (m0 * m0 + m1 * m1)) / s2]
        out = []
        for c, gate in zip(chi, (CHI2_H, CHI2_H, CHI2_E, CHI2_E)):
            c = np.broadcast_to(c, x.shape)
            keep = c < gate
            out.append(int(((CHI2_H - c[keep]) * FIXED).astype(np.int64).sum()))
    return out[0] + out[1], out[2] + out[3]


def model_scores(H, E, K, px1, px2, sigma=1.0):
    """(S_H, S_E as float sums, ratio) by ORB-SLAM's definition."""
    c = score_terms(H, E, K, px1, px2, sigma)
    with np.errstate(invalid="ignore"):
        sh = np.where(c[:, :2] < CHI2_H, CHI2_H - c[:, :2], 0.0).sum()
        se = np.where(c[:, 2:] < CHI2_E, CHI2_H - c[:, 2:], 0.0).sum()
    return float(sh), float(se), float(sh / (sh + se)) if sh + se > 0 else 0.0


# ---------------------------------------------------------------- what two_view_ref lacks: noisy planar scenes, four-point samples
def scenes_planar_noisy(seed=0, n=200, noise_px=0.5, outlier_share=0.3):
    """two_view_ref.scenes_planar with pixel noise on both images and a share of the second image's points replaced by uniform
    pixels; "true_inlier" marks the rest."""
    out = []
    for sc in ref.scenes_planar(seed, n):
        rng = np.random.default_rng([seed, 201, len(out)])
        sc = dict(sc)
        px1 = sc["px1"] + rng.normal(0, noise_px, (n, 2))
        px2 = sc["px2"] + rng.normal(0, noise_px, (n, 2))
        bad = rng.choice(n, int(round(outlier_share * n)), replace=False)
        px2[bad] = np.stack([rng.uniform(0, ref.IMAGE[0], len(bad)), rng.uniform(0, ref.IMAGE[1], len(bad))], 1)
        ti = np.ones(n, bool)
        ti[bad] = False
        sc.update(px1=px1, px2=px2, true_inlier=ti, family="planar_noisy")
        out.append(sc)
    return out


def fourpoint_samples(seed, S, n=200):
    """S four-point samples from the tilted planar scene of ``n`` matches (general motion, EuRoC intrinsics), four distinct
    matches each: (p1 [S,4,2], p2 [S,4,2] in pixels, H_true [9])."""
    sc = ref.scenes_planar(seed, n)[1]
    rng = np.random.default_rng([seed, 202])
    idx = np.array([rng.choice(n, 4, replace=False) for _ in range(S)])
    return sc["px1"][idx], sc["px2"][idx], homography_from_pose(sc["R"], sc["t"], sc["plane"])


def family_scenes(seed=0, n=200):
    """The scenes the homography tests run on: (name, scene) of the planar, pure-rotation and four general families."""
    out = [(f"{sc['family']}/{sc['variant']}", sc) for fam in ("planar", "pure_rotation") for sc in ref.FAMILIES[fam](seed, n)]
    for fam in ("general", "forward", "sideways", "integer_pixels"):
        sc = ref.FAMILIES[fam](seed, n)[0]
        out.append((f"{sc['family']}/{sc['variant']}", sc))
    return out
