"""The independent numpy statement of SE(3) pose-graph optimisation that the pose-graph tests compare the kernels with,
and the scenes they run on.  Nothing here is imported by the product.

Conventions (include/slamhip.h): T = [R|t] with X_cam = R X_world + t, tangent [w, v] rotation first, update T <- Exp(d) T;
edge (i, j) measures Z ~ T_j T_i^-1, r = Log(T_j T_i^-1 Z^-1), F = sum rho(r^T Omega r), H = sum w J^T Omega J,
b = sum w J^T Omega r, dr/dd_j = Jl^-1(r), dr/dd_i = -Jl^-1(r) Ad(T_j T_i^-1).

Two paths to the same numbers, so that their difference measures what f64 leaves undetermined:
  closed   Log, V^-1 and Jl^-1 from the closed forms (Barfoot, State Estimation for Robotics, 7.86), Taylor below 0.2 rad
  series   V^-1 = sum_n B_n / n! (w^)^n and Jl^-1 = sum_n B_n / n! ad(r)^n with the Bernoulli numbers (angles below 2 pi)
and two solvers: scipy's sparse direct solve, and an own block-Jacobi PCG (the algorithm the kernels implement).
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

PCG_TOL = 1e-8
PCG_MAX_ITER = 500


# ---------------------------------------------------------------- SE(3) -----------------------------------------------------
def hat(w):
    w = np.asarray(w, np.float64)
    W = np.zeros(w.shape[:-1] + (3, 3))
    W[..., 0, 1], W[..., 0, 2] = -w[..., 2], w[..., 1]
    W[..., 1, 0], W[..., 1, 2] = w[..., 2], -w[..., 0]
    W[..., 2, 0], W[..., 2, 1] = -w[..., 1], w[..., 0]
    return W


def as34(T):
    T = np.asarray(T, np.float64)
    if T.shape[-1] == 12:
        T = T.reshape(T.shape[:-1] + (3, 4))
    return T[..., :3, :4]


def inv(T):
    T = as34(T)
    Rt = np.swapaxes(T[..., :3], -1, -2)
    return np.concatenate([Rt, -Rt @ T[..., 3:]], -1)


def mul(A, B):
    A, B = as34(A), as34(B)
    return np.concatenate([A[..., :3] @ B[..., :3], A[..., :3] @ B[..., 3:] + A[..., 3:]], -1)


def _abc(th):
    """sin(th)/th, (1-cos)/th^2, (th-sin)/th^3"""
    th = np.asarray(th, np.float64)
    small = th < 1e-2
    t = np.where(small, 1.0, th)
    t2 = th * th
    a = np.where(small, 1 - t2 / 6 + t2 * t2 / 120, np.sin(t) / t)
    b = np.where(small, 0.5 - t2 / 24 + t2 * t2 / 720, (1 - np.cos(t)) / (t * t))
    c = np.where(small, 1 / 6 - t2 / 120 + t2 * t2 / 5040, (t - np.sin(t)) / (t * t * t))
    return a, b, c


def exp_se3(xi):
    xi = np.asarray(xi, np.float64)
    w, v = xi[..., :3], xi[..., 3:]
    th = np.linalg.norm(w, axis=-1)
    a, b, c = (x[..., None, None] for x in _abc(th))
    W = hat(w)
    W2 = W @ W
    I = np.eye(3)
    R = I + a * W + b * W2
    V = I + b * W + c * W2
    return np.concatenate([R, V @ v[..., None]], -1)


def _k(th):
    """coefficient of W^2 in Jso3^-1 = I - W/2 + k W^2"""
    th = np.asarray(th, np.float64)
    small = th < 0.2
    t = np.where(small, 1.0, th)
    t2 = th * th
    return np.where(small, 1 / 12 + t2 / 720 + t2 ** 2 / 30240 + t2 ** 3 / 1209600, (1 - t * np.sin(t) / (2 * (1 - np.cos(t)))) / (t * t))


def log_so3(R):
    s = 0.5 * np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1)
    c = 0.5 * (np.trace(R, axis1=-2, axis2=-1) - 1)
    sn = np.linalg.norm(s, axis=-1)
    th = np.arctan2(sn, c)
    small = sn < 1e-6
    f = np.where(small, 1 + th * th / 6, th / np.where(small, 1.0, sn))
    return f[..., None] * s


def log_se3(T, series=False):
    """[w, v] with v = V^-1 t; V^-1 = Jso3^-1(w) from its closed form, or (series) as sum_n B_n / n! (w^)^n"""
    T = as34(T)
    w = log_so3(T[..., :3])
    th = np.linalg.norm(w, axis=-1)
    W = hat(w)
    if series:
        Vinv = np.zeros_like(W) + np.eye(3)
        P = np.zeros_like(W) + np.eye(3)
        fact = Fraction(1)
        for n in range(1, 81):
            P = P @ W
            fact *= n
            if _BERN[n] != 0:
                Vinv = Vinv + float(_BERN[n] / fact) * P
    else:
        Vinv = np.eye(3) - 0.5 * W + _k(th)[..., None, None] * (W @ W)
    return np.concatenate([w, (Vinv @ T[..., 3:])[..., 0]], -1)


def adjoint(T):
    T = as34(T)
    R, t = T[..., :3], T[..., 3]
    Ad = np.zeros(T.shape[:-2] + (6, 6))
    Ad[..., :3, :3] = R
    Ad[..., 3:, 3:] = R
    Ad[..., 3:, :3] = hat(t) @ R
    return Ad


def ad(xi):
    """ad([w, v]) = [[w^, 0], [v^, w^]] (rotation first)"""
    xi = np.asarray(xi, np.float64)
    M = np.zeros(xi.shape[:-1] + (6, 6))
    M[..., :3, :3] = hat(xi[..., :3])
    M[..., 3:, 3:] = hat(xi[..., :3])
    M[..., 3:, :3] = hat(xi[..., 3:])
    return M


def jl_inv_closed(xi):
    xi = np.asarray(xi, np.float64)
    w, v = xi[..., :3], xi[..., 3:]
    th = np.linalg.norm(w, axis=-1)
    small = th < 0.2          # the closed forms cancel (c3 loses eps / th^5): Taylor to th^6 below, next term < 1e-13 relative
    t = np.where(small, 1.0, th)
    t2 = th * th
    c1 = np.where(small, 1 / 6 - t2 / 120 + t2 ** 2 / 5040 - t2 ** 3 / 362880, (t - np.sin(t)) / t ** 3)
    c2 = np.where(small, 1 / 24 - t2 / 720 + t2 ** 2 / 40320 - t2 ** 3 / 3628800, (t * t + 2 * np.cos(t) - 2) / (2 * t ** 4))
    c3 = np.where(small, 1 / 120 - t2 / 2520 + t2 ** 2 / 120960 - t2 ** 3 / 9979200,
                  (2 * t - 3 * np.sin(t) + t * np.cos(t)) / (2 * t ** 5))
    c1, c2, c3 = (x[..., None, None] for x in (c1, c2, c3))
    W, P = hat(w), hat(v)
    W2 = W @ W
    Q = 0.5 * P + c1 * (W @ P + P @ W + W @ P @ W) + c2 * (W2 @ P + P @ W2 - 3 * W @ P @ W) + c3 * (W @ P @ W2 + W2 @ P @ W)
    Ji = np.eye(3) - 0.5 * W + _k(th)[..., None, None] * W2
    J = np.zeros(xi.shape[:-1] + (6, 6))
    J[..., :3, :3] = Ji
    J[..., 3:, 3:] = Ji
    J[..., 3:, :3] = -Ji @ Q @ Ji
    return J


def bernoulli(n):
    """B_0 .. B_n (B_1 = -1/2) as floats, from exact fractions"""
    B = [Fraction(0)] * (n + 1)
    B[0] = Fraction(1)
    for m in range(1, n + 1):
        acc = Fraction(0)
        c = 1
        for k in range(m):
            acc += c * B[k]
            c = c * (m + 1 - k) // (k + 1)
        B[m] = -acc / (m + 1)
    return B


_BERN = bernoulli(80)


def jl_inv_series(xi, terms=80):
    """sum_{n} B_n / n! ad(xi)^n: the inverse left Jacobian as its defining series"""
    A = ad(xi)
    out = np.zeros_like(A) + np.eye(6)
    P = np.zeros_like(A) + np.eye(6)
    fact = Fraction(1)
    for n in range(1, terms + 1):
        P = P @ A
        fact *= n
        if _BERN[n] != 0:
            out = out + float(_BERN[n] / fact) * P
    return out


# ---------------------------------------------------------------- the graph -------------------------------------------------
def residuals(poses, edges, meas, series=False):
    poses, meas = as34(poses), as34(meas)
    A = mul(poses[edges[:, 1]], inv(poses[edges[:, 0]]))
    return log_se3(mul(A, inv(meas)), series), A


def robust(chi2, huber):
    """(rho, weight) as pose_opt.hip applies Huber"""
    if huber <= 0:
        return chi2, np.ones_like(chi2)
    e = np.sqrt(chi2)
    out = e > huber
    es = np.where(out, e, 1.0)
    return np.where(out, 2 * huber * e - huber * huber, chi2), np.where(out, huber / es, 1.0)


def cost(poses, edges, meas, info, huber=0.0):
    r, _ = residuals(poses, edges, meas)
    chi2 = np.einsum("ea,eab,eb->e", r, info, r)
    return float(robust(chi2, huber)[0].sum())


def max_residual_angle(poses, edges, meas):
    r, _ = residuals(poses, edges, meas)
    return float(np.linalg.norm(r[:, :3], axis=1).max()) if len(r) else 0.0


def linearize(poses, edges, meas, info, huber=0.0, series=False):
    """cost, b [V,6], Hd [V,6,6], W [E,6,6] (row block i, column block j)"""
    V = len(poses)
    r, A = residuals(poses, edges, meas, series)
    Jj = jl_inv_series(r) if series else jl_inv_closed(r)
    Ji = -Jj @ adjoint(A)
    chi2 = np.einsum("ea,eab,eb->e", r, info, r)
    rho, w = robust(chi2, huber)
    wI = w[:, None, None] * info
    Or = np.einsum("eab,eb->ea", wI, r)
    JiT, JjT = np.swapaxes(Ji, 1, 2), np.swapaxes(Jj, 1, 2)
    W = JiT @ wI @ Jj
    Hd = np.zeros((V, 6, 6))
    b = np.zeros((V, 6))
    np.add.at(Hd, edges[:, 0], JiT @ wI @ Ji)
    np.add.at(Hd, edges[:, 1], JjT @ wI @ Jj)
    np.add.at(b, edges[:, 0], np.einsum("eba,eb->ea", Ji, Or))
    np.add.at(b, edges[:, 1], np.einsum("eba,eb->ea", Jj, Or))
    return float(rho.sum()), b, Hd, W


def assemble(V, edges, Hd, W):
    """the full 6V x 6V H as CSR (duplicate edges add up)"""
    k = np.arange(6)
    rows, cols, vals = [], [], []

    def put(bi, bj, blocks):
        rows.append((6 * bi[:, None, None] + k[None, :, None]).repeat(6, 2).ravel())
        cols.append((6 * bj[:, None, None] + k[None, None, :]).repeat(6, 1).ravel())
        vals.append(blocks.ravel())

    put(np.arange(V), np.arange(V), Hd)
    if len(edges):
        put(edges[:, 0], edges[:, 1], W)
        put(edges[:, 1], edges[:, 0], np.swapaxes(W, 1, 2))
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(6 * V, 6 * V))


def free_index(fixed):
    free = np.flatnonzero(~np.asarray(fixed, bool))
    return (6 * free[:, None] + np.arange(6)[None]).ravel()


def hmul(H, fixed, lam, x):
    """(H + lam I) x restricted to the free vertices: rows of fixed vertices 0, their columns ignored"""
    f = free_index(fixed)
    y = np.zeros(H.shape[0])
    xf = np.asarray(x, np.float64).ravel()[f]
    y[f] = H[f][:, f] @ xf + lam * xf
    return y.reshape(-1, 6)


def pcg(Hff, bf, lam, tol=PCG_TOL, max_iter=PCG_MAX_ITER):
    """block-Jacobi PCG on (Hff + lam I) x = -bf; returns (x, iterations, |r|/|b| of the recurrence)"""
    n = Hff.shape[0] // 6
    A = (Hff + lam * sp.identity(6 * n, format="csr")).tocsr()
    D = np.stack([A[6 * v:6 * v + 6, 6 * v:6 * v + 6].toarray() for v in range(n)]) if n < 4000 else _diag_blocks(A, n)
    Minv = np.linalg.inv(D)
    r = -bf.copy()
    x = np.zeros_like(r)
    bb = float(r @ r)
    if bb == 0.0:
        return x, 0, 0.0
    z = np.einsum("vab,vb->va", Minv, r.reshape(n, 6)).ravel()
    p = z.copy()
    rz = float(r @ z)
    rr = bb
    it = 0
    while it < max_iter and rr > tol * tol * bb:
        q = A @ p
        alpha = rz / float(p @ q)
        x += alpha * p
        r -= alpha * q
        z = np.einsum("vab,vb->va", Minv, r.reshape(n, 6)).ravel()
        rz_new = float(r @ z)
        rr = float(r @ r)
        p = z + (rz_new / rz) * p
        rz = rz_new
        it += 1
    return x, it, float(np.sqrt(rr / bb))


def _diag_blocks(A, n):
    A = A.tocoo()
    m = (A.row // 6) == (A.col // 6)
    D = np.zeros((n, 6, 6))
    np.add.at(D, (A.row[m] // 6, A.row[m] % 6, A.col[m] % 6), A.data[m])
    return D


def optimize(poses, edges, meas, info, fixed, iterations=15, huber=0.0, solver="direct", tol=PCG_TOL, max_iter=PCG_MAX_ITER,
             visit=None):
    """g2o's LM schedule as slamhip/pose_opt.py restates it.  Returns (poses [V,3,4], stats dict).  `visit(poses)` is called at
    every state the loop evaluates (the start and every candidate)."""
    poses = as34(poses).copy()
    fixed = np.asarray(fixed, bool)
    V = len(poses)
    f = free_index(fixed)
    free_v = np.flatnonzero(~fixed)
    if visit:
        visit(poses)
    F, b, Hd, W = linearize(poses, edges, meas, info, huber)
    F0 = F
    dmax = float(np.max(np.einsum("vaa->va", Hd[free_v]))) if len(free_v) else 0.0
    lam, ni = 1e-5 * max(dmax, 1e-12), 2.0
    accepted = trials = cg = 0
    for _ in range(iterations):
        Hff = assemble(V, edges, Hd, W)[f][:, f].tocsc()
        bf = b.ravel()[f]
        taken = False
        for _trial in range(10):
            if solver == "direct":
                xf = spla.spsolve((Hff + lam * sp.identity(len(f), format="csc")).tocsc(), -bf)
            else:
                xf, n_it, _ = pcg(Hff.tocsr(), bf, lam, tol, max_iter)
                cg += n_it
            trials += 1
            dx = np.zeros(6 * V)
            dx[f] = xf
            cand = poses.copy()
            cand[free_v] = mul(exp_se3(dx.reshape(V, 6)[free_v]), poses[free_v])
            if visit:
                visit(cand)
            Fc = cost(cand, edges, meas, info, huber)
            scale = float(xf @ (lam * xf - bf)) + 1e-3
            rho = (F - Fc) / scale
            if rho > 0 and np.isfinite(Fc):
                poses, F = cand, Fc
                lam *= max(1 / 3, min(1 - (2 * rho - 1) ** 3, 2 / 3))
                ni = 2.0
                accepted += 1
                taken = True
                _, b, Hd, W = linearize(poses, edges, meas, info, huber)
                break
            lam *= ni
            ni *= 2.0
            if not np.isfinite(lam):
                break
        if not taken:
            break
    return poses, dict(chi2_initial=F0, chi2_final=F, iterations=accepted, trials=trials, cg_iterations=cg, lam=lam)


def pose_gap(A, B):
    """largest rotation angle and largest translation distance (of the camera centres) between two pose sets"""
    A, B = as34(A), as34(B)
    ang = np.linalg.norm(log_so3(A[:, :, :3] @ np.swapaxes(B[:, :, :3], 1, 2)), axis=1)   # atan2 form: exact near zero
    return float(ang.max()), float(np.linalg.norm(centres(A) - centres(B), axis=1).max())


def centres(T):
    T = as34(T)
    return -(np.swapaxes(T[:, :, :3], 1, 2) @ T[:, :, 3:])[:, :, 0]


def extent(T):
    c = centres(T)
    return float(np.linalg.norm(c.max(0) - c.min(0)))


# ---------------------------------------------------------------- scenes -----------------------------------------------------
def _world_to_cam(Rwc, p):
    """T = [R|t] from camera-to-world rotation and camera centre"""
    R = np.swapaxes(Rwc, -1, -2)
    return np.concatenate([R, -R @ p[..., None]], -1)


def _rot_z(a):
    c, s, z, o = np.cos(a), np.sin(a), np.zeros_like(a), np.ones_like(a)
    return np.stack([np.stack([c, -s, z], -1), np.stack([s, c, z], -1), np.stack([z, z, o], -1)], -2)


def _rot_y(a):
    c, s, z, o = np.cos(a), np.sin(a), np.zeros_like(a), np.ones_like(a)
    return np.stack([np.stack([c, z, s], -1), np.stack([z, o, z], -1), np.stack([-s, z, c], -1)], -2)


def _measure(gt, edges, rng, sig_r, sig_t):
    E = len(edges)
    noise = np.concatenate([rng.normal(0, sig_r, (E, 3)), rng.normal(0, sig_t, (E, 3))], 1)
    Z = mul(exp_se3(noise), mul(gt[edges[:, 1]], inv(gt[edges[:, 0]])))
    info = np.tile(np.diag([1 / sig_r ** 2] * 3 + [1 / sig_t ** 2] * 3), (E, 1, 1))
    return Z, info


def _chain(gt0, Z_odo):
    """initial guess by chaining odometry: T_{k+1} = Z_k T_k"""
    out = np.empty((len(Z_odo) + 1, 3, 4))
    out[0] = gt0
    for k in range(len(Z_odo)):
        out[k + 1] = mul(Z_odo[k], out[k])
    return out


class Scene:
    def __init__(self, name, gt, init, edges, meas, info, fixed):
        self.name, self.gt, self.init = name, gt, init
        self.edges = np.ascontiguousarray(edges, np.int32)
        self.meas, self.info = np.ascontiguousarray(meas), np.ascontiguousarray(info)
        self.fixed = np.ascontiguousarray(fixed, np.uint8)
        self.V, self.E = len(gt), len(edges)


def sphere(rings=50, per_ring=50, radius=100.0, sig_r=0.01, sig_t=0.1, seed=11):
    """g2o's classic sphere restated from its description: `rings` x `per_ring` poses on a sphere, odometry along the spiral,
    loop edges to the three nearest poses of the ring below, Gaussian noise, initial guess by chaining odometry."""
    rng = np.random.default_rng(seed)
    n = rings * per_ring
    k = np.arange(n)
    lon = 2 * np.pi * k / per_ring
    lat = -0.45 * np.pi + 0.9 * np.pi * k / (n - 1)
    p = radius * np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)], 1)
    gt = _world_to_cam(_rot_z(lon) @ _rot_y(-lat), p)
    odo = np.stack([k[:-1], k[1:]], 1)
    loops = [np.stack([k[per_ring + d:] - per_ring - d, k[per_ring + d:]], 1) for d in (-1, 0, 1)]
    edges = np.concatenate([odo] + loops)
    Z, info = _measure(gt, edges, rng, sig_r, sig_t)
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    return Scene("sphere", gt, _chain(gt[0], Z[:n - 1]), edges, Z, info, fixed)


def loop_closure(n=512, closures=48, outlier_fraction=0.0, sig_r=0.004, sig_t=0.03, seed=5):
    """a 512-keyframe trajectory (two laps of a wavy circle) with drifting odometry and a few dozen closures between the laps;
    `outlier_fraction` of the closures carry a wrong measurement (rotation off by up to 0.8 rad, translation by metres)."""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    a = 4 * np.pi * k / n
    p = np.stack([20 * np.cos(a), 20 * np.sin(a), 1.5 * np.sin(3 * a) + 0.002 * k], 1)
    gt = _world_to_cam(_rot_z(a + np.pi / 2) @ _rot_y(0.1 * np.sin(2 * a)), p)
    odo = np.stack([k[:-1], k[1:]], 1)
    first = rng.choice(n // 2 - 8, closures, replace=False)
    second = first + n // 2 + rng.integers(-4, 5, closures)
    edges = np.concatenate([odo, np.stack([first, second], 1)])
    Z, info = _measure(gt, edges, rng, sig_r, sig_t)
    n_bad = int(round(outlier_fraction * closures))
    if n_bad:
        bad = (n - 1) + rng.choice(closures, n_bad, replace=False)
        wrong = np.concatenate([rng.uniform(-0.45, 0.45, (n_bad, 3)), rng.uniform(-4, 4, (n_bad, 3))], 1)
        Z[bad] = mul(exp_se3(wrong), Z[bad])
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    return Scene("loop_closure", gt, _chain(gt[0], Z[:n - 1]), edges, Z, info, fixed)


def hub(spokes=1000, sig_r=0.01, sig_t=0.05, seed=3):
    """vertex 0 with `spokes` incident edges (alternating direction) and a rim that links consecutive spoke vertices;
    vertex 1 is the fixed one, so the hub's row stays in the system"""
    rng = np.random.default_rng(seed)
    n = spokes + 1
    a = 2 * np.pi * np.arange(spokes) / spokes
    p = np.concatenate([np.zeros((1, 3)), np.stack([10 * np.cos(a), 10 * np.sin(a), np.sin(5 * a)], 1)])
    yaw = np.concatenate([[0.0], a + np.pi / 2])
    gt = _world_to_cam(_rot_z(yaw), p)
    s = np.arange(1, n)
    spokes_e = np.where((s % 2 == 0)[:, None], np.stack([np.zeros_like(s), s], 1), np.stack([s, np.zeros_like(s)], 1))
    rim = np.stack([s[:-1], s[1:]], 1)
    edges = np.concatenate([spokes_e, rim])
    Z, info = _measure(gt, edges, rng, sig_r, sig_t)
    init = mul(exp_se3(np.concatenate([rng.normal(0, 0.05, (n, 3)), rng.normal(0, 0.3, (n, 3))], 1)), gt)
    init[1] = gt[1]
    fixed = np.zeros(n, np.uint8)
    fixed[1] = 1
    return Scene("hub", gt, init, edges, Z, info, fixed)


def multi_hub(hubs=70, leaves=140, sig_r=0.01, sig_t=0.05, seed=13):
    """`hubs` vertices that each see all `leaves` leaf vertices (alternating direction) plus a chain through the leaves:
    every hub has `leaves` incident edges, more hubs than the product kernel has hub waves; the first leaf is fixed"""
    rng = np.random.default_rng(seed)
    n = hubs + leaves
    ah, al = 2 * np.pi * np.arange(hubs) / hubs, 2 * np.pi * np.arange(leaves) / leaves
    p = np.concatenate([np.stack([3 * np.cos(ah), 3 * np.sin(ah), 0.5 * np.cos(3 * ah)], 1),
                        np.stack([12 * np.cos(al), 12 * np.sin(al), np.sin(4 * al)], 1)])
    gt = _world_to_cam(_rot_z(np.concatenate([ah, al + np.pi / 2])), p)
    h, l = np.meshgrid(np.arange(hubs), hubs + np.arange(leaves), indexing="ij")
    h, l = h.ravel(), l.ravel()
    flip = ((h + l) % 2 == 0)[:, None]
    spokes = np.where(flip, np.stack([h, l], 1), np.stack([l, h], 1))
    chain = np.stack([hubs + np.arange(leaves - 1), hubs + np.arange(1, leaves)], 1)
    edges = np.concatenate([spokes, chain])
    Z, info = _measure(gt, edges, rng, sig_r, sig_t)
    init = mul(exp_se3(np.concatenate([rng.normal(0, 0.05, (n, 3)), rng.normal(0, 0.3, (n, 3))], 1)), gt)
    init[hubs] = gt[hubs]
    fixed = np.zeros(n, np.uint8)
    fixed[hubs] = 1
    return Scene("multi_hub", gt, init, edges, Z, info, fixed)


def large(n=100_000, sig_r=0.005, sig_t=0.02, seed=9):
    """10^5 poses on a long spiral, edges to the poses 1, 10, 100 and 1000 steps ahead (about 4 * 10^5), start = truth
    perturbed pose by pose"""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    a = 2 * np.pi * k / 1000.0
    p = np.stack([(50 + 0.001 * k) * np.cos(a), (50 + 0.001 * k) * np.sin(a), 0.01 * k + np.sin(7 * a)], 1)
    gt = _world_to_cam(_rot_z(a + np.pi / 2), p)
    edges = np.concatenate([np.stack([k[:-d], k[d:]], 1) for d in (1, 10, 100, 1000)])
    Z, info = _measure(gt, edges, rng, sig_r, sig_t)
    init = mul(exp_se3(np.concatenate([rng.normal(0, 0.02, (n, 3)), rng.normal(0, 0.2, (n, 3))], 1)), gt)
    init[0] = gt[0]
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    return Scene("large", gt, init, edges, Z, info, fixed)


def noise_free(scene):
    """the same graph with exact measurements and the truth as the start: already at its optimum"""
    Z = mul(scene.gt[scene.edges[:, 1]], inv(scene.gt[scene.edges[:, 0]]))
    return Scene(scene.name + "_exact", scene.gt, scene.gt.copy(), scene.edges, Z, scene.info, scene.fixed)


def trajectory_error(poses, gt):
    return float(np.linalg.norm(centres(poses) - centres(gt), axis=1).mean())


SMALL_SCENES = {"sphere": sphere, "loop_closure": loop_closure, "hub": hub}
