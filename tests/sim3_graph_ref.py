"""The independent numpy statement of Sim(3) pose-graph optimisation that the sim3-graph tests compare the kernels with, and
the scenes they run on.  Nothing here is imported by the product.  The SE(3) functions come from pose_graph_ref by import.

Conventions (include/slamhip.h): S = (s, R, t) stored [13] = row-major [R|t] then s, X_cam = s R X_world + t; tangent
[w, v, sigma]; chart Phi(d) = Exp_SE3(w, v) o Scale(e^sigma) = (e^sigma, Exp(w), V(w) v); update S <- Phi(d) o S; edge (i, j)
measures Z ~ S_j S_i^-1, D = S_j S_i^-1 Z^-1, r = Phi^-1(D) = [Log_SE3(R_D, t_D), log s_D]; F = sum rho(r^T Omega r);
J_j = [[Jl^-1, Jl^-1 (0; t_D)], [0, 1]], J_i = -J_j Ad(A), A = S_j S_i^-1, Ad(A) = [[R, 0, 0], [t^ R, s R, -t], [0, 0, 1]].
`numeric=True` replaces the Jacobian formulas by central differences of the residual under Phi(d) o S.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import pose_graph_ref as P

PCG_TOL = P.PCG_TOL
PCG_MAX_ITER = P.PCG_MAX_ITER


# ---------------------------------------------------------------- Sim(3) ------------------------------------------------------
def pack(s, T):
    """(s [...], [R|t] [...,3,4]) -> [...,13]"""
    T = P.as34(T)
    return np.concatenate([T.reshape(T.shape[:-2] + (12,)), np.asarray(s, np.float64)[..., None]], -1)


def parts(S):
    S = np.asarray(S, np.float64)
    T = S[..., :12].reshape(S.shape[:-1] + (3, 4))
    return S[..., 12], T[..., :3], T[..., 3]


def inv(S):
    s, R, t = parts(S)
    Rt = np.swapaxes(R, -1, -2)
    return pack(1.0 / s, np.concatenate([Rt, -(Rt @ t[..., None]) / s[..., None, None]], -1))


def mul(A, B):
    sa, Ra, ta = parts(A)
    sb, Rb, tb = parts(B)
    return pack(sa * sb, np.concatenate([Ra @ Rb, sa[..., None, None] * (Ra @ tb[..., None]) + ta[..., None]], -1))


def phi(d):
    d = np.asarray(d, np.float64)
    return pack(np.exp(d[..., 6]), P.exp_se3(d[..., :6]))


def phi_inv(D, series=False):
    s, R, t = parts(D)
    return np.concatenate([P.log_se3(np.concatenate([R, t[..., None]], -1), series), np.log(s)[..., None]], -1)


def adjoint(A):
    s, R, t = parts(A)
    Ad = np.zeros(s.shape + (7, 7))
    Ad[..., :3, :3] = R
    Ad[..., 3:6, :3] = P.hat(t) @ R
    Ad[..., 3:6, 3:6] = s[..., None, None] * R
    Ad[..., 3:6, 6] = -t
    Ad[..., 6, 6] = 1.0
    return Ad


def residuals(sims, edges, meas, series=False):
    A = mul(sims[edges[:, 1]], inv(sims[edges[:, 0]]))
    D = mul(A, inv(meas))
    return phi_inv(D, series), A, D


def jacobians(sims, edges, meas, series=False, numeric=False, fix_scale=False, h=1e-6):
    """(r [E,7], J_i [E,7,7], J_j [E,7,7])"""
    r, A, D = residuals(sims, edges, meas, series)
    E = len(edges)
    if numeric:
        Ji, Jj = np.zeros((E, 7, 7)), np.zeros((E, 7, 7))
        Si, Sj = sims[edges[:, 0]], sims[edges[:, 1]]
        for k in range(7):
            d = np.zeros((E, 7))
            d[:, k] = h
            res = lambda a, b: phi_inv(mul(mul(b, inv(a)), inv(meas)), series)
            Ji[:, :, k] = (res(mul(phi(d), Si), Sj) - res(mul(phi(-d), Si), Sj)) / (2 * h)
            Jj[:, :, k] = (res(Si, mul(phi(d), Sj)) - res(Si, mul(phi(-d), Sj))) / (2 * h)
    else:
        J6 = P.jl_inv_series(r[:, :6]) if series else P.jl_inv_closed(r[:, :6])
        Jj = np.zeros((E, 7, 7))
        Jj[:, :6, :6] = J6
        tD = np.concatenate([np.zeros((E, 3)), parts(D)[2]], 1)
        Jj[:, :6, 6] = np.einsum("eab,eb->ea", J6, tD)
        Jj[:, 6, 6] = 1.0
        Ji = -Jj @ adjoint(A)
    if fix_scale:
        Ji[:, :, 6] = 0.0
        Jj[:, :, 6] = 0.0
    return r, Ji, Jj


def cost(sims, edges, meas, info, huber=0.0):
    r, _, _ = residuals(sims, edges, meas)
    chi2 = np.einsum("ea,eab,eb->e", r, info, r)
    return float(P.robust(chi2, huber)[0].sum())


def linearize(sims, edges, meas, info, huber=0.0, series=False, numeric=False, fix_scale=False):
    """cost, b [V,7], Hd [V,7,7], W [E,7,7] (row block i, column block j)"""
    V = len(sims)
    r, Ji, Jj = jacobians(sims, edges, meas, series, numeric, fix_scale)
    chi2 = np.einsum("ea,eab,eb->e", r, info, r)
    rho, w = P.robust(chi2, huber)
    wI = w[:, None, None] * info
    Or = np.einsum("eab,eb->ea", wI, r)
    JiT, JjT = np.swapaxes(Ji, 1, 2), np.swapaxes(Jj, 1, 2)
    W = JiT @ wI @ Jj
    Hd = np.zeros((V, 7, 7))
    b = np.zeros((V, 7))
    np.add.at(Hd, edges[:, 0], JiT @ wI @ Ji)
    np.add.at(Hd, edges[:, 1], JjT @ wI @ Jj)
    np.add.at(b, edges[:, 0], np.einsum("eba,eb->ea", Ji, Or))
    np.add.at(b, edges[:, 1], np.einsum("eba,eb->ea", Jj, Or))
    return float(rho.sum()), b, Hd, W


def assemble(V, edges, Hd, W):
    """the full 7V x 7V H as CSR (duplicate edges add up)"""
    k = np.arange(7)
    rows, cols, vals = [], [], []

    def put(bi, bj, blocks):
        rows.append((7 * bi[:, None, None] + k[None, :, None]).repeat(7, 2).ravel())
        cols.append((7 * bj[:, None, None] + k[None, None, :]).repeat(7, 1).ravel())
        vals.append(blocks.ravel())

    put(np.arange(V), np.arange(V), Hd)
    if len(edges):
        put(edges[:, 0], edges[:, 1], W)
        put(edges[:, 1], edges[:, 0], np.swapaxes(W, 1, 2))
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(7 * V, 7 * V))


def free_index(fixed):
    free = np.flatnonzero(~np.asarray(fixed, bool))
    return (7 * free[:, None] + np.arange(7)[None]).ravel()


def hmul(H, fixed, lam, x):
    f = free_index(fixed)
    y = np.zeros(H.shape[0])
    xf = np.asarray(x, np.float64).ravel()[f]
    y[f] = H[f][:, f] @ xf + lam * xf
    return y.reshape(-1, 7)


def pcg(Hff, bf, lam, tol=PCG_TOL, max_iter=PCG_MAX_ITER):
    """block-Jacobi PCG on (Hff + lam I) x = -bf; returns (x, iterations, |r|/|b| of the recurrence)"""
    n = Hff.shape[0] // 7
    A = (Hff + lam * sp.identity(7 * n, format="csr")).tocsr()
    C = A.tocoo()
    m = (C.row // 7) == (C.col // 7)
    D = np.zeros((n, 7, 7))
    np.add.at(D, (C.row[m] // 7, C.row[m] % 7, C.col[m] % 7), C.data[m])
    Minv = np.linalg.inv(D)
    r = -bf.copy()
    x = np.zeros_like(r)
    bb = float(r @ r)
    if bb == 0.0:
        return x, 0, 0.0
    z = np.einsum("vab,vb->va", Minv, r.reshape(n, 7)).ravel()
    p = z.copy()
    rz = float(r @ z)
    rr = bb
    it = 0
    while it < max_iter and rr > tol * tol * bb:
        q = A @ p
        alpha = rz / float(p @ q)
        x += alpha * p
        r -= alpha * q
        z = np.einsum("vab,vb->va", Minv, r.reshape(n, 7)).ravel()
        rz_new = float(r @ z)
        rr = float(r @ r)
        p = z + (rz_new / rz) * p
        rz = rz_new
        it += 1
    return x, it, float(np.sqrt(rr / bb))


def optimize(sims, edges, meas, info, fixed, iterations=15, huber=0.0, solver="direct", tol=PCG_TOL, max_iter=PCG_MAX_ITER,
             fix_scale=False):
    """g2o's LM schedule as pose_graph_ref.optimize.  Returns (sims [V,13], stats dict)."""
    sims = np.array(sims, np.float64)
    fixed = np.asarray(fixed, bool)
    V = len(sims)
    f = free_index(fixed)
    free_v = np.flatnonzero(~fixed)
    F, b, Hd, W = linearize(sims, edges, meas, info, huber, fix_scale=fix_scale)
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
            dx = np.zeros(7 * V)
            dx[f] = xf
            cand = sims.copy()
            cand[free_v] = mul(phi(dx.reshape(V, 7)[free_v]), sims[free_v])
            Fc = cost(cand, edges, meas, info, huber)
            scale = float(xf @ (lam * xf - bf)) + 1e-3
            rho = (F - Fc) / scale
            if rho > 0 and np.isfinite(Fc):
                sims, F = cand, Fc
                lam *= max(1 / 3, min(1 - (2 * rho - 1) ** 3, 2 / 3))
                ni = 2.0
                accepted += 1
                taken = True
                _, b, Hd, W = linearize(sims, edges, meas, info, huber, fix_scale=fix_scale)
                break
            lam *= ni
            ni *= 2.0
            if not np.isfinite(lam):
                break
        if not taken:
            break
    return sims, dict(chi2_initial=F0, chi2_final=F, iterations=accepted, trials=trials, cg_iterations=cg, lam=lam)


def to_poses(sims):
    """[R | t / s]: the metric pose of each keyframe"""
    s, R, t = parts(sims)
    return np.concatenate([R, (t / s[..., None])[..., None]], -1)


def sim_gap(A, B):
    """largest rotation angle, largest distance of the metric camera centres, largest |log s_A - log s_B|"""
    ang, dist = P.pose_gap(to_poses(A), to_poses(B))
    return ang, dist, float(np.abs(np.log(parts(A)[0]) - np.log(parts(B)[0])).max())


def ate(sims, gt_poses):
    return P.trajectory_error(to_poses(sims), gt_poses)


# ---------------------------------------------------------------- scenes -----------------------------------------------------
class Scene:
    """gt: the metric poses [V,3,4]; truth: the vertices at which exact edges cost nothing; init: where the optimiser starts"""

    def __init__(self, name, gt, truth, init, edges, meas, info, fixed):
        self.name, self.gt, self.truth, self.init = name, gt, truth, init
        self.edges = np.ascontiguousarray(edges, np.int32)
        self.meas, self.info = np.ascontiguousarray(meas), np.ascontiguousarray(info)
        self.fixed = np.ascontiguousarray(fixed, np.uint8)
        self.V, self.E = len(init), len(edges)


SIG = (0.01, 0.1, 0.05)              # rotation, translation, log-scale sigma of the scenes' information


def _info(E, sig=SIG):
    return np.tile(np.diag([1 / sig[0] ** 2] * 3 + [1 / sig[1] ** 2] * 3 + [1 / sig[2] ** 2]), (E, 1, 1))


def drift_loop(n=60, step=0.4 / 60, noise=0.0, skips=6, seed=21):
    """A ring of n keyframes mapped by a monocular tracker whose scale grows by e^step per keyframe.  The metric poses are
    gt; the local map around keyframe k is e^(k step) times too large, so the vertices at which every exact edge costs
    nothing are truth_k = (a_k, R_k, a_k t_k), a_k = e^(k step) (their metric poses [R | t/s] are gt).  Edges: n - 1 odometry
    edges, `skips` edges three keyframes ahead and the closing edge (n - 1, 0), each the exact S_j S_i^-1 of truth (noise = 0)
    or that times Phi(noise * N(0, SIG)).  init: the tracker's own trajectory, the SE(3) parts of the odometry edges chained
    with every s = 1 - it does not close."""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    a = 2 * np.pi * k / n
    p = np.stack([5 * np.cos(a), 5 * np.sin(a), 0.3 * np.sin(3 * a)], 1)
    gt = P._world_to_cam(P._rot_z(a + np.pi / 2) @ P._rot_y(0.1 * np.sin(2 * a)), p)
    ak = np.exp(step * k)
    truth = pack(ak, np.concatenate([gt[:, :, :3], ak[:, None, None] * gt[:, :, 3:]], 2))
    sk = (np.arange(skips) * (n // max(skips, 1)) + 5) % (n - 3)
    edges = np.concatenate([np.stack([k[:-1], k[1:]], 1), np.stack([sk, sk + 3], 1), [[n - 1, 0]]]).astype(np.int32)
    Z = mul(truth[edges[:, 1]], inv(truth[edges[:, 0]]))
    if noise > 0:
        Z = mul(phi(noise * rng.normal(0, 1, (len(edges), 7)) * np.array([SIG[0]] * 3 + [SIG[1]] * 3 + [SIG[2]])), Z)
    init = np.empty((n, 13))
    init[0] = truth[0]
    for q in range(n - 1):
        step_se3 = Z[q].copy()
        step_se3[12] = 1.0
        init[q + 1] = mul(step_se3, init[q])
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    return Scene("drift_loop", gt, truth, init, edges, Z, _info(len(edges)), fixed)


def _lift(scene, name, rng, scale_noise):
    """an SE(3) scene of pose_graph_ref in Sim(3) form; scale_noise > 0 perturbs the scales of start and measurements"""
    V, E = scene.V, scene.E
    sv = np.exp(rng.normal(0, scale_noise, V)) if scale_noise else np.ones(V)
    sv[np.flatnonzero(scene.fixed)] = 1.0
    sz = np.exp(rng.normal(0, SIG[2], E)) if scale_noise else np.ones(E)
    info = np.zeros((E, 7, 7))
    info[:, :6, :6] = scene.info
    info[:, 6, 6] = 1 / SIG[2] ** 2
    return Scene(name, scene.gt, pack(np.ones(V), scene.gt), pack(sv, scene.init), scene.edges, pack(sz, scene.meas), info, scene.fixed)


def hub(spokes=1000, seed=3):
    """pose_graph_ref.hub (a vertex of degree `spokes`) with noisy scales on the start and on the measurements"""
    return _lift(P.hub(spokes, seed=seed), "hub", np.random.default_rng(seed + 100), 0.05)


def sphere_s1(rings=50, per_ring=50):
    """pose_graph_ref.sphere - the SE(3) suite's own sphere, 2500 poses on a radius of 100 - lifted with every s = 1"""
    return _lift(P.sphere(rings, per_ring), "sphere_s1", None, 0.0)


def large(n=100_000):
    """pose_graph_ref.large (10^5 poses) lifted with noisy scales: for the timing tool only"""
    return _lift(P.large(n), "large", np.random.default_rng(19), 0.02)


SMALL_SCENES = {"drift_loop": lambda: drift_loop(noise=1.0), "hub": hub, "sphere_s1": sphere_s1}
