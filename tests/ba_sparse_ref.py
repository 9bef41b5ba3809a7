"""The numpy statement of the sparse bundle adjustment (slamhip/ba_sparse.py, csrc/ba_sparse.hip): point elimination into
diagonal and covisibility-edge blocks, back-substitution, and the Levenberg-Marquardt loop of bundle_adjust_device with a
plain block-Jacobi preconditioned CG in place of the dense solve.  Residuals and Jacobians come from the C oracle
(oracle.reproj_rj_c); the covisibility edges are built here by brute force, point by point, not by the product's function.
Shared by tests/test_ba_sparse_cpu.py and tests/test_ba_sparse_gpu.py; tests/test_ba_limits_gpu.py takes its scenes from here."""
import numpy as np

from oracle import oracle

EPS = 2.0 ** -52
# roundings on the way to ONE entry of Hpl or E before any sum over pairs starts: the projection (12), a Jacobian entry (6),
# the Huber weight (4), the two products of w Jp^T Jq (4), a cofactor and the determinant of the 3x3 inverse (14)
CHAIN_ROUNDINGS = 40


def brute_covisibility(op, ol, K, fixed):
    """{(k1, k2): [(l, obs of (k1, l), obs of (k2, l)), ...] ascending in l} over the free poses, by sets."""
    fixed = np.asarray(fixed, bool)
    seen = {}
    for o, (k, l) in enumerate(zip(np.asarray(op).tolist(), np.asarray(ol).tolist())):
        seen.setdefault(l, []).append((k, o))
    out = {}
    for l in sorted(seen):
        obs = sorted(seen[l])
        for i in range(len(obs)):
            for j in range(i + 1, len(obs)):
                (k1, a), (k2, b) = obs[i], obs[j]
                if not fixed[k1] and not fixed[k2]:
                    out.setdefault((k1, k2), []).append((l, a, b))
    return out


def linearize(T12, X, op, ol, meas, intr, delta):
    """Blocks at a state: Hpp [K,6,6], bp [K,6], Hll [L,3,3], bl [L,3], Hpl [O,6,3], cost, cost_pose [K]."""
    T12 = np.ascontiguousarray(T12, np.float64).reshape(-1, 12)
    X = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
    K, L = len(T12), len(X)
    e, Jp, Jq = oracle.reproj_rj_c(T12, X, op, ol, meas, *intr, with_point=True)
    c2 = (e * e).sum(1)
    s = np.sqrt(c2)
    out = (delta > 0) & (s > delta)
    w = np.where(out, delta / np.where(out, s, 1.0), 1.0)
    rho = np.where(out, 2.0 * delta * s - delta * delta, c2)
    cost, cost_pose = float(rho.sum()), np.zeros(K)
    np.add.at(cost_pose, op, rho)
    Jpw, Jqw = Jp * w[:, None, None], Jq * w[:, None, None]
    Hpp, bp, Hll, bl = np.zeros((K, 6, 6)), np.zeros((K, 6)), np.zeros((L, 3, 3)), np.zeros((L, 3))
    np.add.at(Hpp, op, np.einsum("oia,oib->oab", Jpw, Jp))
    np.add.at(bp, op, np.einsum("oia,oi->oa", Jpw, e))
    np.add.at(Hll, ol, np.einsum("oia,oib->oab", Jqw, Jq))
    np.add.at(bl, ol, np.einsum("oia,oi->oa", Jqw, e))
    return dict(Hpp=Hpp, bp=bp, Hll=Hll, bl=bl, Hpl=np.einsum("oia,oib->oab", Jpw, Jq), cost=cost, cost_pose=cost_pose, K=K, L=L)


def reduce(lin, op, ol, fixed, lam, cov=None):
    """The reduced system at damping lam: edges [E,2], Hdiag [K,6,6] (without lam), W [E,6,6], b [K,6], E [L,3,3] (0 for
    points nobody observes), and a rounding bound per entry of Hdiag, W and b (see `bound`)."""
    K, L = lin["K"], lin["L"]
    op, ol = np.asarray(op, np.int64), np.asarray(ol, np.int64)
    cov = brute_covisibility(op, ol, K, fixed) if cov is None else cov
    keys = sorted(cov)
    edges = np.array(keys, np.int32).reshape(-1, 2)
    seen = np.zeros(L, bool)
    seen[ol] = True
    M = lin["Hll"] + lam * np.eye(3)
    M[~seen] = np.eye(3)
    Einv = np.linalg.inv(M)
    kappa = np.linalg.cond(M)
    Einv[~seen] = 0.0
    Hpl, aH, aE = lin["Hpl"], np.abs(lin["Hpl"]), np.abs(Einv)
    pe = np.array([i for i, k in enumerate(keys) for _ in cov[k]], np.int64)
    pl = np.array([t[0] for k in keys for t in cov[k]], np.int64)
    pa = np.array([t[1] for k in keys for t in cov[k]], np.int64)
    pb = np.array([t[2] for k in keys for t in cov[k]], np.int64)
    E = len(keys)
    W, aW, kW, nW = np.zeros((E, 6, 6)), np.zeros((E, 6, 6)), np.ones(E), np.zeros(E)
    if len(pe):
        np.add.at(W, pe, -np.einsum("pab,pbc,pdc->pad", Hpl[pa], Einv[pl], Hpl[pb]))
        np.add.at(aW, pe, np.einsum("pab,pbc,pdc->pad", aH[pa], aE[pl], aH[pb]))
        np.maximum.at(kW, pe, kappa[pl])
        np.add.at(nW, pe, 1.0)
    Y = np.einsum("oab,obc->oac", Hpl, Einv[ol])
    Hdiag, b = lin["Hpp"].copy(), lin["bp"].copy()
    np.subtract.at(Hdiag, op, np.einsum("oac,odc->oad", Y, Hpl))
    np.subtract.at(b, op, np.einsum("oac,oc->oa", Y, lin["bl"][ol]))
    aD, ab, kD, nD = np.abs(lin["Hpp"]), np.abs(lin["bp"]), np.ones(K), np.zeros(K)
    aY = np.einsum("oab,obc->oac", aH, aE[ol])
    np.add.at(aD, op, np.einsum("oac,odc->oad", aY, aH))
    np.add.at(ab, op, np.einsum("oac,oc->oa", aY, np.abs(lin["bl"])[ol]))
    np.maximum.at(kD, op, kappa[ol])
    np.add.at(nD, op, 1.0)
    # bound: (terms of the sum + the roundings before it) * 2^-52 * sum of |terms| * the worst condition number of the 3x3
    # inverses involved; a diagonal block also sums its pose's Hpp terms (2 products per observation), bl_l is itself a sum
    # over the point's track, which the factor 2 on the chain covers
    bound = dict(W=((9 * nW + CHAIN_ROUNDINGS) * kW)[:, None, None] * EPS * aW,
                 Hdiag=((11 * nD + CHAIN_ROUNDINGS) * kD)[:, None, None] * EPS * aD,
                 b=((5 * nD + 2 * CHAIN_ROUNDINGS) * kD)[:, None] * EPS * ab)
    return dict(edges=edges, Hdiag=Hdiag, W=W, b=b, E=Einv, seen=seen, bound=bound, weights=nW.astype(np.int64))


def hmul(red, fixed, lam, x):
    """(S + lam I) x over the free poses (rows of fixed poses 0, their columns ignored)."""
    free = ~np.asarray(fixed, bool)
    x = np.asarray(x, np.float64).reshape(-1, 6) * free[:, None]
    y = np.einsum("kab,kb->ka", red["Hdiag"], x) + lam * x
    e0, e1 = red["edges"][:, 0], red["edges"][:, 1]
    if len(e0):
        np.add.at(y, e0, np.einsum("eab,eb->ea", red["W"], x[e1]))
        np.add.at(y, e1, np.einsum("eba,eb->ea", red["W"], x[e0]))
    return y * free[:, None]


def dense_system(red, lam):
    """S + lam I as a [K,K,6,6] array."""
    K = len(red["Hdiag"])
    S = np.zeros((K, K, 6, 6))
    kk = np.arange(K)
    S[kk, kk] = red["Hdiag"] + lam * np.eye(6)
    e0, e1 = red["edges"][:, 0], red["edges"][:, 1]
    S[e0, e1] = red["W"]
    S[e1, e0] = red["W"].transpose(0, 2, 1)
    return S


def pcg(red, fixed, lam, tol, max_iter):
    """Block-Jacobi preconditioned CG on (S + lam I) x = -b over the free poses -> (x [K,6], iterations, converged)."""
    free = ~np.asarray(fixed, bool)
    Minv = np.linalg.inv(red["Hdiag"] + lam * np.eye(6))
    r = -red["b"] * free[:, None]
    x = np.zeros_like(r)
    bb = float((r * r).sum())
    if bb == 0.0:
        return x, 0, True
    z = np.einsum("kab,kb->ka", Minv, r) * free[:, None]
    p, rz = z.copy(), float((r * z).sum())
    for n in range(1, max_iter + 1):
        q = hmul(red, fixed, lam, p)
        pq = float((p * q).sum())
        if not pq > 0:
            return x, n, False
        alpha = rz / pq
        x += alpha * p
        r -= alpha * q
        if float((r * r).sum()) <= tol * tol * bb:
            return x, n, True
        z = np.einsum("kab,kb->ka", Minv, r) * free[:, None]
        rz, old = float((r * z).sum()), rz
        p = z + (rz / old) * p
    return x, max_iter, False


def backsub(lin, red, op, ol, dp):
    """dl_l = -E_l (bl_l + sum_{o of l} Hpl_o^T dp_pose(o))."""
    t = lin["bl"].copy()
    np.add.at(t, ol, np.einsum("oab,oa->ob", lin["Hpl"], np.asarray(dp).reshape(-1, 6)[op]))
    return -np.einsum("lab,lb->la", red["E"], t)


def cost_at(T12, X, op, ol, meas, intr, delta):
    e, _, _ = oracle.reproj_rj_c(np.ascontiguousarray(T12).reshape(-1, 12), X, op, ol, meas, *intr, with_point=False)
    c2 = (e * e).sum(1)
    if delta <= 0:
        return float(c2.sum())
    s = np.sqrt(c2)
    return float(np.where(s <= delta, c2, 2.0 * delta * s - delta * delta).sum())


def lm(T0, X0, op, ol, meas, intr, iterations, fixed_poses, delta, pcg_tol=1e-10, pcg_max_iter=500):
    """The schedule of bundle_adjust_device (lambda_0 = 1e-5 * largest diagonal entry over free poses and points, the gain
    ratio, ten trials) with `pcg` for the solve; a solve that does not converge is a failed trial.
    -> (T [K,4,4], X, cost0, cost, accepted, stats dict)."""
    T = np.array(T0, np.float64)
    X = np.array(X0, np.float64).reshape(-1, 3)
    K = len(T)
    op, ol = np.asarray(op, np.int32), np.asarray(ol, np.int32)
    fixed = np.zeros(K, bool)
    fixed[list(fixed_poses)] = True
    cov = brute_covisibility(op, ol, K, fixed)
    rt = lambda Tm: Tm[:, :3, :4].reshape(K, 12)
    lin = linearize(rt(T), X, op, ol, meas, intr, delta)
    cost0 = cost = lin["cost"]
    dmax = max(lin["Hpp"][~fixed].reshape(-1, 36)[:, ::7].max(initial=0.0), lin["Hll"].reshape(-1, 9)[:, ::4].max(initial=0.0))
    lam, ni, accepted = 1e-5 * max(dmax, 1e-12), 2.0, 0
    st = dict(trials=0, cg_iterations=0, unconverged=0, edges=len(cov))
    for _ in range(iterations):
        step_ok = False
        for _trial in range(10):
            st["trials"] += 1
            red = reduce(lin, op, ol, fixed, lam, cov)
            dp, n, conv = pcg(red, fixed, lam, pcg_tol, pcg_max_iter)
            st["cg_iterations"] += n
            if not conv:
                st["unconverged"] += 1
                lam *= ni; ni *= 2
                continue
            dl = backsub(lin, red, op, ol, dp)
            Tn = np.stack([T[k] if fixed[k] else oracle.se3_exp_np(dp[k]) @ T[k] for k in range(K)])
            Xn = X + dl
            new = cost_at(rt(Tn), Xn, op, ol, meas, intr, delta)
            scale = float((dp * (lam * dp - lin["bp"]))[~fixed].sum() + (dl * (lam * dl - lin["bl"])).sum()) + 1e-3
            rho = (cost - new) / scale
            if rho > 0 and np.isfinite(new):
                T, X, cost = Tn, Xn, new
                lin = linearize(rt(T), X, op, ol, meas, intr, delta)
                lam *= max(1.0 / 3.0, min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0))
                ni = 2.0
                accepted += 1
                step_ok = True
                break
            lam *= ni; ni *= 2
        if not step_ok:
            break
    st["lam"] = lam
    return T, X, cost0, cost, accepted, st


# ---- scenes (`scene` and `window` also build the windows of tests/test_ba_limits_gpu.py: its intrinsics, shuffled observations, 0.3 px noise) -----
FX, FY, CX, CY = 458.654, 457.296, 367.215, 248.375
INTR = (FX, FY, CX, CY)


def scene(rng, K, L):
    from scipy.spatial.transform import Rotation

    T = np.tile(np.eye(4), (K, 1, 1))
    T[:, :3, :3] = Rotation.from_rotvec(rng.uniform(-0.15, 0.15, (K, 3))).as_matrix()
    T[:, :3, 3] = rng.uniform(-0.5, 0.5, (K, 3))
    X = np.c_[rng.uniform(-4, 4, (L, 2)), rng.uniform(6, 15, L)]
    return T, X


def window(rng, T, X, op, ol, fixed, noise=0.3):
    """Shuffle the observations, measure them with pixel noise, perturb the moving poses and every point."""
    K = T.shape[0]
    perm = rng.permutation(len(op))
    op, ol = np.asarray(op, np.int32)[perm], np.asarray(ol, np.int32)[perm]
    pc = np.einsum("oij,oj->oi", T[op, :3, :3], X[ol]) + T[op, :3, 3]
    meas = np.c_[FX * pc[:, 0] / pc[:, 2] + CX, FY * pc[:, 1] / pc[:, 2] + CY] + rng.normal(0, noise, (len(op), 2))
    T0 = T.copy()
    for k in range(K):
        if k not in fixed:
            T0[k] = oracle.se3_exp_np(rng.normal(0, 0.01, 6)) @ T[k]
    X0 = X + rng.normal(0, 0.05, X.shape)
    return dict(T0=T0, X0=X0, op=op, ol=ol, meas=meas, fixed=tuple(fixed), T=T, X=X)


def chain_tracks(rng, first, last, O, lo=2, hi=6):
    """Tracks over lo..hi consecutive poses of [first, last], exactly O observations (the last track takes what is left)."""
    spans, left = [], O
    while left > 0:
        n = min(int(rng.integers(lo, hi + 1)), left)
        spans.append(np.arange(n) + int(rng.integers(first, last - n + 2)))
        left -= n
    return spans


def tracks_window(rng, K, tracks, fixed):
    """One point per track (the list of poses that see it; an empty track is a point nobody observes)."""
    tracks = [np.asarray(t, np.int64) for t in tracks]
    T, X = scene(rng, K, len(tracks))
    op = np.concatenate(tracks)
    ol = np.concatenate([np.full(len(t), i) for i, t in enumerate(tracks)])
    return window(rng, T, X, op, ol, fixed)


def sliding(rng, K, O, fixed=(0, 1), lo=2, hi=6):
    """A keyframe chain: every point seen by lo..hi consecutive poses, exactly O observations."""
    return tracks_window(rng, K, chain_tracks(rng, 0, K - 1, O, lo, hi), fixed)


def uneven(rng):
    """K = 7: poses 0 and 1 fixed and well observed (the gauge), pose 6 fixed with no observation; pose 2 moving with no
    observation, pose 3 moving with two, pose 4 moving with more than half of all observations, pose 5 moving.  Points seen
    by every pose that sees anything (0, 1, 4, 5; two of them by pose 3 too), points seen by pose 4 and one gauge pose,
    by poses 4 and 5, by pose 4 alone, and points nobody sees."""
    A, D, E, B, C = 1000, 11000, 4000, 3000, 500
    L = A + D + E + B + C
    T, X = scene(rng, 7, L)
    a, d, e, b = np.arange(A), A + np.arange(D), A + D + np.arange(E), A + D + E + np.arange(B)
    op = np.concatenate([np.repeat([0, 1, 4, 5], A), np.full(D, 4), d % 2, np.full(E, 4), np.full(E, 5), np.full(B, 4), [3, 3]])
    ol = np.concatenate([np.tile(a, 4), d, d, e, e, b, [a[0], a[A // 2]]])
    return window(rng, T, X, op, ol, (0, 1, 6))


def smallest(rng):
    """K = 3, poses 0 and 1 fixed, pose 2 moving; 12 points: pose 0 sees one of them, poses 1 and 2 all of them."""
    T, X = scene(rng, 3, 12)
    op = np.concatenate([[0], np.ones(12, int), np.full(12, 2)])
    ol = np.concatenate([[5], np.arange(12), np.arange(12)])
    return window(rng, T, X, op, ol, (0, 1))


def case_edges(seed=23):
    """K = 23, poses 0, 9 and 15 fixed (scattered), a chain of tracks of 2 to 6 over poses 0..20, and on top of it:
    ONE point shared by poses 1 and 20 (an edge of exactly one pair), 130 points shared by poses 2 and 19 (an edge of 130
    pairs: more than a wave, not a multiple of 64), three tracks of length 1, two points nobody observes, two points seen
    only by fixed poses, pose 21 free WITHOUT an observation, pose 22 free with 40 points it shares with fixed pose 0 alone
    (no covisible neighbour).  23 poses and the edge count are no multiples of 4 (edges per workgroup) or 64."""
    rng = np.random.default_rng(seed)
    tracks = chain_tracks(rng, 0, 20, 2000)
    n_chain = len(tracks)
    tracks += [[1, 20]] + [[2, 19]] * 130 + [[5], [12], [20]] + [[], []] + [[0, 9], [9, 15]] + [[0, 22]] * 40
    w = tracks_window(rng, 23, tracks, (0, 9, 15))
    w["unseen"] = [n_chain + 134, n_chain + 135]
    return w


def case_hub(seed=41):
    """K = 41, pose 0 fixed, a chain of tracks of 2 to 6, and one point seen by all 40 free poses: 780 pairs from one point,
    every pair of free poses an edge (780 edges).  Every vertex has 39 neighbours: with K <= 64 none can pass the 128 slots
    above which the solver's product treats a vertex as a hub, so that path is left to the solver's own tests."""
    rng = np.random.default_rng(seed)
    tracks = chain_tracks(rng, 0, 40, 4000) + [np.arange(1, 41)]
    return tracks_window(rng, 41, tracks, (0,))


def case_chain512(seed=512):
    """A chain of 512 keyframes and about 6 000 points with tracks of 2 to 6, the gauge held by poses 0 and 1."""
    rng = np.random.default_rng(seed)
    return tracks_window(rng, 512, chain_tracks(rng, 0, 511, 24000), (0, 1))
