"""The numpy statement of the stereo / level-weighted adjustments (csrc/stereo_edge.h, pose_stereo.hip,
ba_stereo.hip): the edge model operation for operation in the header's order (so that float64 gives the header's bits), a
sequential Levenberg-Marquardt pose optimisation with g2o's schedule as oracle.pose_lm_np restates it, and a `linearize`
whose dict feeds ba_sparse_ref.reduce / pcg / backsub / lm unchanged.  Every function takes a dtype: np.longdouble is the
statement's own higher-precision run."""
import contextlib

import numpy as np

import ba_sparse_ref as R
from oracle import oracle

CHI2_MONO, CHI2_STEREO = 5.991, 7.815
GATES = (CHI2_MONO, CHI2_STEREO)
DELTAS = (CHI2_MONO ** 0.5, CHI2_STEREO ** 0.5)


def info_ok(info):
    info = np.asarray(info)
    with np.errstate(invalid="ignore"):
        return (info >= 0) & np.isfinite(info)


def edge(P, p, meas3, info, cam, deltas=(0.0, 0.0), dtype=np.float64):
    """The edges (P [O,12] pose rows, p [O,3] points, meas3 [O,3], info [O]) under cam = (fx, fy, cx, cy, bf): dict of X, Y, Z,
    e [O,3], stereo bool, s, chi2, w, rho, Jp [O,3,6], Jq [O,3,3]; the text of se_residual and se_jacobians."""
    f = dtype
    P, p, m = np.asarray(P, f).reshape(-1, 12), np.asarray(p, f).reshape(-1, 3), np.asarray(meas3, f).reshape(-1, 3)
    fx, fy, cx, cy, bf = (f(v) for v in cam)
    dm, ds = (f(v) for v in deltas)
    with np.errstate(all="ignore"):
        X = P[:, 0] * p[:, 0] + P[:, 1] * p[:, 1] + P[:, 2] * p[:, 2] + P[:, 3]
        Y = P[:, 4] * p[:, 0] + P[:, 5] * p[:, 1] + P[:, 6] * p[:, 2] + P[:, 7]
        Z = P[:, 8] * p[:, 0] + P[:, 9] * p[:, 1] + P[:, 10] * p[:, 2] + P[:, 11]
        u = (fx * X + cx * Z) / Z
        v = (fy * Y + cy * Z) / Z
        e0, e1 = m[:, 0] - u, m[:, 1] - v
        stereo = ~np.isnan(m[:, 2])
        c2 = e0 * e0 + e1 * e1
        e2 = np.where(stereo, m[:, 2] - (u - bf / Z), f(0))
        c2 = np.where(stereo, c2 + e2 * e2, c2)
        s = np.where(info_ok(info), np.asarray(info, f), f(0))
        chi2 = s * c2
        delta = np.where(stereo, ds, dm)
        en = np.sqrt(chi2)
        out = (delta > 0) & (en > delta)
        w = np.where(out, delta / np.where(out, en, f(1)), f(1))
        rho = np.where(out, f(2) * delta * en - delta * delta, chi2)
        Zinv = f(1) / (Z + f(1e-18))
        Zinv2 = Zinv * Zinv
        O = len(X)
        Jp, Jq = np.zeros((O, 3, 6), f), np.zeros((O, 3, 3), f)
        Jp[:, 0, 0] = fx * X * Y * Zinv2; Jp[:, 0, 1] = -fx - fx * X * X * Zinv2; Jp[:, 0, 2] = fx * Y * Zinv
        Jp[:, 0, 3] = -fx * Zinv; Jp[:, 0, 5] = fx * X * Zinv2
        Jp[:, 1, 0] = fy + fy * Y * Y * Zinv2; Jp[:, 1, 1] = -fy * X * Y * Zinv2; Jp[:, 1, 2] = -fy * X * Zinv
        Jp[:, 1, 4] = -fy * Zinv; Jp[:, 1, 5] = fy * Y * Zinv2
        A00, A02, A11, A12 = fx * Zinv, -fx * X * Zinv2, fy * Zinv, -fy * Y * Zinv2
        g = bf * Zinv2
        for c in range(3):
            Jq[:, 0, c] = -(A00 * P[:, c] + A02 * P[:, 8 + c])
            Jq[:, 1, c] = -(A11 * P[:, 4 + c] + A12 * P[:, 8 + c])
            Jq[:, 2, c] = np.where(stereo, Jq[:, 0, c] - g * P[:, 8 + c], f(0))
        Jp[:, 2, 0] = np.where(stereo, Jp[:, 0, 0] - g * Y, f(0)); Jp[:, 2, 1] = np.where(stereo, Jp[:, 0, 1] + g * X, f(0))
        Jp[:, 2, 2] = np.where(stereo, Jp[:, 0, 2], f(0)); Jp[:, 2, 3] = np.where(stereo, Jp[:, 0, 3], f(0))
        Jp[:, 2, 5] = np.where(stereo, Jp[:, 0, 5] - g, f(0))
    return dict(X=X, Y=Y, Z=Z, e=np.stack([e0, e1, e2], 1), stereo=stereo, s=s, chi2=chi2, w=w, rho=rho, Jp=Jp, Jq=Jq)


def inlier(E, gates=GATES):
    """se_inlier: information, positive depth, the gate of the kind."""
    with np.errstate(invalid="ignore"):
        return (E["s"] > 0) & (E["Z"] > 0) & (E["chi2"] <= np.where(E["stereo"], gates[1], gates[0]))


def edges_table(T12, X, op, ol, meas3, info, cam, deltas=(0.0, 0.0), gates=GATES):
    """The surface of slam_reproj_rj_stereo_f64 (and of the twin) over an observation table: an index outside its range gives
    NaN outputs, no inlier and one count; an information that is none counts once."""
    T12, X = np.asarray(T12, np.float64).reshape(-1, 12), np.asarray(X, np.float64).reshape(-1, 3)
    op, ol = np.asarray(op, np.int64), np.asarray(ol, np.int64)
    bad = (op < 0) | (op >= len(T12)) | (ol < 0) | (ol >= len(X))
    E = edge(T12[np.where(bad, 0, op)], X[np.where(bad, 0, ol)], meas3, info, cam, deltas)
    out = dict(e=E["e"], Jpose=E["Jp"], Jpoint=E["Jq"], chi2=E["chi2"], w=E["w"], rho=E["rho"], inlier=inlier(E, gates))
    for k in ("e", "Jpose", "Jpoint", "chi2", "w", "rho"):
        out[k] = out[k].copy()
        out[k][bad] = np.nan
    out["inlier"] = out["inlier"] & ~bad
    out["count"] = int(bad.sum() + (~info_ok(info) & ~bad).sum())
    return out


# ---- pose optimisation ----------------------------------------------------------------------------------------------------
def _exp(xi, dtype):
    """exp([w, v]) 4x4: scipy's matrix exponential in float64 (oracle.se3_exp_np), the closed form in any other dtype."""
    if dtype is np.float64:
        return oracle.se3_exp_np(np.asarray(xi, np.float64))
    f = dtype
    w, v = np.asarray(xi[:3], f), np.asarray(xi[3:], f)
    th = np.sqrt(w @ w)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], f)
    if th < f(1e-10):
        a, b, c = f(1), f(1) / f(2), f(1) / f(6)
    else:
        a, b, c = np.sin(th) / th, (f(1) - np.cos(th)) / (th * th), (th - np.sin(th)) / (th * th * th)
    T = np.eye(4, dtype=f)
    T[:3, :3] = np.eye(3, dtype=f) + a * W + b * (W @ W)
    T[:3, 3] = (np.eye(3, dtype=f) + b * W + c * (W @ W)) @ v
    return T


def _solve(A, b, dtype):
    """A x = b: numpy in float64, Gaussian elimination with partial pivoting otherwise; None for a singular system."""
    if dtype is np.float64:
        try:
            return np.linalg.solve(A, b)
        except np.linalg.LinAlgError:
            return None
    M = np.concatenate([np.array(A, dtype), np.array(b, dtype).reshape(-1, 1)], 1)
    n = len(M)
    for i in range(n):
        piv = i + int(np.argmax(np.abs(M[i:, i])))
        if M[piv, i] == 0:
            return None
        M[[i, piv]] = M[[piv, i]]
        M[i] = M[i] / M[i, i]
        for r in range(n):
            if r != i:
                M[r] = M[r] - M[r, i] * M[i]
    return M[:, n]


def pose_lm(pose, points, meas3, info, cam, rounds=4, iterations=10, gates=GATES, deltas=DELTAS, dtype=np.float64):
    """ORB-SLAM's PoseOptimization on arrays with the schedule of oracle.pose_lm_np: every round restarts from `pose`, up to ten
    trials per iteration, the active set recomputed from the classification of ALL edges after every round, the kernel
    dropped after round index 2.  An edge with information 0 is never active.
    -> (T 4x4, inliers bool [O], weighted chi2 [O] at T, accepted steps, stereo inliers)."""
    f = dtype
    P = np.asarray(pose, f)
    T0 = np.eye(4, dtype=f)
    T0[:3, :4] = P.reshape(3, 4) if P.size == 12 else P.reshape(-1, 4)[:3, :4]
    points = np.asarray(points, f).reshape(-1, 3)
    O = len(points)
    info = np.asarray(info, np.float64).reshape(-1)
    active = np.where(info_ok(info), info, 0.0) > 0
    dl = tuple(deltas)
    accepted = 0

    def evaluate(Tm):
        E = edge(np.broadcast_to(Tm[:3, :4].reshape(1, 12), (O, 12)), points, meas3, info, cam, dl, f)
        ws = (E["w"] * E["s"])[active]
        Jp, e = E["Jp"][active], E["e"][active]
        H = np.einsum("o,oia,oib->ab", ws, Jp, Jp)
        b = np.einsum("o,oia,oi->a", ws, Jp, e)
        return H, b, E["rho"][active].sum(), E

    T, E = T0, None
    for rnd in range(rounds):
        T = T0.copy()
        H, b, cur, E = evaluate(T)
        lam = f(1e-5) * max(np.max(np.diag(H)) if O else f(0), f(1e-12))
        ni = f(2)
        for _ in range(iterations):
            if not active.any():
                break
            stepped = False
            for _trial in range(10):
                dx = _solve(H + lam * np.eye(6, dtype=f), -b, f)
                if dx is None:
                    lam, ni = lam * ni, ni * 2
                    continue
                Tn = _exp(dx, f) @ T
                Hn, bn, new, En = evaluate(Tn)
                rho = (cur - new) / (dx @ (lam * dx - b) + f(1e-3))
                if rho > 0 and np.isfinite(new):
                    T, H, b, cur, E = Tn, Hn, bn, new, En
                    lam = lam * max(f(1) / f(3), min(f(1) - (f(2) * rho - f(1)) ** 3, f(2) / f(3)))
                    ni = f(2)
                    stepped = True
                    accepted += 1
                    break
                lam, ni = lam * ni, ni * 2
                if not np.isfinite(lam):
                    break
            if not stepped:
                break
        active = inlier(E, gates)
        if rnd == 2:
            dl = (0.0, 0.0)
    if E is None:
        E = edge(np.broadcast_to(T0[:3, :4].reshape(1, 12), (O, 12)), points, meas3, info, cam, (0.0, 0.0), f)
        active = inlier(E, gates)
    return T, active, E["chi2"], accepted, int((active & E["stereo"]).sum())


# ---- sparse bundle adjustment ----------------------------------------------------------------------------------------------
def linearize(T12, X, op, ol, meas3, info, cam, deltas):
    """ba_sparse_ref.linearize with the stereo / weighted edge model: the dict its reduce / pcg / backsub take.  An edge with
    information 0 adds nothing (its terms are dropped, not multiplied by 0)."""
    T12 = np.ascontiguousarray(T12, np.float64).reshape(-1, 12)
    X = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
    K, L = len(T12), len(X)
    op, ol = np.asarray(op, np.int64), np.asarray(ol, np.int64)
    E = edge(T12[op], X[ol], meas3, info, cam, deltas)
    on = E["s"] > 0
    ws = np.where(on, E["w"] * E["s"], 0.0)
    Jp, Jq, e = np.where(on[:, None, None], E["Jp"], 0.0), np.where(on[:, None, None], E["Jq"], 0.0), np.where(on[:, None], E["e"], 0.0)
    rho = np.where(on, E["rho"], 0.0)
    cost_pose = np.zeros(K)
    np.add.at(cost_pose, op, rho)
    Jpw, Jqw = Jp * ws[:, None, None], Jq * ws[:, None, None]
    Hpp, bp, Hll, bl = np.zeros((K, 6, 6)), np.zeros((K, 6)), np.zeros((L, 3, 3)), np.zeros((L, 3))
    np.add.at(Hpp, op, np.einsum("oia,oib->oab", Jpw, Jp))
    np.add.at(bp, op, np.einsum("oia,oi->oa", Jpw, e))
    np.add.at(Hll, ol, np.einsum("oia,oib->oab", Jqw, Jq))
    np.add.at(bl, ol, np.einsum("oia,oi->oa", Jqw, e))
    return dict(Hpp=Hpp, bp=bp, Hll=Hll, bl=bl, Hpl=np.einsum("oia,oib->oab", Jpw, Jq), cost=float(rho.sum()), cost_pose=cost_pose, K=K, L=L)


def cost_at(T12, X, op, ol, meas3, info, cam, deltas):
    T12 = np.ascontiguousarray(T12, np.float64).reshape(-1, 12)
    E = edge(T12[np.asarray(op, np.int64)], np.asarray(X, np.float64).reshape(-1, 3)[np.asarray(ol, np.int64)], meas3, info, cam, deltas)
    return float(np.where(E["s"] > 0, E["rho"], 0.0).sum())


def classify(T12, X, op, ol, meas3, info, cam, gates=GATES):
    """(weighted chi2 [O], inlier bool [O]) at a state."""
    T12 = np.ascontiguousarray(T12, np.float64).reshape(-1, 12)
    E = edge(T12[np.asarray(op, np.int64)], np.asarray(X, np.float64).reshape(-1, 3)[np.asarray(ol, np.int64)], meas3, info, cam)
    return E["chi2"], inlier(E, gates)


# Roundings on the way to one entry of Hpl or E (ba_sparse_ref.CHAIN_ROUNDINGS = 40) grow by the product w s (1), the third
# row's Jacobian entry (g = bf Zinv^2, g Y, the difference: 3) and the third product and sum of (w s) Jp^T Jq (2): 46.  The
# sums themselves grow from 2 to 3 products per observation in Hpp (11 -> 13 roundings per term of a diagonal block) and in
# bl (5 -> 6 per term of b).  ba_sparse_ref.reduce returns (terms n + chain) kappa 2^-52 sum|terms|, so its bound times
# max(46 / 40, 13 / 11, 6 / 5) = 1.2 covers every entry of the extended construction.
BOUND_FACTOR = 1.2


@contextlib.contextmanager
def _stereo_model():
    """ba_sparse_ref.lm calls its module's linearize and cost_at with (T12, X, op, ol, meas, intr, delta); for the span of one
    call they are the two functions above, with meas = (meas3, info), intr = cam and delta = the pair of widths."""
    keep = R.linearize, R.cost_at
    R.linearize = lambda T12, X, op, ol, meas, cam, dl: linearize(T12, X, op, ol, meas[0], meas[1], cam, dl)
    R.cost_at = lambda T12, X, op, ol, meas, cam, dl: cost_at(T12, X, op, ol, meas[0], meas[1], cam, dl)
    try:
        yield
    finally:
        R.linearize, R.cost_at = keep


def lm(T0, X0, op, ol, meas3, info, cam, iterations, fixed_poses, deltas, pcg_tol=1e-10, pcg_max_iter=500):
    """ba_sparse_ref.lm, unchanged, on the stereo / weighted model -> (T [K,4,4], X, cost0, cost, accepted, stats)."""
    with _stereo_model():
        return R.lm(T0, X0, op, ol, (meas3, info), cam, iterations, fixed_poses, deltas, pcg_tol, pcg_max_iter)


def local_ba(T0, X0, op, ol, meas3, info, cam, fixed_poses, first=5, second=10, gates=GATES, deltas=DELTAS):
    """LocalBundleAdjustment's schedule on the statement -> (T, X, outliers int64 ascending, outliers after the first stage)."""
    info = np.asarray(info, np.float64)
    rt = lambda Tm: Tm[:, :3, :4].reshape(len(Tm), 12)  # noqa: E731
    T, X, *_ = lm(T0, X0, op, ol, meas3, info, cam, first, fixed_poses, deltas)
    _, inl = classify(rt(T), X, op, ol, meas3, info, cam, gates)
    off = np.where(inl, info, 0.0)
    T, X, *_ = lm(T, X, op, ol, meas3, off, cam, second, fixed_poses, (0.0, 0.0))
    _, inl2 = classify(rt(T), X, op, ol, meas3, off, cam, gates)
    return T, X, np.flatnonzero(~inl2 & (info > 0)), np.flatnonzero(~inl & (info > 0))
