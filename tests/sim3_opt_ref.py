"""numpy statement of slam_sim3_optimize_f64 (include/slamhip.h), written from the header on another route than the kernel.

Imports neither the product nor the twin.  The kernel forms analytic Jacobians, sums in a stated lane order and solves by
LDL^T; this file takes the Jacobians by CENTRAL DIFFERENCES of its own residual through its own retraction, sums with plain
numpy and solves with ``np.linalg.solve``.  The schedule (activity, stage 1 with Huber, the gate, rejection, stage 2, the
final gate) and g2o's Levenberg-Marquardt are restated here in full, so an agreement of the two is not an agreement of one
piece of code with itself.

Also the scene list of the tests: EuRoC intrinsics, 752 x 480 image, X1 from pixels uniform in the image and a depth range,
X2 = s R X1 + t, keypoints = projections + Gaussian pixel noise; a planted outlier is a wrong match: X2 and its keypoint
belong to a point whose image is 20 - 80 px away from the right one."""
from __future__ import annotations

import numpy as np

import sim3_ref as base

EUROC = base.EUROC
TH2 = 10.0
ITERATIONS = (5, 10, 5)
MIN_PAIRS = 10
SEED = 4242
STEP = 1e-6                           # central-difference step in the tangent space
REJECTED, BAD_MODEL, STALLED = 1, 2, 4
pack, split = base.pack, base.split


# ---------------------------------------------------------------- residual, chart
def project(P, K):
    with np.errstate(all="ignore"):
        return np.stack([K[0] * (P[:, 0] / P[:, 2]) + K[2], K[1] * (P[:, 1] / P[:, 2]) + K[3]], 1)


def residual(model, sc, K):
    """(e2 [n,2], e1 [n,2], z [n], wz [n]) at a model."""
    s, R, t = split(np.asarray(model, np.float64))
    with np.errstate(all="ignore"):
        Y = s * (sc["X1"] @ R.T) + t
        W = (sc["X2"] - t) @ R
        return sc["px2"] - project(Y, K), sc["px1"] - project(W, K), Y[:, 2], W[:, 2]


def chi2(model, sc, K):
    """(c [n,2] = (c1, c2), front bool [n])."""
    e2, e1, z, wz = residual(model, sc, K)
    with np.errstate(all="ignore"):
        c = np.stack([(e1 * e1).sum(1) / sc["sigma2"][:, 0], (e2 * e2).sum(1) / sc["sigma2"][:, 1]], 1)
        return c, (z > 0) & (wz > 0)


def retract(model, x):
    s, R, t = split(np.asarray(model, np.float64))
    a = np.asarray(x[:3]) / 2
    n = a @ a
    ax = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    Rd = ((1 - n) * np.eye(3) + 2 * np.outer(a, a) + 2 * ax) / (1 + n)
    sd = 1 + x[6] + x[6] * x[6] / 2
    return pack(sd * s, Rd @ R, sd * (Rd @ t) + np.asarray(x[3:6]))


def huber(c, delta):
    """(weight, rho) of chi2 values c."""
    if delta <= 0:
        return np.ones_like(c), c
    with np.errstate(all="ignore"):
        q = np.sqrt(c)
        over = q > delta
        return np.where(over, delta / np.where(over, q, 1.0), 1.0), np.where(over, 2 * delta * q - delta * delta, c)


def cost(model, sc, K, active, delta):
    """(robust cost over the active pairs, True when an active pair is not in front of both cameras)."""
    c, front = chi2(model, sc, K)
    _, rho = huber(c[active], delta)
    return float(rho.sum()), bool((~front[active]).any())


def stacked(model, sc, K):
    e2, e1, _, _ = residual(model, sc, K)
    return np.concatenate([e2, e1], 1)                   # [n,4]


def jacobian(model, sc, K, fix_scale=False):
    """[n,4,7] by central differences through the retraction (rows: e2, e1; columns [omega, upsilon, sigma])."""
    J = np.zeros((len(sc["X1"]), 4, 7))
    for k in range(6 if fix_scale else 7):
        x = np.zeros(7)
        x[k] = STEP
        J[:, :, k] = (stacked(retract(model, x), sc, K) - stacked(retract(model, -x), sc, K)) / (2 * STEP)
    return J


def linearize(model, sc, K, active, delta, fix_scale=False):
    """(H [7,7], b [7], cost) over the active pairs."""
    idx = np.flatnonzero(active)
    sub = {k: sc[k][idx] for k in ("X1", "X2", "px1", "px2", "sigma2")}
    e, J = stacked(model, sub, K), jacobian(model, sub, K, fix_scale)
    c, _ = chi2(model, sub, K)
    w, rho = huber(c, delta)
    H, b = np.zeros((7, 7)), np.zeros(7)
    for edge, (rows, col) in enumerate((((0, 1), 1), ((2, 3), 0))):          # edge 2 (sigma2 column 1), edge 1 (column 0)
        Je, ee, we = J[:, rows, :], e[:, rows], w[:, col] / sub["sigma2"][:, col]
        H += np.einsum("n,nra,nrb->ab", we, Je, Je)
        b += np.einsum("n,nra,nr->a", we, Je, ee)
    return H, b, float(rho.sum())


# ---------------------------------------------------------------- Levenberg-Marquardt and the schedule
def run_stage(model, sc, K, active, delta, iters, fix_scale, work):
    """(model, accepted steps, stalled)."""
    accepted, lam, ni = 0, 0.0, 2.0
    for it in range(iters):
        H, b, F = linearize(model, sc, K, active, delta, fix_scale)
        work["linearisations"] += 1
        if it == 0:
            lam = 1e-5 * max(float(np.diag(H).max()), 1e-12)
        took = False
        for _ in range(10):
            work["trials"] += 1
            ok, rho = False, -1.0
            A = H + lam * np.eye(7)
            try:
                np.linalg.cholesky(A)
                x = np.linalg.solve(A, -b)
                ok = bool(np.isfinite(x).all())
            except np.linalg.LinAlgError:
                ok = False
            if ok:
                if fix_scale:
                    x[6] = 0.0
                cand = retract(model, x)
                ok = bool(np.isfinite(cand).all() and cand[12] > 0)
            if ok:
                Fn, bad = cost(cand, sc, K, active, delta)
                ok = bool(np.isfinite(Fn)) and not bad
                rho = (F - Fn) / (float(x @ (lam * x - b)) + 1e-3)
            if ok and rho > 0:
                model = cand
                lam *= max(1 / 3, min(1 - (2 * rho - 1) ** 3, 2 / 3))
                ni = 2.0
                accepted += 1
                took = True
                break
            lam *= ni
            ni *= 2
        if not took:
            return model, accepted, True
    return model, accepted, False


def start_activity(model, sc, K):
    data = np.concatenate([sc["X1"], sc["X2"], sc["px1"], sc["px2"], sc["sigma2"]], 1)
    with np.errstate(all="ignore"):
        ok = np.isfinite(data).all(1) & (sc["X1"][:, 2] > 0) & (sc["X2"][:, 2] > 0) & (sc["sigma2"] > 0).all(1)
        _, front = chi2(model, sc, K)
    return ok & front


def optimize(sc, model_in, K=EUROC, th2=TH2, iterations=ITERATIONS, min_pairs=MIN_PAIRS, fix_scale=False):
    """The whole call for one candidate: dict(model, mask, chi2, stats, start_active, work, fitted = the pairs stage 2 ran on)."""
    sc = dict(sc)
    n = len(sc["X1"])
    if sc.get("sigma2") is None:
        sc["sigma2"] = np.ones((n, 2))
    model_in = np.asarray(model_in, np.float64)
    work = dict(trials=0, linearisations=0)
    none = dict(mask=np.zeros(n, bool), chi2=np.full((n, 2), np.nan), start_active=np.zeros(n, bool), work=work)
    if not (np.isfinite(model_in).all() and model_in[12] > 0):
        return dict(none, model=base.IDENTITY.copy(), stats=np.array([0, 0, 0, REJECTED | BAD_MODEL], np.int32))
    active = start_activity(model_in, sc, K)
    live = active.copy()
    model, accepted, status, nbad = model_in.copy(), 0, 0, 0
    for stage in range(2):
        delta = np.sqrt(th2) if stage == 0 else 0.0
        iters = iterations[0] if stage == 0 else (iterations[1] if nbad > 0 else iterations[2])
        model, acc, stalled = run_stage(model, sc, K, active, delta, iters, fix_scale, work)
        accepted += acc
        status |= STALLED if stalled else 0
        c, front = chi2(model, sc, K)
        with np.errstate(all="ignore"):
            keep = active & (c[:, 0] <= th2) & (c[:, 1] <= th2) & front
        if stage == 0:
            nbad = int(active.sum() - keep.sum())
            fitted = keep
        active = keep
        if stage == 0 and active.sum() < min_pairs:
            return dict(none, model=model_in.copy(), start_active=live, stats=np.array([0, accepted, nbad, status | REJECTED], np.int32))
    return dict(model=model, mask=active, chi2=np.where(live[:, None], c, np.nan), start_active=live, work=work, fitted=fitted,
                stats=np.array([int(active.sum()), accepted, nbad, status], np.int32))


def polished(sc, model, mask, K=EUROC, fix_scale=False, steps=40):
    """The minimiser of the plain (no kernel) cost over ``mask`` that ``model`` lies next to: undamped Gauss-Newton from it
    until the step no longer moves the model.  What the models of the fixed schedule are measured against on a noisy scene,
    where the planted similarity is not the optimum."""
    sc = dict(sc)
    if sc.get("sigma2") is None:
        sc["sigma2"] = np.ones((len(sc["X1"]), 2))
    model = np.asarray(model, np.float64).copy()
    for _ in range(steps):
        H, b, _ = linearize(model, sc, K, mask, 0.0, fix_scale)
        if fix_scale:
            H[6, 6] = 1.0
        x = np.linalg.solve(H, -b)
        model = retract(model, x)
        if np.abs(x).max() < 1e-15:
            break
    return model


# ---------------------------------------------------------------- scenes
def make_scene(rng, n, scale=1.0, pixel_noise=0.0, outlier_share=0.0, depth=(2.0, 20.0), offset=0.0, with_sigma=False, K=EUROC):
    """dict(X1, X2 [n,3], px1, px2 [n,2], sigma2 [n,2], model the planted similarity, true_inlier bool [n]).  ``offset``: the
    points live at that offset along every world axis and both cameras look at them from there, so the camera coordinates
    carry the rounding of a subtraction at that magnitude.  ``with_sigma``: squared sigmas drawn from {1, 1.44, 2.0736} and
    the noise of a keypoint scaled by its sigma."""
    s, R, t = base.random_similarity(rng, scale)
    o = np.full(3, float(offset))
    Pw = base.cloud(rng, max(n, 1), depth, K)[:n] + o
    X1 = Pw - o
    X2 = s * (Pw @ R.T) + (t - s * (R @ o))
    out = rng.random(n) < outlier_share if outlier_share else np.zeros(n, bool)
    ang, far = rng.uniform(0, 2 * np.pi, n), rng.uniform(20.0, 80.0, n)
    shift = np.stack([far * np.cos(ang) / K[0], far * np.sin(ang) / K[1], np.zeros(n)], 1) * X2[:, 2:]
    X2 = np.where(out[:, None], X2 + shift, X2)
    sigma2 = rng.choice([1.0, 1.44, 2.0736], (n, 2)) if with_sigma else np.ones((n, 2))
    px1 = project(X1, K) + pixel_noise * np.sqrt(sigma2[:, :1]) * rng.normal(size=(n, 2))
    px2 = project(X2, K) + pixel_noise * np.sqrt(sigma2[:, 1:]) * rng.normal(size=(n, 2))
    return dict(X1=np.ascontiguousarray(X1), X2=np.ascontiguousarray(X2), px1=px1, px2=px2, sigma2=sigma2, model=pack(s, R, t),
                true_inlier=~out, K=K)


def moved(rng, model, rot=0.005, trans=0.01, sigma=0.02):
    """The model moved by about ``rot`` rad, ``trans`` m and ``sigma`` in log scale (through this file's retraction)."""
    d = lambda size: rng.normal(size=3) / np.sqrt(3) * size
    return retract(model, np.concatenate([d(rot), d(trans), [sigma * rng.choice([-1.0, 1.0])]]))


def ransac_start(sc, K=EUROC, H=64):
    """The scene's own RANSAC + refit model (sim3_ref's numpy statements); the RANSAC mask too."""
    m, mask, st = base.ransac(sc["X1"], sc["X2"], K, H, base.CHI2, 0)
    if mask.sum() >= 3:
        m, _ = base.refit(sc["X1"], sc["X2"], mask)
    return m, mask


def scene_list():
    """name -> (scene, start model, kind); kind 'exact' (noise-free: converges to the planted similarity) or 'noisy'."""
    rng = np.random.default_rng(SEED)
    out = {}
    for scale in (0.5, 1.0, 2.0):
        for offset in (0.0, 1e4):
            sc = make_scene(rng, 200, scale, offset=offset)
            out[f"exact_s{scale:g}_o{offset:g}"] = (sc, moved(rng, sc["model"]), "exact")
    for scale in (0.5, 1.0, 2.0):
        for share in (0.0, 0.3):
            sc = make_scene(rng, 200, scale, 1.0, share, depth=(2.0, 20.0))
            out[f"noisy_s{scale:g}_out{int(share * 100)}"] = (sc, moved(rng, sc["model"]), "noisy")
    sc = make_scene(rng, 200, 1.3, 1.0, 0.3, with_sigma=True)
    out["noisy_sigma_out30"] = (sc, moved(rng, sc["model"]), "noisy")
    sc = make_scene(rng, 200, 1.2, 1.0, 0.3)
    out["ransac_out30"] = (sc, ransac_start(sc)[0], "noisy")
    sc = make_scene(rng, 200, 0.9, 1.0, 0.0)
    out["ransac_out0"] = (sc, ransac_start(sc)[0], "noisy")
    return out


def extreme_cases():
    """name -> (scene, start): finite data at the edges of f64 - squares that overflow, sigmas that make chi2 overflow or
    vanish, depths next to zero, a start far from the data.  Nothing here has a right answer; the contract is a finite
    model and, on the device, the twin's bits."""
    rng = np.random.default_rng(SEED + 9)
    out = {}

    def fresh():
        sc = make_scene(rng, 60, 1.1, 1.0, 0.2)
        return {k: sc[k].copy() for k in ("X1", "X2", "px1", "px2", "sigma2", "model")}

    sc = fresh(); sc["X1"][3] *= 1e200; sc["X2"][7] *= 1e160; sc["px1"][11] = [1e308, -1e308]
    out["huge_values"] = (sc, moved(rng, sc["model"]))
    sc = fresh(); sc["sigma2"][::5, 0] = 1e-300; sc["sigma2"][1::5, 1] = 1e300; sc["sigma2"][2, :] = 5e-324
    out["extreme_sigmas"] = (sc, moved(rng, sc["model"]))
    sc = fresh(); sc["X1"][4, 2] = 1e-300; sc["X2"][9, 2] = 5e-324; sc["X1"][20] *= 1e-160
    out["depths_next_to_zero"] = (sc, moved(rng, sc["model"]))
    sc = fresh(); start = moved(rng, sc["model"]); start[3] = 1e150; start[12] = 1e-150
    out["start_far_away"] = (sc, start)
    sc = fresh(); start = moved(rng, sc["model"], rot=1.0, trans=3.0, sigma=1.0)
    out["start_a_radian_off"] = (sc, start)
    sc = fresh(); sc["X2"][:] = sc["X2"][0]; sc["px2"][:] = sc["px2"][0]
    out["one_point_repeated"] = (sc, moved(rng, sc["model"]))
    return out


def model_errors(model, truth):
    """(|s / s_true - 1|, |R - R_true| Frobenius, |t - t_true| / (1 + |t_true|))."""
    q = base.model_quantities(np.asarray(model).reshape(1, 13), np.asarray(truth))
    return q["scale"], q["rotation"], q["translation"]
