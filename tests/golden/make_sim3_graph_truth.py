"""Maker of tests/golden/sim3_graph_truth.npz: one edge's Sim(3) linearisation from definitions, in mpmath at 80 digits.

A case is built backwards, as tests/pose_graph_truth.py builds its own: choose f64 r, S_i, Z and Omega, form
S_j = Phi(r) o Z o S_i at 80 digits (Phi through the matrix exponential of the 4x4 twist, the group products in exact
arithmetic) and round it to f64.  Then the residual is r - Phi^-1 is never evaluated, which matters because mpmath.logm loses
the principal branch beyond about 3 rad - and the Jacobians follow from the definition r(d) = Phi^-1(Phi(d) o ...) by the
inverse function theorem: Phi(r + J d) = [the perturbed D] to first order, so J = DPhi(r)^+ D_d[perturbed D], both
differentials by mpmath.diff of the 13 numbers of the similarity.  The rounding of S_j is part of the problem every f64
implementation is handed; the yardsticks of tests/test_sim3_graph_cpu.py are the numpy reference's distance to this truth and
so contain it.  Cost, weight and blocks in 80 digits, rounded to f64 once at the end.
Run from tests/: python golden/make_sim3_graph_truth.py (about two minutes)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import sim3_graph_ref as R  # noqa: E402

DIGITS = 80
SEED = 4107
ANGLES = (1e-10, 1e-7, 5e-5, 0.9e-4, 1.1e-4, 9e-4, 2e-3, 0.04, 0.19, 0.21, 0.45, 1.5, 2.6, 3.09)   # both sides of 1e-4 and 0.2
TRANSLATIONS = (1e-3, 1.0, 1e3)
LOG_SCALES = (0.0, -3.0, 3.0, -0.7, 0.3)       # s_D; 0.0 is s_D = 1 EXACTLY (power-of-two scales around it)
N_AXES = 2
FAMILIES = ("diag", "spd1", "spd1e4", "spd1e8", "rot_scale_only")
FIXTURE = os.path.join(HERE, "sim3_graph_truth.npz")


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def sweep_inputs():
    """the f64 inputs, a function of SEED alone: r [N,7], Si, Z [N,13], info_<family> [N,7,7] (S_j is made at 80 digits)"""
    rng = np.random.default_rng(SEED)
    rt, Si, Z = [], [], []
    k = 0
    for th in ANGLES:
        for tm in TRANSLATIONS:
            for ax in range(N_AXES):
                axis = np.eye(3)[k % 3] if ax == 0 else _unit(rng)
                ls = LOG_SCALES[k % len(LOG_SCALES)]
                rt.append(np.concatenate([th * axis, tm * _unit(rng), [ls]]))
                if ls == 0.0 or k % 4 == 0:          # power-of-two scales, identity rotation: exact products
                    Si.append(R.pack(2.0 ** rng.integers(-1, 3), np.concatenate([np.eye(3), rng.integers(-3, 4, (3, 1)).astype(float)], 1)))
                    Z.append(R.pack(2.0 ** rng.integers(-1, 3), np.concatenate([np.eye(3), rng.integers(-3, 4, (3, 1)).astype(float)], 1)))
                else:
                    Si.append(R.phi(np.concatenate([rng.uniform(0, 3) * _unit(rng), rng.normal(0, 200, 3), [rng.normal(0, 0.5)]])))
                    Z.append(R.phi(np.concatenate([rng.uniform(0, 3) * _unit(rng), rng.normal(0, 5, 3), [rng.normal(0, 0.5)]])))
                k += 1
    rt, Si, Z = np.array(rt), np.array(Si), np.array(Z)
    N = len(rt)
    out = dict(r=rt, Si=Si, Z=Z)
    sig = np.array([0.01] * 3 + [0.1] * 3 + [0.05])
    out["info_diag"] = np.tile(np.diag(1 / sig ** 2), (N, 1, 1))
    for fam, cond in (("spd1", 1.0), ("spd1e4", 1e4), ("spd1e8", 1e8)):
        M = np.empty((N, 7, 7))
        for n in range(N):
            Q, _ = np.linalg.qr(rng.normal(size=(7, 7)))
            C = Q @ np.diag(np.logspace(0, np.log10(cond), 7)) @ Q.T if cond > 1 else 3.0 * np.eye(7)
            M[n] = 0.5 * (C + C.T)
        out["info_" + fam] = M
    ro = out["info_diag"].copy()
    ro[:, 3:6, 3:6] = 0.0
    out["info_rot_scale_only"] = ro
    return out


# ---------------------------------------------------------------- mpmath -----------------------------------------------------
def _mp():
    """mpmath at DIGITS; the precision is set on first use only: mpmath.diff raises it while it evaluates"""
    import mpmath

    if not getattr(_mp, "ready", False):
        mpmath.mp.dps = DIGITS
        _mp.ready = True
    return mpmath


def mp_sim(S):
    mp = _mp()
    S = [mp.mpf(float(x)) for x in S]
    return S[12], mp.matrix(3, 3) + mp.matrix([[S[0], S[1], S[2]], [S[4], S[5], S[6]], [S[8], S[9], S[10]]]), mp.matrix([S[3], S[7], S[11]])


def mp_mul(A, B):
    return A[0] * B[0], A[1] * B[1], A[0] * (A[1] * B[2]) + A[2]


def mp_inv(A):
    return 1 / A[0], A[1].T, -(A[1].T * A[2]) / A[0]


def mp_hat(w):
    mp = _mp()
    return mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def mp_expm4(X):
    """the matrix exponential of a 4x4 twist by its series after halving 12 times, squared back (terms to the working precision)"""
    mp = _mp()
    A = X / 4096
    term, out, k = mp.eye(4), mp.eye(4), 0
    while True:
        k += 1
        term = term * A / k
        out += term
        if k > 8 and mp.mnorm(term, 1) < mp.eps * mp.mpf(10) ** -10:
            break
    for _ in range(12):
        out = out * out
    return out


def mp_phi(d):
    """(e^sigma, Exp(w), V(w) v) through the matrix exponential of the 4x4 twist"""
    mp = _mp()
    X = mp.zeros(4)
    W = mp_hat(d[:3])
    for i in range(3):
        for j in range(3):
            X[i, j] = W[i, j]
        X[i, 3] = d[3 + i]
    M = mp_expm4(X)
    return mp.exp(d[6]), M[:3, :3], M[:3, 3]


def _vec(S):
    return [S[1][i, j] for i in range(3) for j in range(3)] + [S[2][i] for i in range(3)] + [S[0]]


def _differential(fun):
    """13 x 7 matrix of d vec(fun(d)) / d d at 0 by mpmath.diff (the evaluations are shared between the 13 components)"""
    mp = _mp()
    out = mp.zeros(13, 7)
    for c in range(7):
        cache = {}

        def f(x, c=c, cache=cache):
            key = (mp.mp.prec, mp.nstr(x, 40))
            if key not in cache:
                d = [mp.mpf(0)] * 7
                d[c] = x
                cache[key] = _vec(fun(d))
            return cache[key]

        for a in range(13):
            out[a, c] = mp.diff(lambda x, a=a: f(x)[a], 0)
    return out


def mp_case(r, Si, Z):
    """(S_j rounded to f64 [13], J_i, J_j as 7x7 mpmath matrices) of one case"""
    mp = _mp()
    rv = [mp.mpf(float(x)) for x in r]
    Si, Zm = mp_sim(Si), mp_sim(Z)
    D = mp_phi(rv)
    A = mp_mul(D, Zm)
    Sj = mp_mul(A, Si)
    Sj64 = np.array([float(Sj[1][i, j]) if j < 3 else float(Sj[2][i]) for i in range(3) for j in range(4)] + [float(Sj[0])])
    Ainv = mp_inv(A)
    M1 = _differential(lambda d: mp_phi([rv[k] + d[k] for k in range(7)]))
    Mj = _differential(lambda d: mp_mul(mp_phi(d), D))                                   # S_j' S_i^-1 Z^-1 = Phi(d) o D
    Mi = _differential(lambda d: mp_mul(mp_mul(mp_mul(A, mp_inv(mp_phi(d))), Ainv), D))    # S_j (Phi(d) S_i)^-1 Z^-1
    G = mp.inverse(M1.T * M1) * M1.T
    return Sj64, G * Mi, G * Mj


def mp_edge(r, Ji, Jj, Om, delta):
    """f64 (cost, w, W, Hii, Hjj, bi, bj) of one edge at 80 digits"""
    mp = _mp()
    O = mp.matrix(7, 7)
    for a in range(7):
        for b in range(7):
            O[a, b] = mp.mpf(float(Om[a, b]))
    rv = mp.matrix([mp.mpf(float(x)) for x in r])
    chi2 = (rv.T * O * rv)[0]
    w, rho = mp.mpf(1), chi2
    if delta > 0:
        en = mp.sqrt(chi2)
        if en > delta:
            w, rho = mp.mpf(float(delta)) / en, 2 * mp.mpf(float(delta)) * en - mp.mpf(float(delta)) ** 2
    f = lambda M: np.array([[float(M[i, j]) for j in range(M.cols)] for i in range(M.rows)])
    Or = O * rv
    return (float(rho), float(w), f(w * (Ji.T * O * Jj)), f(w * (Ji.T * O * Ji)), f(w * (Jj.T * O * Jj)), f(w * (Ji.T * Or))[:, 0],
            f(w * (Jj.T * Or))[:, 0])


def build_fixture(idx=None):
    inp = sweep_inputs()
    N = len(inp["r"])
    idx = np.arange(N) if idx is None else np.asarray(idx)
    out = {k: v[idx] for k, v in inp.items()}
    geo = [mp_case(inp["r"][n], inp["Si"][n], inp["Z"][n]) for n in idx]
    out["Sj"] = np.array([g[0] for g in geo])
    for fam in FAMILIES:
        Om = inp["info_" + fam]
        # the Huber delta of a family: the median of sqrt(chi2) over the WHOLE sweep (a function of the inputs alone)
        delta = float(np.median(np.sqrt(np.einsum("ea,eab,eb->e", inp["r"], Om, inp["r"]))))
        out["delta_" + fam] = np.float64(delta)
        for hub, d in (("", 0.0), ("_huber", delta)):
            res = [mp_edge(inp["r"][n], g[1], g[2], Om[n], d) for g, n in zip(geo, idx)]
            for q, name in enumerate(("cost", "w", "W", "Hii", "Hjj", "bi", "bj")):
                out[f"{name}_{fam}{hub}"] = np.array([x[q] for x in res])
    return out


def load_fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


if __name__ == "__main__":
    fx = build_fixture()
    np.savez_compressed(FIXTURE, **fx)
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes,", len(fx["r"]), "edges")
