"""Truth for the pose-graph kernels that shares none of their formulas, and the graphs the edge tests run on.  Nothing here
is imported by the product.

Three kinds of truth:

  mpmath     one edge at 80 digits from definitions only: Exp as the matrix exponential of the 4x4 twist, Jl(xi) as
             sum_n ad(xi)^n / (n+1)! inverted numerically, Ad(T) as the matrix of x -> (T x^ T^-1)^vee.  A case is built
             backwards: choose f64 xi, T_i, Z and Omega, form T_j = Exp(xi) Z T_i at 80 digits and round it to f64; then
             r = xi, J_j = Jl^-1(xi), J_i = -J_j Ad(T_j T_i^-1) = -J_j Ad(Exp(xi) Z) (the convention of include/slamhip.h,
             which tests/test_pose_graph_cpu.py pins by central differences), chi2 = xi^T Omega xi, W = J_i^T Omega J_j,
             the two diagonal shares J^T Omega J and the two gradient shares J^T Omega xi.  The rounding of T_j (and the
             1e-16 by which the f64 T_i and Z miss being rotations) is part of the problem every f64 implementation is
             handed; the yardsticks of tests/test_pose_graph_edges_cpu.py are the numpy reference's distance to this truth
             and so contain it.  tests/golden/make_pose_graph_truth.py writes the sweep to tests/golden/pose_graph_truth.npz.
  integers   graphs whose poses and measurements are pure translations with integer coordinates and whose information has
             integer entries: th = 0, ad(xi)^2 = 0, so Jl^-1 = I - ad(xi) / 2 exactly and every number of the linearisation
             is a multiple of 1/4 far below 2^53: any order of f64 additions gives the same bits.  Computed here in int64
             (times 4) and, for the small graphs, again in fractions.Fraction.
  longdouble the reference's PCG algorithm on blocks in any numpy float type, to measure what f64 leaves open after m steps.
"""
from __future__ import annotations

import math
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_ref as R  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_graph_truth.npz")
DIGITS = 80

# ---------------------------------------------------------------- the sweep ---------------------------------------------------
# the kernel switches th / sin(th) at sin(th) = 1e-4 and its coefficient series at 0.2 rad; its contract ends at 3.1 rad
ANGLES = (1e-12, 1e-9, 0.99e-4, 1.01e-4, 0.01, 0.1999999, 0.2000001, 0.5, 1.0, float(np.pi / 2), 2.0, 2.5, 3.0, 3.09, 3.0999)
BEYOND = (3.1001, 3.14)
TRANSLATIONS = (1e-3, 1.0, 1e3)
BAND_CUTS = (1e-3, 0.05, 0.2, 0.5, 2.5)
FAMILIES = ("iso", "spd1", "spd1e4", "spd1e8", "rot_only")
N_AXES = 3                     # per angle: two random axes and one coordinate axis (two components of the vector part vanish)


def band_of(angle):
    return int(np.searchsorted(BAND_CUTS, angle, side="right"))


def sweep_inputs():
    """the f64 inputs of the sweep: dict(xi [n,6], Ti [n,3,4], Z [n,3,4], beyond [n] bool, info_<family> [n,6,6])"""
    from slamhip import loop_edges_from_two_view

    rng = np.random.default_rng(20240607)
    xi, Ti, Z, beyond = [], [], [], []
    k = 0
    for a_idx, th in enumerate(ANGLES + BEYOND):
        for ax in range(N_AXES):
            for t_idx, tm in enumerate(TRANSLATIONS):
                if ax < 2:
                    axis = rng.normal(size=3)
                    axis /= np.linalg.norm(axis)
                else:
                    axis = np.zeros(3)
                    axis[(a_idx + t_idx) % 3] = 1.0 if (a_idx + t_idx) % 2 else -1.0
                v = rng.normal(size=3)
                v *= tm / np.linalg.norm(v)
                xi.append(np.concatenate([th * axis, v]))
                general = (ax + t_idx + a_idx) % 2 == 1             # T_i: the identity, or a pose with coordinates up to 1e3
                scale = (1.0, 30.0, 1e3)[k % 3]
                Ti.append(R.exp_se3(np.concatenate([rng.normal(0, 1.2, 3), rng.uniform(-scale, scale, 3)])) if general
                          else np.eye(4)[:3])
                Z.append(np.eye(4)[:3] if k % 4 == 0 else R.exp_se3(np.concatenate([rng.normal(0, 0.8, 3), rng.uniform(-5, 5, 3)])))
                beyond.append(th > 3.1)
                k += 1
    n = len(xi)
    out = dict(xi=np.array(xi), Ti=np.array(Ti), Z=np.array(Z), beyond=np.array(beyond))
    out["info_iso"] = np.array([np.diag([(1.0, 1e4, 2.5e3)[i % 3]] * 3 + [(1.0, 100.0, 4e2)[i % 3]] * 3) for i in range(n)])
    for name, cond in (("spd1", 1.0), ("spd1e4", 1e4), ("spd1e8", 1e8)):
        mats = []
        for _ in range(8):                                           # eight matrices per family, dealt round the edges
            Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
            M = (Q * np.geomspace(1.0, cond, 6)) @ Q.T
            mats.append(0.5 * (M + M.T))
        out["info_" + name] = np.array([mats[i % 8] for i in range(n)])
    # rotation-only information exactly as the product builds it for a two-view loop closure of unknown scale
    counts = 20 + (np.arange(n) * 37) % 400
    _, _, info = loop_edges_from_two_view(np.stack([np.arange(n), np.arange(n) + n], 1), np.tile(np.eye(3), (n, 1, 1)),
                                          np.tile([0.0, 0.6, 0.8], (n, 1)), counts, min_inliers=20, rotation_sigma=0.01)
    out["info_rot_only"] = info
    return out


# ---------------------------------------------------------------- mpmath ------------------------------------------------------
def _mp():
    import mpmath

    mpmath.mp.dps = DIGITS
    return mpmath.mp


def _hat4(mp, xi):
    w0, w1, w2, v0, v1, v2 = xi
    return mp.matrix([[0, -w2, w1, v0], [w2, 0, -w0, v1], [-w1, w0, 0, v2], [0, 0, 0, 0]])


def _ad6(mp, xi):
    M = mp.zeros(6, 6)
    W, P = _hat4(mp, xi)[:3, :3], _hat4(mp, list(xi[3:]) + [0, 0, 0])[:3, :3]
    for i in range(3):
        for j in range(3):
            M[i, j] = W[i, j]
            M[3 + i, 3 + j] = W[i, j]
            M[3 + i, j] = P[i, j]
    return M


def _series(mp, A, shift):
    """sum_n A^n / (n + shift)! (shift 0: exp, shift 1: the left Jacobian), summed until the terms fall below 10^-(DIGITS+10)"""
    n = A.rows
    term = mp.eye(n) / mp.factorial(shift)
    out = term.copy()
    k = 0
    while True:
        k += 1
        term = term * A / (k + shift)
        out += term
        if mp.norm(term, "inf") < mp.mpf(10) ** (-(DIGITS + 10)) and k > 8:
            return out


def _T4(mp, T):
    M = mp.eye(4)
    for i in range(3):
        for j in range(4):
            M[i, j] = mp.mpf(float(T[i][j]))
    return M


def _Ad(mp, T):
    """the matrix of x -> (T x^ T^-1)^vee in [w, v] order, column by column"""
    Tinv = mp.inverse(T)
    Ad = mp.zeros(6, 6)
    for k in range(6):
        e = [0] * 6
        e[k] = 1
        M = T * _hat4(mp, e) * Tinv
        col = [M[2, 1], M[0, 2], M[1, 0], M[0, 3], M[1, 3], M[2, 3]]
        for i in range(6):
            Ad[i, k] = col[i]
    return Ad


def _f(M):
    return np.array([[float(M[i, j]) for j in range(M.cols)] for i in range(M.rows)])


def mp_geometry(xi, Ti, Z):
    """(T_j rounded to f64 [3,4], J_j, J_i as mpmath matrices) of one case"""
    mp = _mp()
    x = [mp.mpf(float(c)) for c in xi]
    # the terms of exp's series grow to |A|^|A| / |A|! before they fall: 80 digits leave more than 60 at |v| = 1e3 only after
    # scaling, so halve 12 times and square back
    E = _series(mp, _hat4(mp, x) / 4096, 0)
    for _ in range(12):
        E = E * E
    A = E * _T4(mp, Z)
    Tj = _f(A * _T4(mp, Ti))[:3]
    Jj = mp.inverse(_series(mp, _ad6(mp, x), 1))
    return Tj, Jj, -Jj * _Ad(mp, A)


def mp_edge(xi, Jj, Ji, info, huber=0.0):
    """f64 roundings of the 80-digit chi2, W [6,6], H_i share, H_j share, b_i share, b_j share (all for weight 1), and of the
    Huber weight and rho at `huber`"""
    mp = _mp()
    x = mp.matrix([mp.mpf(float(c)) for c in xi])
    Om = mp.matrix([[mp.mpf(float(c)) for c in row] for row in info])
    Or = Om * x
    chi2 = (x.T * Or)[0]
    w, rho = mp.mpf(1), chi2
    if huber > 0:
        e, d = mp.sqrt(chi2), mp.mpf(float(huber))
        if e > d:
            w, rho = d / e, 2 * d * e - d * d
    return (float(chi2), _f(Ji.T * Om * Jj), _f(Ji.T * Om * Ji), _f(Jj.T * Om * Jj), _f(Ji.T * Or)[:, 0], _f(Jj.T * Or)[:, 0],
            float(w), float(rho))


def build_fixture(indices=None):
    """the fixture's arrays (all samples, or the samples `indices`); Huber deltas: per family the median of sqrt(chi2) over the
    in-contract samples, rounded to three digits, so some samples exceed it and some do not"""
    inp = sweep_inputs()
    n = len(inp["xi"])
    idx = np.arange(n) if indices is None else np.asarray(indices)
    out = {k: v[idx] for k, v in inp.items()}
    Tj = np.zeros((len(idx), 3, 4))
    geo = []
    for q, s in enumerate(idx):
        Tj[q], Jj, Ji = mp_geometry(inp["xi"][s], inp["Ti"][s], inp["Z"][s])
        geo.append((Jj, Ji))
    out["Tj"] = Tj
    ok = ~inp["beyond"]
    for fam in FAMILIES:
        info = inp["info_" + fam]
        chi = np.einsum("ea,eab,eb->e", inp["xi"], info, inp["xi"])[ok]          # only to place the delta: f64 is enough
        delta = float(f"{np.sqrt(np.median(chi)):.3g}")
        cols = [[] for _ in range(8)]
        for q, s in enumerate(idx):
            res = mp_edge(inp["xi"][s], geo[q][0], geo[q][1], info[s], delta)
            for c, v in zip(cols, res):
                c.append(v)
        iu = np.triu_indices(6)
        out["delta_" + fam] = np.array(delta)
        out["chi2_" + fam] = np.array(cols[0])
        out["W_" + fam] = np.array(cols[1])
        out["Hi_" + fam] = np.array(cols[2])[:, iu[0], iu[1]]            # upper triangles: the blocks are symmetric
        out["Hj_" + fam] = np.array(cols[3])[:, iu[0], iu[1]]
        out["gi_" + fam] = np.array(cols[4])
        out["gj_" + fam] = np.array(cols[5])
        out["w_" + fam] = np.array(cols[6])
        out["rho_" + fam] = np.array(cols[7])
    return out


def load_fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def sym_from_upper(u):
    iu = np.triu_indices(6)
    M = np.zeros(u.shape[:-1] + (6, 6))
    M[..., iu[0], iu[1]] = u
    M[..., iu[1], iu[0]] = u
    return M


def truth_graph(fx, family, huber, select=None):
    """The graph of disjoint edges (vertices 2e and 2e+1) over the fixture samples `select` (default: the in-contract ones) and
    its truth: dict(poses, edges, meas, info, huber, angle [E], cost, rho [E], grad [V,6], Hdiag [V,6,6], W [E,6,6]).  With
    Huber on, the 80-digit weight (rounded to f64) multiplies the f64 truths: one more rounding of 1.1e-16."""
    sel = np.flatnonzero(~fx["beyond"]) if select is None else np.asarray(select)
    E = len(sel)
    poses = np.empty((2 * E, 3, 4))
    poses[0::2], poses[1::2] = fx["Ti"][sel], fx["Tj"][sel]
    w = fx["w_" + family][sel] if huber else np.ones(E)
    rho = fx["rho_" + family][sel] if huber else fx["chi2_" + family][sel]
    dead = fx["beyond"][sel]
    w, rho = np.where(dead, 0.0, w), np.where(dead, 0.0, rho)
    grad, Hd = np.empty((2 * E, 6)), np.empty((2 * E, 6, 6))
    grad[0::2], grad[1::2] = w[:, None] * fx["gi_" + family][sel], w[:, None] * fx["gj_" + family][sel]
    Hd[0::2] = w[:, None, None] * sym_from_upper(fx["Hi_" + family][sel])
    Hd[1::2] = w[:, None, None] * sym_from_upper(fx["Hj_" + family][sel])
    return dict(poses=poses, edges=np.stack([2 * np.arange(E), 2 * np.arange(E) + 1], 1).astype(np.int32), meas=fx["Z"][sel],
                info=fx["info_" + family][sel], huber=float(fx["delta_" + family]) if huber else 0.0,
                angle=np.linalg.norm(fx["xi"][sel, :3], axis=1), dead=dead, cost=math.fsum(rho), rho=rho, grad=grad, Hdiag=Hd,
                W=w[:, None, None] * fx["W_" + family][sel])


def edge_errors(g, b, Hd, W):
    """per edge: the error of the gradient shares, diagonal shares and W, each relative to that edge's own largest magnitude of
    the quantity in the truth (dead edges, whose truth is zero: the absolute value)"""
    E = len(g["edges"])
    out = {}
    for key, got, ref in (("grad", b.reshape(E, -1), g["grad"].reshape(E, -1)), ("Hdiag", Hd.reshape(E, -1), g["Hdiag"].reshape(E, -1)),
                          ("W", W.reshape(E, -1), g["W"].reshape(E, -1))):
        scale = np.abs(ref).max(1)
        out[key] = np.abs(got - ref).max(1) / np.where(scale > 0, scale, 1.0)
    return out


def band_max(angle, err, keep=None):
    """largest error per angle band (NaN counts as infinite)"""
    out = np.zeros(len(BAND_CUTS) + 1)
    for e in range(len(angle)):
        if keep is None or keep[e]:
            b = band_of(angle[e])
            out[b] = max(out[b], err[e] if err[e] == err[e] else np.inf)
    return out


# ---------------------------------------------------------------- exact integer graphs -----------------------------------------
class ExactGraph:
    """pure integer translations, integer information; fixed masks to run products and solves under"""

    def __init__(self, name, V, edges, seed, masks=()):
        rng = np.random.default_rng(seed)
        self.name, self.V = name, int(V)
        self.edges = np.ascontiguousarray(np.asarray(edges, np.int32).reshape(-1, 2))
        self.E = len(self.edges)
        self.t = rng.integers(-8, 9, (self.V, 3))
        self.tz = rng.integers(-8, 9, (self.E, 3))
        B = rng.integers(-1, 2, (self.E, 6, 2))
        self.info_int = B @ np.swapaxes(B, 1, 2) + rng.integers(1, 5, (self.E, 1, 1)) * np.eye(6, dtype=np.int64)
        self.poses = np.tile(np.eye(4)[:3], (self.V, 1, 1))
        self.poses[:, :, 3] = self.t
        self.meas = np.tile(np.eye(4)[:3], (self.E, 1, 1))
        self.meas[:, :, 3] = self.tz
        self.info = self.info_int.astype(np.float64)
        first = np.zeros(self.V, np.uint8)
        first[0] = 1
        self.masks = [first] + [np.ascontiguousarray(m, np.uint8) for m in masks]
        self.seed = seed

    # -- linearisation -----------------------------------------------------------------------------------------------------------
    def _jacobians2(self):
        """2 J_j and 2 J_i as integers: J_j = I - ad(r) / 2 with r = [0, d], J_i = -J_j Ad([I | t_j - t_i])"""
        i, j = self.edges[:, 0], self.edges[:, 1]
        d = self.t[j] - self.t[i] - self.tz
        a = self.t[j] - self.t[i]
        E = self.E
        Jj2 = np.tile(2 * np.eye(6, dtype=np.int64), (E, 1, 1))
        Jj2[:, 3:, :3] = -_hat_int(d)
        Ad = np.tile(np.eye(6, dtype=np.int64), (E, 1, 1))
        Ad[:, 3:, :3] = _hat_int(a)
        return d, Jj2, -(Jj2 @ Ad)

    def linearize_int(self):
        """(cost, b [V,6], Hd [V,6,6], W [E,6,6]) as f64, from int64 arithmetic on 4x the values"""
        d, Jj2, Ji2 = self._jacobians2()
        r = np.concatenate([np.zeros_like(d), d], 1)
        Om = self.info_int
        Or = np.einsum("eab,eb->ea", Om, r)
        cost = int(np.einsum("ea,ea->", r, Or))
        JiT, JjT = np.swapaxes(Ji2, 1, 2), np.swapaxes(Jj2, 1, 2)
        Hd4 = np.zeros((self.V, 6, 6), np.int64)
        b2 = np.zeros((self.V, 6), np.int64)
        np.add.at(Hd4, self.edges[:, 0], JiT @ Om @ Ji2)
        np.add.at(Hd4, self.edges[:, 1], JjT @ Om @ Jj2)
        np.add.at(b2, self.edges[:, 0], np.einsum("eba,eb->ea", Ji2, Or))
        np.add.at(b2, self.edges[:, 1], np.einsum("eba,eb->ea", Jj2, Or))
        W4 = JiT @ Om @ Jj2
        assert max(np.abs(Hd4).max(initial=0), np.abs(W4).max(initial=0), abs(cost)) < 2 ** 50
        return float(cost), b2 / 2.0, Hd4 / 4.0, W4 / 4.0

    def linearize_fraction(self):
        """the same from fractions.Fraction, edge by edge (small graphs)"""
        half = Fraction(1, 2)
        Hd = [[[Fraction(0)] * 6 for _ in range(6)] for _ in range(self.V)]
        b = [[Fraction(0)] * 6 for _ in range(self.V)]
        W, cost = [], Fraction(0)
        for e, (i, j) in enumerate(self.edges.tolist()):
            d = [int(self.t[j][c] - self.t[i][c] - self.tz[e][c]) for c in range(3)]
            a = [int(self.t[j][c] - self.t[i][c]) for c in range(3)]
            r = [Fraction(0)] * 3 + [Fraction(c) for c in d]
            ad_r = _ad_frac(r)
            Jj = [[Fraction(int(p == q)) - half * ad_r[p][q] for q in range(6)] for p in range(6)]
            Ad = [[Fraction(int(p == q)) for q in range(6)] for p in range(6)]
            hat_a = _ad_frac([0, 0, 0] + a)
            for p in range(3):
                for q in range(3):
                    Ad[3 + p][q] = hat_a[3 + p][q]
            Ji = [[-sum(Jj[p][k] * Ad[k][q] for k in range(6)) for q in range(6)] for p in range(6)]
            Om = [[Fraction(int(c)) for c in row] for row in self.info_int[e]]
            Or = [sum(Om[p][q] * r[q] for q in range(6)) for p in range(6)]
            cost += sum(r[p] * Or[p] for p in range(6))
            W.append(_quad_frac(Ji, Om, Jj))
            for v, J in ((i, Ji), (j, Jj)):
                H = _quad_frac(J, Om, J)
                for p in range(6):
                    b[v][p] += sum(J[k][p] * Or[k] for k in range(6))
                    for q in range(6):
                        Hd[v][p][q] += H[p][q]
        return float(cost), _to_f64(b, (self.V, 6)), _to_f64(Hd, (self.V, 6, 6)), _to_f64(W, (self.E, 6, 6))

    # -- product -----------------------------------------------------------------------------------------------------------------
    def product_inputs(self):
        """integer Hd [V,6,6], W [E,6,6], x [V,6] in [-8, 8] and lam (as f64 arrays, and lam as a float)"""
        rng = np.random.default_rng(self.seed + 1)
        return (rng.integers(-8, 9, (self.V, 6, 6)).astype(np.float64), rng.integers(-8, 9, (self.E, 6, 6)).astype(np.float64),
                rng.integers(-8, 9, (self.V, 6)).astype(np.float64), float(rng.integers(-8, 9)))

    def hmul_int(self, fixed, Hd, W, lam, x):
        Hd, W, x, lam = (np.asarray(a).astype(np.int64) for a in (Hd, W, x, lam))
        free = np.asarray(fixed) == 0
        xf = np.where(free[:, None], x, 0)
        y = np.einsum("vab,vb->va", Hd, xf) + lam * xf
        i, j = self.edges[:, 0], self.edges[:, 1]
        np.add.at(y, i, np.einsum("eab,eb->ea", W, xf[j]))
        np.add.at(y, j, np.einsum("eba,eb->ea", W, xf[i]))
        return np.where(free[:, None], y, 0).astype(np.float64)


def _hat_int(w):
    W = np.zeros(w.shape[:-1] + (3, 3), np.int64)
    W[..., 0, 1], W[..., 0, 2] = -w[..., 2], w[..., 1]
    W[..., 1, 0], W[..., 1, 2] = w[..., 2], -w[..., 0]
    W[..., 2, 0], W[..., 2, 1] = -w[..., 1], w[..., 0]
    return W


def _ad_frac(xi):
    def hat(w):
        return [[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]
    M = [[Fraction(0)] * 6 for _ in range(6)]
    W, P = hat(xi[:3]), hat(xi[3:])
    for p in range(3):
        for q in range(3):
            M[p][q] = M[3 + p][3 + q] = Fraction(W[p][q])
            M[3 + p][q] = Fraction(P[p][q])
    return M


def _quad_frac(A, Om, B):
    """A^T Om B"""
    return [[sum(A[k][p] * Om[k][l] * B[l][q] for k in range(6) for l in range(6)) for q in range(6)] for p in range(6)]


def _to_f64(A, shape):
    return np.array([float(x) for x in _flat(A)]).reshape(shape)


def _flat(A):
    if isinstance(A, list):
        for x in A:
            yield from _flat(x)
    else:
        yield A


def _chain_plus(V, extra, rng):
    k = np.arange(V)
    chain = np.stack([k[:-1], k[1:]], 1) if V > 1 else np.zeros((0, 2), np.int64)
    if V < 3 or extra == 0:
        return chain
    a = rng.integers(0, V, extra)
    b = (a + rng.integers(1, V, extra)) % V
    return np.concatenate([chain, np.stack([a, b], 1)])


def _degrees_graph(degrees, pool):
    """vertex q gets exactly degrees[q] edges to the first degrees[q] of `pool` leaf vertices (alternating direction)"""
    n = len(degrees)
    edges = [(q, n + l) if (q + l) % 2 else (n + l, q) for q, d in enumerate(degrees) for l in range(d)]
    return n + pool, np.array(edges, np.int64).reshape(-1, 2)


def _uneven_masks(V, rng):
    v = np.arange(V)
    return [np.isin(v % 10, (0, 1, 2, 5)), (v % 40) >= 33, rng.random(V) < 0.3, np.ones(V, bool)]


def exact_graphs(big=True):
    """the graphs that straddle the launch boundaries of pose_graph.hip (the comments name the boundary)"""
    rng = np.random.default_rng(99)
    out = []
    # 10 vertices per wave, 40 per block, the 512-block cap of the vector kernels (grid stride from V = 20 481)
    for V in (1, 2, 9, 10, 11, 39, 40, 41) + ((20480, 20481, 20521) if big else ()):
        out.append(ExactGraph(f"V{V}", V, _chain_plus(V, V // 2, rng), 100 + V, _uneven_masks(V, rng)))
    # every degree 0..13: the four-slot unroll remainder of the product and of the gather, and a degree-0 vertex
    V, e = _degrees_graph(list(range(14)), 13)
    out.append(ExactGraph("deg0_13", V, e, 201, _uneven_masks(V, rng)))
    # PG_HUB_DEG = 128 from both sides, and the ten-group stride remainder of the hub path
    hubs = [127, 128, 129, 130, 137, 138, 139, 140]
    V, e = _degrees_graph(hubs, 140)
    m = _uneven_masks(V, rng)
    fixed_hubs = np.zeros(V, bool)
    fixed_hubs[[2, 5]] = True                                        # fixed hubs
    leaves_fixed = np.arange(V) >= len(hubs)                         # hubs all of whose neighbours are fixed
    out.append(ExactGraph("hub_degrees", V, e, 202, m + [fixed_hubs, leaves_fixed]))
    # 64 edges per edge block; 8 vertices per gather block
    for E in (63, 64, 65):
        out.append(ExactGraph(f"E{E}", 30, _chain_plus(30, E - 29, rng), 300 + E, _uneven_masks(30, rng)))
    for V in (7, 8):
        out.append(ExactGraph(f"V{V}", V, _chain_plus(V, 5, rng), 100 + V, _uneven_masks(V, rng)))
    # duplicate edges and both orientations of one pair
    e = np.array([[0, 1], [0, 1], [1, 0], [1, 2], [2, 1], [2, 3], [2, 3], [2, 3], [3, 0], [0, 3]])
    out.append(ExactGraph("duplicates", 5, e, 203, _uneven_masks(5, rng)))             # vertex 4 has no edge
    if big:
        # the one-block hub scan with more than 256 count blocks, hubs in the first and last blocks, more hubs than hub waves
        V = 70000
        hub_v = sorted(set([0, 255, 256, 65535, 65536, 69999] + list(range(500, 65000, 1000))))
        assert len(hub_v) > 64
        k = np.arange(V)
        parts = [np.stack([k[:-1], k[1:]], 1)]
        for q, h in enumerate(hub_v):
            others = (h + 7 + 523 * np.arange(1, 128 + 1 + q % 12)) % V
            others = others[others != h]
            parts.append(np.stack([np.full(len(others), h), others], 1)[:, ::1 if q % 2 else -1])
        e = np.concatenate(parts)
        fm = np.zeros(V, bool)
        fm[[0, 256, 65536]] = True
        out.append(ExactGraph("V70000_hubs", V, e, 204, [fm, np.isin(k % 10, (0, 1, 2, 5))]))
    return out


# ---------------------------------------------------------------- PCG on blocks in any float type --------------------------------
def pcg_blocks(edges, fixed, Hd, W, b, lam, tol, max_iter, dtype=np.float64, keep=()):
    """pose_graph_ref.pcg on the blocks themselves in `dtype`: (x [V,6], iterations, relres of the recurrence,
    {m: (x after m iterations, relres after m)} for m in keep)"""
    f = dtype
    free = (np.asarray(fixed) == 0)[:, None]
    Hd = np.asarray(Hd, f) + f(lam) * np.eye(6, dtype=f)
    W, i, j = np.asarray(W, f), edges[:, 0], edges[:, 1]
    Minv = np.linalg.inv(np.asarray(Hd, np.float64)).astype(f)
    if f is not np.float64:                                            # two Newton steps X <- X (2 I - A X): exact to the wider type,
        for _ in range(2):                                             # so the f64 run's inverse is part of what is measured
            Minv = Minv @ (2 * np.eye(6, dtype=f) - Hd @ Minv)

    def A(p):
        p = np.where(free, p, f(0))
        y = np.einsum("vab,vb->va", Hd, p)
        np.add.at(y, i, np.einsum("eab,eb->ea", W, p[j]))
        np.add.at(y, j, np.einsum("eba,eb->ea", W, p[i]))
        return np.where(free, y, f(0))

    r = np.where(free, -np.asarray(b, f).reshape(-1, 6), f(0))
    x = np.zeros_like(r)
    bb = (r * r).sum()
    snaps = {}
    if bb == 0:
        return x, 0, 0.0, snaps
    z = np.einsum("vab,vb->va", Minv, r)
    p = z.copy()
    rz, rr, it = (r * z).sum(), bb, 0
    tol2 = f(tol) * f(tol) * bb
    while it < max_iter and rr > tol2:
        q = A(p)
        alpha = rz / (p * q).sum()
        x = x + alpha * p
        r = r - alpha * q
        z = np.einsum("vab,vb->va", Minv, r)
        rz_new = (r * z).sum()
        rr = (r * r).sum()
        p = z + (rz_new / rz) * p
        rz = rz_new
        it += 1
        if it in keep:
            snaps[it] = (x.copy(), float(np.sqrt(rr / bb)))
    return x, it, float(np.sqrt(rr / bb)), snaps
