"""Exact reference for the f64 geometry kernels (residual, Jacobians, Huber weights, normal equations, Schur reduction).

Plain helper module shared by tests/test_exact_geometry_cpu.py and tests/test_exact_geometry_gpu.py.  The arithmetic uses
the standard library only: every input double is converted to ``fractions.Fraction`` exactly, and everything after that is
exact rational arithmetic, except square roots, which are taken with ``decimal`` at 80 significant digits.  No float
arithmetic happens before the final comparison.  numpy is used only to generate the inputs and to hold kernel outputs.

What is computed from definitions, not copied from a kernel:

* residual      p = R X + t;  e = m - (K p)[:2] / (K p)[2], written (fx X + cx Z) / Z as frontend.py:275-277 does;
* pose Jacobian d e(exp(d) T) / d d at d = 0, d = (w, v) rotation first: forward-mode dual numbers along the tangent
                directions p -> e_i x p (rotation) and p -> e_i (translation);
* point Jacobian d e / d X with the same dual numbers, along the columns of R;
* Huber         w = 1 if c2 <= delta^2 else delta / sqrt(c2);  rho = c2 or 2 delta sqrt(c2) - delta^2 (g2o RobustKernelHuber);
* normal equations of one pose, and the Schur reduction of a window in the conventions of ``oracle.ba_schur_np`` /
  ``ba_backsub_np`` (E = (Hll + lambda I)^-1, the identity for a point nobody observes).

The one exception is the ``tiny_z`` case (|Z| <= 1e-6): there the reference's convention Zinv = 1 / (Z + 1e-18)
(frontend.py:286) changes the Jacobian by more than rounding, so its Jacobian reference is the literal frontend.py:286-291
expression evaluated exactly with Fraction(1e-18).  The CPU suite checks that this expression, with the 1e-18 dropped, is
exactly the dual-number derivative on every case.

Error bound.  Every value is a ``B``: its exact value ``v`` and a magnitude ``m`` >= |v|, propagated to first order
(a + b -> m_a + m_b, a b -> m_a |b| + |a| m_b, a / b -> m_a / |b| + |a / b| m_b / |b|, sqrt a -> sqrt a + m_a / (2 sqrt a);
an input double has m = |v|).  By induction an f64 evaluation with a chain of n roundings is within n 2^-53 m of the exact
value, whatever the order of its sums.  The bound of p is 2 |R||X| + |t|, not |p|; the bound of H is the sum of about
4 |w| |J_a| |J_b| over the observations, and so on.  Products take the exact value of the other factor, not its magnitude:
evaluating products on magnitudes (m_a m_b) multiplies the cancellation of e = m - proj (|e| << m_e) through c2, the Huber
weight, Hll and the 3x3 cofactors into bounds far larger than the values, which no wrong result could exceed.  Magnitudes are rounded UP to 64-bit mantissas to keep them small; values
are rounded only where a square root or a division by a sum enters (the Huber weight, the 3x3 inverse) and where
per-observation values enter a sum over observations: to 256-bit mantissas (77 digits), which keeps the rationals small.
Every compared value is still correct to well over 30 significant digits.

Tolerance rule: a kernel or oracle value g passes when |g - exact| <= C 2^-53 m.  An element whose bound is 0 (a structural
zero such as Jp[0,4], or a product with an exact zero) must therefore be exactly the exact value.
"""
from __future__ import annotations

from dataclasses import dataclass
from decimal import Decimal, localcontext
from fractions import Fraction
from functools import lru_cache

import numpy as np

# C: the longest chain of dependent roundings in any of the kernels measured here, as a power of two.  The longest is a
# Schur-complement entry of slam_ba_reduce_f64: the projection (3 roundings), Zinv and Zinv^2 (3), a Jacobian entry (3),
# the Huber weight (3: c2, sqrt, divide), the Hpl / Hll products (3), the Hll sum and the 3x3 cofactor inverse (5), Y = Hpl E
# (3), Y Hpl^T (3), the wave/block reduction tree of the pose-pair kernel (6 + 2 + a short per-thread sum) and the host's
# Hpp + lambda I - W (2): about 40, so C = 64.  The f64 normal equations (a 256-lane tree over at most 128 block partials)
# and the per-observation values (at most ~15) are shorter.  The 1e-18 of Zinv = 1 / (Z + 1e-18) moves the Jacobian by
# 2e-18 / |Z| relative: on the cases that use the dual-number derivative the smallest |Z| is near's, a little above 5e-4,
# which makes at most 4e-15, 36 units of 2^-53; with near's own chain (~15 roundings) that still fits.  Not to be raised to make a case pass: a case that fails at this C is a finding.
C = 64
U = Fraction(1, 2 ** 53)
EPS_Z = Fraction(1e-18)           # frontend.py:286, as the double the kernels add

CASES = ("benign", "wide", "far", "near", "cancel", "rotations", "behind", "tiny_z", "huber_edge")
LM_CASES = ("wide", "far", "near", "cancel")
EUROC = (458.654, 457.296, 367.215, 248.375)       # config/orb.yaml:1


# ---------------------------------------------------------------------------------------------------------------------
# exact arithmetic with a forward-error magnitude
# ---------------------------------------------------------------------------------------------------------------------
def _up(x: Fraction) -> Fraction:
    """x >= 0 rounded up to a 64-bit mantissa (an upper bound that stays cheap to carry)."""
    n, d = x.numerator, x.denominator
    if n == 0 or (n.bit_length() <= 64 and d.bit_length() <= 64):
        return x
    s = n.bit_length() - d.bit_length() - 64
    q = -(-n // (d << s)) if s >= 0 else -(-(n << -s) // d)
    return Fraction(q << s) if s >= 0 else Fraction(q, 1 << -s)


PREC_BITS = 256    # 77 significant digits


def rnd(x: Fraction) -> Fraction:
    """x rounded to the nearest PREC_BITS-bit mantissa (a dyadic rational: sums of these stay small)."""
    n, d = abs(x.numerator), x.denominator
    if n == 0 or (d & (d - 1) == 0 and n.bit_length() <= PREC_BITS):
        return x
    s = n.bit_length() - d.bit_length() - PREC_BITS
    q = (n + ((d << s) >> 1)) // (d << s) if s >= 0 else ((n << -s) + (d >> 1)) // d
    r = Fraction(q << s) if s >= 0 else Fraction(q, 1 << -s)
    return r if x > 0 else -r


def dsqrt(x: Fraction) -> Fraction:
    """sqrt(x) to 80 significant digits (exact for the squares of short decimals, e.g. 25 * 4^-k)."""
    if x < 0:
        raise ValueError("sqrt of a negative value")
    if x == 0:
        return Fraction(0)
    with localcontext() as ctx:
        ctx.prec = 80
        return rnd(Fraction((Decimal(x.numerator) / Decimal(x.denominator)).sqrt()))


class B:
    """An exact value with its forward-error magnitude (see the module docstring)."""
    __slots__ = ("v", "m")

    def __init__(self, v, m=None):
        self.v = v if isinstance(v, Fraction) else Fraction(v)
        self.m = abs(self.v) if m is None else m

    def __add__(self, o):
        o = o if isinstance(o, B) else B(o)
        return B(self.v + o.v, _up(self.m + o.m))

    __radd__ = __add__

    def __neg__(self):
        return B(-self.v, self.m)

    def __sub__(self, o):
        o = o if isinstance(o, B) else B(o)
        return B(self.v - o.v, _up(self.m + o.m))

    def __rsub__(self, o):
        return (-self) + o

    def __mul__(self, o):
        o = o if isinstance(o, B) else B(o)
        return B(self.v * o.v, _up(self.m * abs(o.v) + abs(self.v) * o.m))

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = o if isinstance(o, B) else B(o)
        if o.v == 0:
            raise ZeroDivisionError("exact division by zero: no exact value exists")
        q = self.v / o.v
        return B(q, _up(self.m / abs(o.v) + abs(q) * o.m / abs(o.v)))

    def __rtruediv__(self, o):
        return B(o) / self

    def rounded(self):
        """The value rounded to PREC_BITS bits (the bound is unchanged: 2^-256 is far below any tolerance here)."""
        return B(rnd(self.v), self.m)

    def sqrt(self):
        r = dsqrt(self.v)
        if r == 0:
            return B(0, _up(dsqrt(self.m)))
        return B(r, _up(r + self.m / (2 * r)))

    def __repr__(self):
        return f"B({float(self.v)!r} +- {float(self.m)!r})"


def bsum(xs) -> B:
    acc = B(0)
    for x in xs:
        acc = acc + x
    return acc


class Dual:
    """Forward-mode dual number over Fraction: value a, derivative b along one direction."""
    __slots__ = ("a", "b")

    def __init__(self, a, b=0):
        self.a, self.b = Fraction(a), Fraction(b)

    def __add__(self, o):
        o = o if isinstance(o, Dual) else Dual(o)
        return Dual(self.a + o.a, self.b + o.b)

    __radd__ = __add__

    def __sub__(self, o):
        o = o if isinstance(o, Dual) else Dual(o)
        return Dual(self.a - o.a, self.b - o.b)

    def __rsub__(self, o):
        return Dual(o) - self

    def __mul__(self, o):
        o = o if isinstance(o, Dual) else Dual(o)
        return Dual(self.a * o.a, self.a * o.b + self.b * o.a)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = o if isinstance(o, Dual) else Dual(o)
        return Dual(self.a / o.a, (self.b * o.a - self.a * o.b) / (o.a * o.a))


def F(x) -> Fraction:
    """A double converted exactly."""
    return Fraction(float(x))


# ---------------------------------------------------------------------------------------------------------------------
# one observation
# ---------------------------------------------------------------------------------------------------------------------
def _cross(i, p):
    """e_i x p."""
    X, Y, Z = p
    return [(0, -Z, Y), (Z, 0, -X), (-Y, X, 0)][i]


def _residual(p, m, cam):
    """e = m - (K p)[:2] / (K p)[2] on any number type: (fx X + cx Z) / Z as frontend.py:275-277."""
    fx, fy, cx, cy = cam
    X, Y, Z = p
    return (m[0] - (fx * X + cx * Z) / Z, m[1] - (fy * Y + cy * Z) / Z)


def dual_jacobians(P, X, m, cam):
    """(Jp [2][6], Jq [2][3]) as Fractions: derivatives of e along the pose tangent (exp([w, v]) T, rotation first)
    and along the world point, by dual numbers."""
    R = [P[0:3], P[4:7], P[8:11]]
    t = (P[3], P[7], P[11])
    p = [sum(R[i][j] * X[j] for j in range(3)) + t[i] for i in range(3)]
    dirs = [_cross(i, p) for i in range(3)] + [tuple(1 if j == i else 0 for j in range(3)) for i in range(3)]
    dirs += [tuple(R[i][c] for i in range(3)) for c in range(3)]       # dp / dX_c = R[:, c]
    cols = []
    for d in dirs:
        e = _residual([Dual(p[i], d[i]) for i in range(3)], m, cam)
        cols.append((e[0].b, e[1].b))
    Jp = [[cols[c][r] for c in range(6)] for r in range(2)]
    Jq = [[cols[6 + c][r] for c in range(3)] for r in range(2)]
    return Jp, Jq


def closed_form_jacobians(Pb, pb, cam_b, eps):
    """frontend.py:286-291 (and the point Jacobian -A R of the kernels) on B values with Zinv = 1 / (Z + eps)."""
    fx, fy, _, _ = cam_b
    X, Y, Z = pb
    Zinv = B(1) / (Z + eps)
    Zinv2 = Zinv * Zinv
    zero = B(0)
    Jp = [[fx * X * Y * Zinv2, -fx - fx * X * X * Zinv2, fx * Y * Zinv, -fx * Zinv, zero, fx * X * Zinv2],
          [fy + fy * Y * Y * Zinv2, -fy * X * Y * Zinv2, -fy * X * Zinv, zero, -fy * Zinv, fy * Y * Zinv2]]
    A0, A2, A4, A5 = fx * Zinv, -fx * X * Zinv2, fy * Zinv, -fy * Y * Zinv2
    Jq = [[-(A0 * Pb[c] + A2 * Pb[8 + c]) for c in range(3)], [-(A4 * Pb[4 + c] + A5 * Pb[8 + c]) for c in range(3)]]
    return Jp, Jq


@dataclass
class Lin:
    """One observation linearised exactly: p [3], e [2], Jp [2][6], Jq [2][3], c2, all B."""
    p: list
    e: tuple
    Jp: list
    Jq: list
    c2: B

    def summand(self):
        """(e, Jp, Jq) rounded to PREC_BITS bits: what enters sums over observations."""
        return ([x.rounded() for x in self.e], [[x.rounded() for x in r] for r in self.Jp],
                [[x.rounded() for x in r] for r in self.Jq])


def linearise(P12, X3, m2, cam, literal: bool = False) -> Lin:
    """Exact residual and Jacobians of one observation; ``literal`` takes the frontend.py:286-291 expression with the
    1e-18 as the Jacobian reference (the tiny_z case), else the dual-number derivative.  Bounds come from the expression
    the kernels evaluate (with the 1e-18)."""
    P = [F(v) for v in P12]
    X = [F(v) for v in X3]
    m = [F(v) for v in m2]
    cb = [B(F(v)) for v in cam]
    Pb = [B(v) for v in P]
    pb = [Pb[4 * i] * B(X[0]) + Pb[4 * i + 1] * B(X[1]) + Pb[4 * i + 2] * B(X[2]) + Pb[4 * i + 3] for i in range(3)]
    e = _residual(pb, [B(v) for v in m], cb)
    Jpc, Jqc = closed_form_jacobians(Pb, pb, cb, B(EPS_Z))
    if not literal:
        Jpd, Jqd = dual_jacobians(P, X, m, [F(v) for v in cam])
        Jpc = [[B(Jpd[r][c], Jpc[r][c].m) for c in range(6)] for r in range(2)]
        Jqc = [[B(Jqd[r][c], Jqc[r][c].m) for c in range(3)] for r in range(2)]
    return Lin(p=pb, e=e, Jp=Jpc, Jq=Jqc, c2=e[0] * e[0] + e[1] * e[1])


def huber(c2: B, delta) -> tuple:
    """(w, rho) of g2o's RobustKernelHuber at e.e = c2 (delta <= 0: no kernel).  The weight is exact (80-digit sqrt);
    where the kernel's rounded sqrt(c2) may fall on the other side of delta than the exact one, the bound covers both
    branches (the function is continuous there, so the difference is of the order of that rounding)."""
    delta = F(delta)
    if delta <= 0:
        return B(1), c2
    en = c2.sqrt()
    near = abs(en.v - delta) <= C * U * en.m
    if c2.v <= delta * delta:
        w, rho = B(1), c2
        if near:
            wo, ro = (B(delta) / en).rounded(), 2 * B(delta) * en - B(delta * delta)
            w, rho = B(1, max(Fraction(1), wo.m)), B(c2.v, _up(c2.m + ro.m))
    else:
        w, rho = (B(delta) / en).rounded(), 2 * B(delta) * en - B(delta * delta)
        if near:
            w, rho = B(w.v, max(Fraction(1), w.m)), B(rho.v, _up(rho.m + c2.m))
    return w, rho


# ---------------------------------------------------------------------------------------------------------------------
# normal equations of one pose and the Schur reduction of a window
# ---------------------------------------------------------------------------------------------------------------------
def pose_normal_eq(lins, active, delta):
    """(H [6][6], b [6], chi2 [O]) over the active observations: H = sum w Jp^T Jp, b = sum w Jp^T e; chi2 for all."""
    H = [[B(0)] * 6 for _ in range(6)]
    b = [B(0)] * 6
    for q, act in zip(lins, active):
        if not act:
            continue
        w, _ = huber(q.c2, delta)
        e, J, _ = q.summand()
        for a in range(6):
            for c in range(a, 6):
                H[a][c] = H[a][c] + w * (J[0][a] * J[0][c] + J[1][a] * J[1][c])
            b[a] = b[a] + w * (J[0][a] * e[0] + J[1][a] * e[1])
    for a in range(6):
        for c in range(a):
            H[a][c] = H[c][a]
    return H, b, [q.c2 for q in lins]


def inverse3(M):
    """Exact inverse of a symmetric 3x3 B matrix by cofactors (the kernels' ba_damped_inverse expression)."""
    m00, m01, m02, m11, m12, m22 = M[0][0], M[0][1], M[0][2], M[1][1], M[1][2], M[2][2]
    c00 = m11 * m22 - m12 * m12
    c01 = m02 * m12 - m01 * m22
    c02 = m01 * m12 - m02 * m11
    det = m00 * c00 + m01 * c01 + m02 * c02
    c11 = m00 * m22 - m02 * m02
    c12 = m01 * m02 - m00 * m12
    c22 = m00 * m11 - m01 * m01
    E = [[c00, c01, c02], [c01, c11, c12], [c02, c12, c22]]
    return [[(E[i][j] / det).rounded() for j in range(3)] for i in range(3)]


def _mm(A, Bm, tb=False):
    n, k = len(A), len(A[0])
    cols = len(Bm) if tb else len(Bm[0])
    get = (lambda r, c: Bm[c][r]) if tb else (lambda r, c: Bm[r][c])
    return [[bsum(A[i][r] * get(r, j) for r in range(k)) for j in range(cols)] for i in range(n)]


def schur(lins, obs_pose, obs_point, K, L, delta, lam):
    """The reduction of oracle.ba_schur_np, exactly: S [K][K][6][6], rhs [K][6], bp [K][6], bl [L][3], E [L][3][3],
    Hpl [O][6][3], cost per pose [K], the diagonals of Hpp [K][6] and Hll [L][3], seen [L]."""
    lam = B(F(lam))
    Hpp = [[[B(0)] * 6 for _ in range(6)] for _ in range(K)]
    bp = [[B(0)] * 6 for _ in range(K)]
    Hll = [[[B(0)] * 3 for _ in range(3)] for _ in range(L)]
    bl = [[B(0)] * 3 for _ in range(L)]
    cost = [B(0)] * K
    Hpl = []
    seen = [False] * L
    for o, q in enumerate(lins):
        k, l = int(obs_pose[o]), int(obs_point[o])
        seen[l] = True
        w, rho = huber(q.c2, delta)
        cost[k] = cost[k] + rho
        e, Jp, Jq = q.summand()
        for a in range(6):
            for c in range(6):
                Hpp[k][a][c] = Hpp[k][a][c] + w * (Jp[0][a] * Jp[0][c] + Jp[1][a] * Jp[1][c])
            bp[k][a] = bp[k][a] + w * (Jp[0][a] * e[0] + Jp[1][a] * e[1])
        for a in range(3):
            for c in range(3):
                Hll[l][a][c] = Hll[l][a][c] + w * (Jq[0][a] * Jq[0][c] + Jq[1][a] * Jq[1][c])
            bl[l][a] = bl[l][a] + w * (Jq[0][a] * e[0] + Jq[1][a] * e[1])
        Hpl.append([[w * (Jp[0][a] * Jq[0][c] + Jp[1][a] * Jq[1][c]) for c in range(3)] for a in range(6)])
    eye3 = [[B(1 if i == j else 0) for j in range(3)] for i in range(3)]
    E = [inverse3([[Hll[l][i][j] + (lam if i == j else B(0)) for j in range(3)] for i in range(3)]) if seen[l] else eye3
         for l in range(L)]
    Y = [_mm(Hpl[o], E[int(obs_point[o])]) for o in range(len(lins))]
    S = [[[[B(0)] * 6 for _ in range(6)] for _ in range(K)] for _ in range(K)]
    for k in range(K):
        S[k][k] = [[Hpp[k][a][c] + (lam if a == c else B(0)) for c in range(6)] for a in range(6)]
    rhs = [[-bp[k][a] for a in range(6)] for k in range(K)]
    by_point = [[] for _ in range(L)]
    for o in range(len(lins)):
        by_point[int(obs_point[o])].append(o)
    for l in range(L):
        for o1 in by_point[l]:
            k1 = int(obs_pose[o1])
            for a in range(6):
                rhs[k1][a] = rhs[k1][a] + bsum(Y[o1][a][c] * bl[l][c] for c in range(3))
            for o2 in by_point[l]:
                k2 = int(obs_pose[o2])
                W = _mm(Y[o1], Hpl[o2], tb=True)
                S[k1][k2] = [[S[k1][k2][a][c] - W[a][c] for c in range(6)] for a in range(6)]
    return {"S": S, "rhs": rhs, "bp": bp, "bl": bl, "E": E, "Hpl": Hpl, "cost": cost, "seen": seen,
            "hpp_diag": [[Hpp[k][a][a] for a in range(6)] for k in range(K)],
            "hll_diag": [[Hll[l][a][a] for a in range(3)] for l in range(L)]}


def backsub(red, obs_pose, obs_point, dp):
    """dl[l] = E[l] (-bl[l] - sum_o Hpl[o]^T dp[pose(o)]); zero for points nobody observes."""
    L = len(red["bl"])
    dpb = [[B(F(v)) for v in row] for row in np.asarray(dp, np.float64).reshape(-1, 6)]
    tmp = [[-red["bl"][l][c] for c in range(3)] for l in range(L)]
    for o, H in enumerate(red["Hpl"]):
        k, l = int(obs_pose[o]), int(obs_point[o])
        for c in range(3):
            tmp[l][c] = tmp[l][c] - bsum(H[a][c] * dpb[k][a] for a in range(6))
    return [[bsum(red["E"][l][c][j] * tmp[l][j] for j in range(3)) if red["seen"][l] else B(0) for c in range(3)]
            for l in range(L)]


def diag_max(red, free=None) -> B:
    """Largest diagonal entry of the Hpp blocks of ``free`` (all if None) and of every Hll (SchurProblem.diag_max)."""
    K = len(red["hpp_diag"])
    cand = [d for k in (range(K) if free is None else free) for d in red["hpp_diag"][k]]
    if any(red["seen"]):
        cand += [d for row in red["hll_diag"] for d in row]
    if not cand:
        return B(0)
    top = max(cand, key=lambda x: x.v)
    return B(top.v, max(x.m for x in cand))


# ---------------------------------------------------------------------------------------------------------------------
# comparison under the tolerance rule
# ---------------------------------------------------------------------------------------------------------------------
def _flat(ref):
    if isinstance(ref, B):
        return [ref]
    out = []
    for r in ref:
        out.extend(_flat(r))
    return out


def violations(got, ref):
    """[(flat index, got, exact, allowed)] of the entries of ``got`` (float array) outside C 2^-53 bound of ``ref``."""
    g = np.asarray(got, np.float64).reshape(-1)
    r = _flat(ref)
    assert g.size == len(r), (g.size, len(r))
    bad = []
    for i, (x, b) in enumerate(zip(g.tolist(), r)):
        tol = C * U * b.m
        if not np.isfinite(x) or abs(Fraction(x) - b.v) > tol:
            bad.append((i, x, float(b.v), float(tol)))
    return bad


def assert_exact(got, ref, what=""):
    bad = violations(got, ref)
    assert not bad, f"{what}: {len(bad)} entries outside C 2^-53 bound, first {bad[:4]} (index, got, exact, allowed)"


def values(ref) -> np.ndarray:
    """The exact values rounded to doubles (for shapes, masks and inputs derived from exact results)."""
    return np.array([float(b.v) for b in _flat(ref)])


# ---------------------------------------------------------------------------------------------------------------------
# the geometry set
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    poses12: np.ndarray      # [K,12] rows of [R|t]
    points: np.ndarray       # [L,3] world points
    obs_pose: np.ndarray     # [O] int32
    obs_point: np.ndarray    # [O] int32
    meas: np.ndarray         # [O,2]
    cam: tuple               # fx, fy, cx, cy
    delta: float             # a Huber delta that splits the observations of this case
    literal: bool            # Jacobian reference: the frontend.py expression with the 1e-18 (tiny_z), else the derivative

    @property
    def K(self):
        return self.poses12.shape[0]

    @property
    def L(self):
        return self.points.shape[0]

    @property
    def O(self):
        return self.obs_pose.shape[0]


def _rotvec(w):
    from scipy.spatial.transform import Rotation

    return Rotation.from_rotvec(w).as_matrix()


def _visibility(rng, K, L):
    """Observations of K poses and L points: point 0 seen by every pose, point 1 only by pose 0, point L-1 by nobody,
    the rest with probability 0.7; pose-major order."""
    vis = rng.uniform(size=(K, L)) < 0.7
    vis[:, 0] = True
    vis[:, 1] = False
    vis[0, 1] = True
    vis[:, L - 1] = False
    op, ol = np.nonzero(vis)
    return op.astype(np.int32), ol.astype(np.int32)


def _project_f64(poses12, points, op, ol, cam):
    fx, fy, cx, cy = cam
    P = poses12.reshape(-1, 3, 4)
    pc = np.einsum("oij,oj->oi", P[op, :, :3], points[ol]) + P[op, :, 3]
    return np.c_[fx * pc[:, 0] / pc[:, 2] + cx, fy * pc[:, 1] / pc[:, 2] + cy]


def _pack(R, t):
    return np.concatenate([np.asarray(R, np.float64), np.asarray(t, np.float64)[:, :, None]], 2).reshape(len(R), 12)


def _generic(name, rng, R, t, X, cam=EUROC, noise=1.0, literal=False):
    K, L = len(R), len(X)
    poses12 = _pack(R, t)
    op, ol = _visibility(rng, K, L)
    meas = _project_f64(poses12, X, op, ol, cam) + rng.normal(0, noise, (len(op), 2))
    return Case(name, poses12, np.asarray(X, np.float64), op, ol, meas, cam, noise, literal)


def _huber_edge(rng):
    """Identity poses, fx = fy = 512, cx = cy = 256, Z a power of two and X/Z, Y/Z multiples of 1/64: every projection
    is exact in f64.  Residuals (3, 4) 2^-k in all sign and order variants, exactly at delta = 5 2^-k, one measurement
    ulp either side, and clearly inside / outside."""
    k = 3
    delta = 5.0 * 2.0 ** -k
    K, L = 3, 40
    cam = (512.0, 512.0, 256.0, 256.0)
    R = np.tile(np.eye(3), (K, 1, 1))
    t = np.zeros((K, 3))
    Z = 2.0 ** rng.integers(0, 5, L)
    X = np.c_[rng.integers(-32, 33, (L, 2)) / 64.0 * Z[:, None], Z]
    op, ol = _visibility(rng, K, L)
    proj = _project_f64(_pack(R, t), X, op, ol, cam)
    base = np.array([3.0, 4.0]) * 2.0 ** -k
    meas = np.empty_like(proj)
    for o in range(len(op)):
        e = base[::-1] if o % 2 else base.copy()
        e = e * np.where(rng.uniform(size=2) < 0.5, -1.0, 1.0)
        kind = o % 5
        if kind == 3:
            e = e * 0.5                          # inside
        if kind == 4:
            e = e * 2.0                          # outside
        m = proj[o] + e                          # exact: proj and e are short dyadics
        if kind == 1:
            m = np.nextafter(m, np.inf * np.sign(e))      # one ulp further out
        if kind == 2:
            m = np.nextafter(m, -np.inf * np.sign(e))     # one ulp further in
        meas[o] = m
    return Case("huber_edge", _pack(R, t), X, op, ol, meas, cam, delta, False)


def _make(name: str) -> Case:
    rng = np.random.default_rng(CASES.index(name) + 1000)
    K, L = 3, 40

    def small_rot(s=0.15):
        return _rotvec(rng.uniform(-s, s, (K, 3)))

    if name == "benign":                         # test_optimize_gpu._scene's distribution
        X = np.c_[rng.uniform(-4, 4, (L, 2)), rng.uniform(6, 15, L)]
        return _generic(name, rng, small_rot(), rng.uniform(-0.5, 0.5, (K, 3)), X)
    if name == "wide":                           # up to ~80 degrees off the axis
        z = rng.uniform(2, 10, L)
        X = np.c_[rng.uniform(-5.5, 5.5, (L, 2)) * z[:, None], z]
        return _generic(name, rng, small_rot(0.05), rng.uniform(-0.2, 0.2, (K, 3)), X)
    if name == "far":                            # translation columns ~1e-5 of the rotation columns
        z = 10.0 ** rng.uniform(3, 5, L)
        X = np.c_[rng.uniform(-0.5, 0.5, (L, 2)) * z[:, None], z]
        return _generic(name, rng, small_rot(), rng.uniform(-0.5, 0.5, (K, 3)), X)
    if name == "near":                           # Jacobian entries ~1e9
        z = 10.0 ** rng.uniform(-3, -2, L)
        X = np.c_[rng.uniform(-0.5, 0.5, (L, 2)) * z[:, None], z]
        return _generic(name, rng, small_rot(0.05), rng.uniform(-1e-5, 1e-5, (K, 3)), X)
    if name == "cancel":                         # world ~1e4, t ~ -R c: p = O(10) after cancellation
        base = np.array([1.2e4, -0.7e4, 0.9e4])
        R = small_rot()
        c = base + rng.uniform(-0.5, 0.5, (K, 3))
        t = -np.einsum("kij,kj->ki", R, c)
        X = base + np.c_[rng.uniform(-4, 4, (L, 2)), rng.uniform(6, 15, L)]
        return _generic(name, rng, R, t, X)
    if name == "rotations":                      # the exact identity, exact quarter turns, angles within 1e-6 of pi
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        R = np.stack([np.eye(3),
                      [[1, 0, 0], [0, 0, -1], [0, 1, 0]],
                      [[0, 0, 1], [0, 1, 0], [-1, 0, 0]],
                      [[0, -1, 0], [1, 0, 0], [0, 0, 1]],
                      _rotvec((np.pi - 3e-7) * n),
                      _rotvec([0.0, 0.0, np.pi - 1e-6])]).astype(np.float64)
        t = np.tile([0.0, 0.0, 20.0], (len(R), 1))            # every camera 20 units from the cloud, looking at it
        X = rng.uniform(-5, 5, (L, 3))
        rng2 = np.random.default_rng(7)
        return _generic(name, rng2, R, t, X)
    if name == "behind":                         # Z < 0: defined, not rejected by the reference
        X = np.c_[rng.uniform(-4, 4, (L, 2)), -rng.uniform(6, 15, L)]
        return _generic(name, rng, small_rot(), rng.uniform(-0.5, 0.5, (K, 3)), X)
    if name == "tiny_z":                         # |Z| in [1e-12, 1e-6], both signs: the 1e-18 of frontend.py:286 matters
        R = np.stack([np.eye(3), [[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.eye(3)]).astype(np.float64)
        t = np.c_[rng.uniform(-0.5, 0.5, (K, 2)), np.zeros(K)]   # t_z = 0 and R's last row e_z: Z = the point's z exactly
        z = 10.0 ** rng.uniform(-12, -6, L) * rng.choice([-1.0, 1.0], L)
        X = np.c_[rng.uniform(-1, 1, (L, 2)), z]
        return _generic(name, rng, R, t, X, literal=True)
    if name == "huber_edge":
        return _huber_edge(rng)
    raise KeyError(name)


@lru_cache(maxsize=None)
def case(name: str) -> Case:
    return _make(name)


@lru_cache(maxsize=None)
def exact_lins(name: str) -> tuple:
    """The exact linearisation of every observation of a case."""
    c = case(name)
    return tuple(linearise(c.poses12[c.obs_pose[o]], c.points[c.obs_point[o]], c.meas[o], c.cam, c.literal)
                 for o in range(c.O))


def windows(c: Case):
    """Windows of at most 4 poses for the Schur reduction: up to three observed poses of the case and one pose with no
    observation.  Yields (pose index list, observation index array)."""
    for s in range(0, c.K, 3):
        ks = list(range(s, min(s + 3, c.K)))
        yield ks, np.flatnonzero(np.isin(c.obs_pose, ks))


def conditioned(c: Case, sel):
    """``sel`` without the observations of points it sees only once: every point left in it is seen by two or more poses
    (with the parallax of their baselines), or by none."""
    cnt = np.bincount(c.obs_point[sel], minlength=c.L)
    return sel[cnt[c.obs_point[sel]] >= 2]


def scaled_lambda(name: str, sel, scale=0.1) -> float:
    """A damping proportional to the point blocks: ``scale`` times the median diagonal entry of the (unweighted) Hll of
    the points ``sel`` observes, so that Hll + lambda I is well conditioned for each of them."""
    c = case(name)
    jq = np.array([values(q.Jq) for q in (exact_lins(name)[o] for o in sel)]).reshape(-1, 2, 3)
    d = np.zeros((c.L, 3))
    np.add.at(d, c.obs_point[sel], (jq * jq).sum(1))
    return float(scale * np.median(d[np.bincount(c.obs_point[sel], minlength=c.L) > 0]))


def relative_allowance(ref) -> np.ndarray:
    """C 2^-53 bound / |exact| of every nonzero entry: how large a relative error the tolerance rule lets through."""
    r = [b for b in _flat(ref) if b.v != 0]
    return np.array([float(C * U * b.m / abs(b.v)) for b in r])


# The Schur checks run each case twice.  WELL CONDITIONED: only points seen by two or more poses (or by none), and a damping
# scaled to the point blocks (scaled_lambda), so that E = (Hll + lambda I)^-1 is well conditioned and the bound of S, rhs
# and dl stays a small fraction of their values (test_*: the median allowance of S and rhs is checked, and dropping the
# point elimination, dropping the coupling blocks, or scaling rhs or dl by 1 + 1e-6 must all fail).  EXTREME: the point
# seen once (Hll of rank 2) and lambda = 1e-8 or 1e3; there E is as ill conditioned as f64 makes it, S, rhs and dl carry
# bounds of that size, and only the quantities E does not enter (bp, bl, the cost, the largest diagonal entry) are
# constrained tightly.
HUBER_SCHUR = ("wide", "near", "rotations", "huber_edge")     # the Huber kernel on in these cases' Schur checks


def schur_configs(name: str, extreme: bool = False):
    """Yields (pose list, observation indices, delta, lambda) for the Schur checks of a case (see the note above)."""
    c = case(name)
    delta = c.delta if name in HUBER_SCHUR else 0.0
    for i, (ks, sel) in enumerate(windows(c)):
        if extreme:
            yield ks, sel, delta, (1e-8, 1e3)[(CASES.index(name) + i) % 2]
        else:
            sel = conditioned(c, sel)
            yield ks, sel, delta, scaled_lambda(name, sel)


def assert_schur_is_tight(S, rhs, bp, dl, ref, dl_ref, what=""):
    """The well-conditioned Schur check can fail: the median allowance of S and rhs is below 2e-6 relative, and each of
    these wrong results of a reduction that passes is outside the bound: rhs = -bp (no point elimination), S without its
    inter-pose blocks, rhs and dl scaled by 1 + 1e-6."""
    for key, v in (("S", ref["S"]), ("rhs", ref["rhs"])):
        med = float(np.median(relative_allowance(v)))
        assert med <= 2e-6, f"{what}: the bound of {key} allows {med:.1e} relative (median): too loose to test anything"
    S = np.array(S, np.float64)
    K = S.shape[0]
    uncoupled = S.copy()
    uncoupled[~np.eye(K, dtype=bool)] = 0.0
    for name, got, r in (("rhs = -bp", -np.asarray(bp), ref["rhs"]), ("S without coupling blocks", uncoupled, ref["S"]),
                         ("rhs * (1 + 1e-6)", np.asarray(rhs) * (1 + 1e-6), ref["rhs"]),
                         ("dl * (1 + 1e-6)", np.asarray(dl) * (1 + 1e-6), dl_ref)):
        assert violations(got, r), f"{what}: {name} passes the bound"


def window_problem(c: Case, ks, sel):
    """(poses12 [len(ks)+1, 12], obs_pose remapped, obs_point, meas) of a window; the extra last pose sees nothing."""
    remap = {k: i for i, k in enumerate(ks)}
    poses = np.concatenate([c.poses12[ks], c.poses12[ks[:1]]])
    op = np.array([remap[int(k)] for k in c.obs_pose[sel]], np.int32)
    return poses, op, c.obs_point[sel].astype(np.int32), c.meas[sel]
