"""Cases for the sparse bundle adjustment (csrc/ba_sparse.hip) whose results are EXACT, and their statement in exact
rational arithmetic.  Shared by tests/test_ba_sparse_edges_cpu.py (which asserts that every case has the property it
exists for) and tests/test_ba_sparse_edges_gpu.py (which compares the kernels with these statements byte for byte).

ba_sparse.hip is compiled without contraction and every sum has a fixed order.  Where every term of every sum is a dyadic
rational of few bits, every partial sum is representable, so the f64 result is the exact one WHATEVER the order: a dropped,
doubled or mis-indexed term shows at any list length, and no tolerance is needed.  Two families:

(A) grid scenes for the linearisation: fx = fy = 256, cx = 320, cy = 240; poses are signed axis permutations with integer
    translations; every observed point has camera coordinates X, Y integers in [-4, 4] and Z in {1, 2, 4, 8}; a measurement
    is the exact projection plus a residual of RESIDUALS (norms 0, 5, 10, 20: Huber weights 1, 1/2, 1/4 at delta = 5, and
    norm 5 = delta keeps weight 1 because the gate is strict).
(B) synthetic blocks for reduce, back-substitution and candidate: Hpl, Hpp, bp, bl, dp small integers and Hll + lambda I one
    of UNIMODULAR (integer, symmetric, positive definite, determinant 1 or a power of two), so that the cofactor inverse is
    exact.

The exact statement: one observation is linearised in fractions.Fraction (`linearise_fraction`, ba_linearise of ba_common.h
term by term); the sums are then taken over a common denominator in 64-bit integers (asserted not to overflow), which is
the same rational arithmetic, a thousand times faster.  `*_fraction` functions state single blocks in Fractions from end to
end; the CPU file holds the integer path to them.  The sign of a zero is not part of any statement (`bits` drops it).
"""
import math
from fractions import Fraction as F

import numpy as np

import ba_sparse_ref as R

GRID_INTR = (256.0, 256.0, 320.0, 240.0)
RESIDUALS = ((0, 0), (3, 4), (-4, 3), (6, 8), (-8, 6), (12, -16))
SQRT2 = float(np.sqrt(2.0))             # a Huber delta that IS the f64 norm of a residual (1, 1) while its square is not 2
RESIDUALS_SQRT2 = ((0, 0), (1, 1), (-1, 1), (1, -1), (-1, -1))
TRI = [(a, c) for a in range(6) for c in range(a, 6)]       # packed upper triangle of a 6x6, rows of 6, 5, .. entries
TRI3 = [(a, c) for a in range(3) for c in range(a, 3)]


def bits(a):
    """The bytes of an f64 array with the sign of zeros dropped (x + 0.0 turns -0.0 into +0.0 and nothing else)."""
    return (np.ascontiguousarray(a, np.float64) + 0.0).tobytes()


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bits(a) == bits(b)


def exact_f64(num, den):
    """num / den as f64, asserted exact: den a power of two and |num| < 2^53."""
    num = np.asarray(num, np.int64)
    assert den > 0 and den & (den - 1) == 0, den
    assert int(np.abs(num).max(initial=0)) < 2 ** 53
    return num.astype(np.float64) / float(den)


# ---- case 1: the layout with long lists ------------------------------------------------------------------------------------
LONG_OBS = {1: 1025, 2: 255, 3: 256, 4: 257, 5: 512, 6: 513, 7: 1}
LONG_EDGES = {(2, 3): 63, (3, 4): 64, (4, 5): 65, (5, 6): 128, (1, 6): 129, (1, 7): 1, (6, 7): 1}


def long_layout(variant="e7", seed=11):
    """Tracks (one tuple of poses per point, in a shuffled order) of the long-list layout -> dict(K, tracks, fixed, obs, edges).

    Pose 0 is fixed and has the most observations; free poses 2..6 have exactly 255, 256, 257, 512 and 513, pose 1 has 1025,
    pose 7 has one; the covisibility edges are exactly LONG_EDGES (63, 64, 65, 128 and 129 pairs and two of one pair);
    tracks of length 1 and two points nobody observes are present.  Variant "e7": K = 8 and E = 7; variant "e8": a pose 8
    with two observations adds the edge (2, 8), so E = 8 is a multiple of the four edges a workgroup takes."""
    groups = [((2, 3), 63), ((3, 4), 64), ((4, 5), 65), ((5, 6), 128), ((1, 6), 128), ((1, 6, 7), 1), ((0, 2), 100), ((2,), 92),
              ((0, 3), 129), ((4,), 64), ((0, 4), 64), ((0, 5), 319), ((0, 6), 256), ((0, 1), 600), ((1,), 296), ((), 2)]
    obs, edges, K = dict(LONG_OBS), dict(LONG_EDGES), 8
    if variant == "e8":
        groups[6] = ((0, 2), 99)
        groups += [((0, 2, 8), 1), ((0, 8), 1)]
        obs[8], edges[(2, 8)], K = 2, 1, 9
    else:
        assert variant == "e7"
    tracks = [t for t, n in groups for _ in range(n)]
    order = np.random.default_rng(seed).permutation(len(tracks))
    tracks = [tracks[i] for i in order]
    obs[0] = sum(1 for t in tracks if 0 in t)
    return dict(K=K, tracks=tracks, fixed=(0,), obs=obs, edges=edges, name=f"long-{variant}")


def hub_layout(seed=12):
    """K = 41, pose 0 fixed: one point seen by all 41 poses (a track of 40 free poses and the fixed one), 60 tracks of
    length 1, 30 tracks of two consecutive poses, three points nobody observes."""
    tracks = [tuple(range(41))] + [(1 + i % 40,) for i in range(60)] + [(1 + i, 2 + i) for i in range(30)] + [()] * 3
    order = np.random.default_rng(seed).permutation(len(tracks))
    return dict(K=41, tracks=[tracks[i] for i in order], fixed=(0,), name="hub41")


def big_layout(winner):
    """K = 300, L = 300, pose 0 fixed, point k seen by pose k; the largest diagonal entry of the free Hpp and all Hll lies
    at pose 299 (winner "pose": it sees every point) or at point 299 (winner "point": every pose sees it), i.e. in the second
    trip of the maximum's loop over 256 threads."""
    if winner == "pose":
        tracks = [(k, 299) if k != 299 else (299,) for k in range(300)]
    else:
        assert winner == "point"
        tracks = [(k,) for k in range(299)] + [tuple(range(300))]
    return dict(K=300, tracks=tracks, fixed=(0,), name=f"big-{winner}")


def observations(tracks, seed):
    """(obs_pose, obs_point) int32 of a list of tracks, shuffled."""
    op = np.array([k for t in tracks for k in t], np.int32)
    ol = np.array([l for l, t in enumerate(tracks) for _ in t], np.int32)
    perm = np.random.default_rng(seed).permutation(len(op))
    return op[perm], ol[perm]


def random_window(layout, seed=5):
    """The layout on ba_sparse_ref's random scene (its intrinsics, 0.3 px noise, perturbed poses and points)."""
    return R.tracks_window(np.random.default_rng(seed), layout["K"], layout["tracks"], layout["fixed"])


# ---- family (A): grid scenes ---------------------------------------------------------------------------------------------
_RZ = [np.array(m) for m in ([[1, 0, 0], [0, 1, 0], [0, 0, 1]], [[0, -1, 0], [1, 0, 0], [0, 0, 1]], [[-1, 0, 0], [0, -1, 0], [0, 0, 1]],
                             [[0, 1, 0], [-1, 0, 0], [0, 0, 1]])]
_RCYC = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]])          # camera (X, Y, Z) = world (z, x, y): not a rotation about z


def _camera_ok(pc):
    return abs(int(pc[0])) <= 4 and abs(int(pc[1])) <= 4 and int(pc[2]) in (1, 2, 4, 8)


def grid_scene(layout, seed, xy=3, residuals=RESIDUALS, cyclic=(2,), zs=(1, 2, 4, 8), tag=""):
    """A grid scene on a layout: poses [K,3,4] of integers (rotations about z by multiples of 90 degrees with a translation in
    {-1, 0, 1}^2 x {0}; the poses in `cyclic` a cyclic axis permutation), world points of integers drawn until every pose of
    the track sees them at X, Y in [-4, 4] and Z in {1, 2, 4, 8}, measurements the exact projection plus one of `residuals`."""
    rng = np.random.default_rng(seed)
    K, tracks = layout["K"], layout["tracks"]
    T = np.zeros((K, 3, 4), np.int64)
    for k in range(K):
        T[k, :, :3] = _RCYC if k in cyclic and K < 100 else _RZ[int(rng.integers(4))]
        T[k, :2, 3] = rng.integers(-1, 2, 2)
    X = np.zeros((len(tracks), 3), np.int64)
    for l, t in enumerate(tracks):
        for _ in range(10000):
            p = np.array([rng.integers(-xy, xy + 1), rng.integers(-xy, xy + 1), zs[int(rng.integers(len(zs)))]])
            if all(_camera_ok(T[k, :, :3] @ p + T[k, :, 3]) for k in t):
                break
        else:
            raise AssertionError(f"no grid point for track {t}")
        X[l] = p
    op, ol = observations(tracks, seed + 1)
    pc = np.einsum("oij,oj->oi", T[op, :, :3], X[ol]) + T[op, :, 3]
    res = np.array(residuals, np.int64)[rng.integers(0, len(residuals), len(op))]
    fx, fy, cx, cy = (int(v) for v in GRID_INTR)
    assert (fx * pc[:, 0] % pc[:, 2] == 0).all() and (fy * pc[:, 1] % pc[:, 2] == 0).all()
    meas = np.stack([fx * pc[:, 0] // pc[:, 2] + cx, fy * pc[:, 1] // pc[:, 2] + cy], 1) + res
    fixed = np.zeros(K, bool)
    fixed[list(layout["fixed"])] = True
    return dict(name=f"{layout['name']}-grid{seed}{tag}", K=K, L=len(tracks), T12=T.reshape(K, 12).astype(np.float64), X=X.astype(np.float64),
                op=op, ol=ol, meas=meas.astype(np.float64), fixed=fixed, pc=pc, res=res, intr=GRID_INTR)


def grid_scenes():
    """The grid scenes of case 2 with their Huber delta: the long layout at delta 0 and 5, its E = 8 variant, the scene whose
    residual norm EQUALS delta in f64, and K = 300 with the largest diagonal at pose 299 / at point 299.  The seeds are ones
    at which the fixed pose of the long layout holds the largest diagonal entry of all (not every seed does; the CPU file
    asserts it)."""
    lay = long_layout()
    return [(grid_scene(lay, 21), 0.0), (grid_scene(lay, 21), 5.0), (grid_scene(long_layout("e8"), 24), 5.0),
            (grid_scene(lay, 23, residuals=RESIDUALS_SQRT2, tag="-sqrt2"), SQRT2),
            (grid_scene(big_layout("pose"), 24, xy=1, zs=(1,)), 5.0), (grid_scene(big_layout("point"), 25, xy=1, zs=(1,)), 5.0)]


def _fsqrt(q):
    """The square root of a Fraction that is the square of one (ValueError otherwise: the case would not be exact)."""
    n, d = math.isqrt(q.numerator), math.isqrt(q.denominator)
    if n * n != q.numerator or d * d != q.denominator:
        raise ValueError(f"sqrt({q}) is not rational")
    return F(n, d)


def linearise_fraction(P, p, m, intr, delta):
    """ba_linearise (ba_common.h) of one observation in Fractions: pose P (12), point p (3), measurement m (2) ->
    (e [2], jp [2][6], jq [2][3], w, rho).  1 / (Z + 1e-18) is stated as 1 / Z: for |Z| >= 1 the f64 sum Z + 1e-18 is Z.
    The Huber gate `en > delta` is decided on the squares, en^2 > delta^2, with delta the f64 number given."""
    P, p, m = [F(v) for v in P], [F(v) for v in p], [F(v) for v in m]
    fx, fy, cx, cy = (F(v) for v in intr)
    X = P[0] * p[0] + P[1] * p[1] + P[2] * p[2] + P[3]
    Y = P[4] * p[0] + P[5] * p[1] + P[6] * p[2] + P[7]
    Z = P[8] * p[0] + P[9] * p[1] + P[10] * p[2] + P[11]
    assert abs(Z) >= 1
    e = [m[0] - (fx * X + cx * Z) / Z, m[1] - (fy * Y + cy * Z) / Z]
    zi = 1 / Z
    zi2 = zi * zi
    jp = [[fx * X * Y * zi2, -fx - fx * X * X * zi2, fx * Y * zi, -fx * zi, F(0), fx * X * zi2],
          [fy + fy * Y * Y * zi2, -fy * X * Y * zi2, -fy * X * zi, F(0), -fy * zi, fy * Y * zi2]]
    A = [[fx * zi, F(0), -fx * X * zi2], [F(0), fy * zi, -fy * Y * zi2]]
    jq = [[-(A[0][0] * P[c] + A[0][2] * P[8 + c]) for c in range(3)], [-(A[1][1] * P[4 + c] + A[1][2] * P[8 + c]) for c in range(3)]]
    c2 = e[0] * e[0] + e[1] * e[1]
    w, rho = F(1), c2
    d = F(delta)
    if d > 0 and c2 > d * d:
        en = _fsqrt(c2)
        w, rho = d / en, 2 * d * en - d * d
    return e, jp, jq, w, rho


def _common(values):
    """(integers, common denominator) of a nested list of Fractions, as an int64 array."""
    flat = np.array(values, object)
    den = 1
    for v in flat.reshape(-1):
        den = den * v.denominator // math.gcd(den, v.denominator)
    ints = np.array([int(v * den) for v in flat.reshape(-1)], object)
    assert max((abs(v) for v in ints), default=0) < 2 ** 31
    return ints.astype(np.int64).reshape(flat.shape), den


_exact_cache = {}


def linearize_exact(sc, delta):
    """Every output of slam_bas_linearize_f64 on a scene, exactly: Hpl [O,18], Hll [L,6] and Hpp [K,21] packed, bl [L,3],
    bp [K,6], cost [K] as f64 arrays that hold the exact rationals (asserted), `total` the exact total cost (a Fraction),
    and `dmax`, the largest diagonal entry of the free poses' Hpp and of every Hll."""
    key = (sc["name"], float(delta))
    if key in _exact_cache:
        return _exact_cache[key]
    K, L, op, ol = sc["K"], sc["L"], sc["op"], sc["ol"]
    O = len(op)
    lin = [linearise_fraction(sc["T12"][op[o]], sc["X"][ol[o]], sc["meas"][o], sc["intr"], delta) for o in range(O)]
    e, de = _common([q[0] for q in lin])
    jp, dp_ = _common([q[1] for q in lin])
    jq, dq = _common([q[2] for q in lin])
    w, dw = _common([q[3] for q in lin])
    rho, dr = _common([q[4] for q in lin])
    big = int(np.abs(jp).max()) ** 2 * 2 * int(w.max()) * (int(np.bincount(op).max()) + 1)
    assert big < 2 ** 62, "the integer sums could overflow"
    pp = w[:, None, None] * np.einsum("oia,oic->oac", jp, jp)
    pl = w[:, None, None] * np.einsum("oia,oic->oac", jp, jq)
    ll = w[:, None, None] * np.einsum("oia,oic->oac", jq, jq)
    pe = w[:, None] * np.einsum("oia,oi->oa", jp, e)
    le = w[:, None] * np.einsum("oia,oi->oa", jq, e)
    Hpp, bp, Hll, bl, cost = (np.zeros(s, np.int64) for s in ((K, 6, 6), (K, 6), (L, 3, 3), (L, 3), (K,)))
    np.add.at(Hpp, op, pp)
    np.add.at(bp, op, pe)
    np.add.at(Hll, ol, ll)
    np.add.at(bl, ol, le)
    np.add.at(cost, op, rho)
    out = dict(Hpl=exact_f64(pl.reshape(O, 18), dw * dp_ * dq), Hpp=exact_f64(np.stack([Hpp[:, a, c] for a, c in TRI], 1), dw * dp_ * dp_),
               bp=exact_f64(bp, dw * dp_ * de), Hll=exact_f64(np.stack([Hll[:, a, c] for a, c in TRI3], 1), dw * dq * dq),
               bl=exact_f64(bl, dw * dq * de), cost=exact_f64(cost, dr), total=F(int(cost.sum()), dr),
               terms=dict(e=e, jp=jp, jq=jq, w=w, rho=rho, den=dict(e=de, jp=dp_, jq=dq, w=dw, rho=dr)), lin=lin)
    free = ~np.asarray(sc["fixed"], bool)
    dg = [TRI.index((a, a)) for a in range(6)]
    dg3 = [TRI3.index((a, a)) for a in range(3)]
    out["dmax_pose"], out["dmax_point"] = out["Hpp"][:, dg].max(1), out["Hll"][:, dg3].max(1)
    out["dmax"] = float(max(out["dmax_pose"][free].max(initial=0.0), out["dmax_point"].max(initial=0.0)))
    _exact_cache[key] = out
    return out


def linearise_f64(sc, delta):
    """ba_linearise restated in numpy f64, operation for operation (no contraction) -> per-observation terms as f64 arrays:
    Hpl [O,6,3], the terms of Hpp [O,6,6], bp [O,6], Hll [O,3,3], bl [O,3] and rho [O]."""
    fx, fy, cx, cy = sc["intr"]
    P, p, m = sc["T12"][sc["op"]], sc["X"][sc["ol"]], sc["meas"]
    X = P[:, 0] * p[:, 0] + P[:, 1] * p[:, 1] + P[:, 2] * p[:, 2] + P[:, 3]
    Y = P[:, 4] * p[:, 0] + P[:, 5] * p[:, 1] + P[:, 6] * p[:, 2] + P[:, 7]
    Z = P[:, 8] * p[:, 0] + P[:, 9] * p[:, 1] + P[:, 10] * p[:, 2] + P[:, 11]
    e0, e1 = m[:, 0] - (fx * X + cx * Z) / Z, m[:, 1] - (fy * Y + cy * Z) / Z
    zi = 1.0 / (Z + 1e-18)
    zi2 = zi * zi
    z = np.zeros_like(X)
    jp = np.array([[fx * X * Y * zi2, -fx - fx * X * X * zi2, fx * Y * zi, -fx * zi, z, fx * X * zi2],
                   [fy + fy * Y * Y * zi2, -fy * X * Y * zi2, -fy * X * zi, z, -fy * zi, fy * Y * zi2]]).transpose(2, 0, 1)
    a00, a02, a11, a12 = fx * zi, -fx * X * zi2, fy * zi, -fy * Y * zi2
    jq = np.array([[-(a00 * P[:, c] + a02 * P[:, 8 + c]) for c in range(3)], [-(a11 * P[:, 4 + c] + a12 * P[:, 8 + c]) for c in range(3)]]).transpose(2, 0, 1)
    c2 = e0 * e0 + e1 * e1
    w, rho = np.ones_like(c2), c2.copy()
    if delta > 0:
        en = np.sqrt(c2)
        out = en > delta
        w[out] = delta / en[out]
        rho[out] = 2.0 * delta * en[out] - delta * delta
    prod = lambda a, b: w[:, None, None] * (a[:, 0, :, None] * b[:, 0, None, :] + a[:, 1, :, None] * b[:, 1, None, :])
    vec = lambda a: w[:, None] * (a[:, 0] * e0[:, None] + a[:, 1] * e1[:, None])
    return dict(Hpl=prod(jp, jq), Hpp=prod(jp, jp), bp=vec(jp), Hll=prod(jq, jq), bl=vec(jq), rho=rho)


# ---- family (B): synthetic blocks ----------------------------------------------------------------------------------------
UNIMODULAR = np.array([[[2, 1, 0], [1, 1, 0], [0, 0, 1]], [[2, 0, 0], [0, 4, 0], [0, 0, 1]], [[1, 0, 0], [0, 2, 1], [0, 1, 1]],
                       [[2, 0, 1], [0, 1, 0], [1, 0, 1]], [[1, 1, 1], [1, 2, 1], [1, 1, 2]], [[1, 0, 0], [0, 2, 0], [0, 0, 2]],
                       [[1, 0, 0], [0, 1, 0], [0, 0, 1]], [[3, 1, 1], [1, 1, 0], [1, 0, 1]]], np.int64)
ESCALE = 8                                # every determinant of UNIMODULAR divides it


def adjugate(M):
    """(adjugate, determinant) of symmetric 3x3 integer matrices [n,3,3], by cofactors."""
    m = lambda i, j: M[:, i, j]
    c = np.empty_like(M)
    c[:, 0, 0], c[:, 0, 1], c[:, 0, 2] = m(1, 1) * m(2, 2) - m(1, 2) * m(1, 2), m(0, 2) * m(1, 2) - m(0, 1) * m(2, 2), m(0, 1) * m(1, 2) - m(0, 2) * m(1, 1)
    c[:, 1, 1], c[:, 1, 2], c[:, 2, 2] = m(0, 0) * m(2, 2) - m(0, 2) * m(0, 2), m(0, 1) * m(0, 2) - m(0, 0) * m(1, 2), m(0, 0) * m(1, 1) - m(0, 1) * m(0, 1)
    c[:, 1, 0], c[:, 2, 0], c[:, 2, 1] = c[:, 0, 1], c[:, 0, 2], c[:, 1, 2]
    return c, m(0, 0) * c[:, 0, 0] + m(0, 1) * c[:, 0, 1] + m(0, 2) * c[:, 0, 2]


def integer_blocks(K, L, op, ol, lam, seed):
    """Integer blocks on an observation list: Hpl [O,6,3], bl [L,3], bp [K,6], dp [K,6] (non-zero on EVERY pose) in [-3, 3],
    Hpp [K,6,6] symmetric in [-40, 40], M [L,3,3] drawn from UNIMODULAR and Hll = M - lam I (lam an integer), `seen` [L]."""
    rng = np.random.default_rng(seed)
    O = len(op)
    M = UNIMODULAR[rng.integers(0, len(UNIMODULAR), L)]
    Hpp = rng.integers(-40, 41, (K, 6, 6))
    Hpp = np.triu(Hpp) + np.triu(Hpp, 1).transpose(0, 2, 1)
    dp = rng.integers(1, 4, (K, 6)) * rng.choice([-1, 1], (K, 6))
    seen = np.zeros(L, bool)
    seen[ol] = True
    lam = int(lam)
    return dict(K=K, L=L, op=np.asarray(op), ol=np.asarray(ol), lam=lam, Hpl=rng.integers(-3, 4, (O, 6, 3)), bl=rng.integers(-3, 4, (L, 3)),
                bp=rng.integers(-3, 4, (K, 6)), dp=dp, Hpp=Hpp, M=M, Hll=M - lam * np.eye(3, dtype=np.int64), seen=seen)


def packed(H, tri):
    return np.stack([H[:, a, c] for a, c in tri], 1)


def reduce_exact(blk, cov):
    """slam_bas_reduce_f64 and slam_bas_backsub_f64 on integer blocks, exactly: E [L,9], Ebl [L,3], W [E,36] in the order of
    sorted(cov), Hdiag [K,36] (full), b [K,6], dl [L,3] as f64 arrays holding the exact rationals.  cov: brute_covisibility.
    dl uses dp of the observing pose AS GIVEN, fixed or not (the solver leaves dp of a fixed pose 0; the
    back-substitution does not look at the mask)."""
    K, L, op, ol, Hpl = blk["K"], blk["L"], blk["op"], blk["ol"], blk["Hpl"]
    adj, det = adjugate(blk["M"])
    assert (det > 0).all() and (ESCALE % det == 0).all()
    Es = adj * (ESCALE // det)[:, None, None]
    Es[~blk["seen"]] = 0
    keys = sorted(cov)
    W = np.zeros((len(keys), 6, 6), np.int64)
    for i, k in enumerate(keys):
        l, a, b = (np.array(v, np.int64) for v in zip(*cov[k]))
        assert (ol[a] == l).all() and (ol[b] == l).all()
        W[i] = -np.einsum("pab,pbc,pdc->ad", Hpl[a], Es[l], Hpl[b])
    Y = np.einsum("oab,obc->oac", Hpl, Es[ol])
    Ebl = np.einsum("lab,lb->la", Es, blk["bl"])
    Hdiag, b = ESCALE * blk["Hpp"].copy(), ESCALE * blk["bp"].copy()
    np.subtract.at(Hdiag, op, np.einsum("oac,odc->oad", Y, Hpl))
    np.subtract.at(b, op, np.einsum("oab,ob->oa", Hpl, Ebl[ol]))
    t = blk["bl"].copy()
    np.add.at(t, ol, np.einsum("oab,oa->ob", Hpl, blk["dp"][op]))
    dl = -np.einsum("lab,lb->la", Es, t)
    return dict(E=exact_f64(Es.reshape(L, 9), ESCALE), Ebl=exact_f64(Ebl, ESCALE), W=exact_f64(W.reshape(-1, 36), ESCALE),
                Hdiag=exact_f64(Hdiag.reshape(K, 36), ESCALE), b=exact_f64(b, ESCALE), dl=exact_f64(dl, ESCALE), keys=keys)


def inverse_fraction(M):
    """The inverse of one symmetric 3x3 integer matrix in Fractions, by cofactors."""
    adj, det = adjugate(np.asarray(M, np.int64)[None])
    return [[F(int(adj[0, i, j]), int(det[0])) for j in range(3)] for i in range(3)]


def edge_fraction(blk, pairs):
    """W of one edge from its pair list [(l, a, b), ..] in Fractions from end to end -> 6x6 list."""
    W = [[F(0)] * 6 for _ in range(6)]
    for l, a, b in pairs:
        E = inverse_fraction(blk["M"][l])
        for r in range(6):
            y = [sum(int(blk["Hpl"][a, r, i]) * E[i][c] for i in range(3)) for c in range(3)]
            for s in range(6):
                W[r][s] -= sum(y[c] * int(blk["Hpl"][b, s, c]) for c in range(3))
    return W


def point_step_fraction(blk, l):
    """dl of one point in Fractions from end to end (0 for a point nobody observes)."""
    obs = np.flatnonzero(blk["ol"] == l)
    if not len(obs):
        return [F(0)] * 3
    t = [F(int(v)) for v in blk["bl"][l]]
    for o in obs:
        for c in range(3):
            t[c] += sum(int(blk["Hpl"][o, a, c]) * int(blk["dp"][blk["op"][o], a]) for a in range(6))
    E = inverse_fraction(blk["M"][l])
    return [-sum(E[c][i] * t[i] for i in range(3)) for c in range(3)]


# ---- case 7: the candidate -----------------------------------------------------------------------------------------------
CANDIDATE_SHAPES = ((300, 262144 + 293), (300, 262144 - 300), (5, 250), (5, 251), (5, 252))      # K + L: past 1024 * 256, at it, 255, 256, 257
ROTATING = 4                                                                                   # free poses with a rotational dp


def candidate_case(K, L, rotating=True, seed=7):
    """Integer inputs of slam_bas_candidate_f64 at lambda = 2: poses of integers (axis permutations, integer translations),
    points, dp, dl, bp, bl integers; every third pose fixed (pose 0 too) WITH non-zero dp and bp; free poses have w = 0
    (a pure translation step); with `rotating`, the last ROTATING free ones have a dp of 0.5 .. 1.5 rad and a translation."""
    rng = np.random.default_rng(seed + K + L)
    T = np.zeros((K, 3, 4))
    T[:, :, :3] = np.array(_RZ + [_RCYC])[rng.integers(0, 5, K)]
    T[:, :, 3] = rng.integers(-9, 10, (K, 3))
    fixed = np.arange(K) % 3 == 0
    dp = (rng.integers(1, 4, (K, 6)) * rng.choice([-1, 1], (K, 6))).astype(np.float64)
    free = np.flatnonzero(~fixed)
    rot = free[-min(ROTATING, len(free) - 1):] if rotating else free[:0]
    dp[np.setdiff1d(free, rot), :3] = 0.0
    axis = rng.normal(size=(len(rot), 3))
    dp[rot, :3] = axis / np.linalg.norm(axis, axis=1)[:, None] * rng.uniform(0.5, 1.5, (len(rot), 1))
    dp[rot, 3:] = rng.uniform(-2, 2, (len(rot), 3))
    nz = lambda shape: (rng.integers(1, 4, shape) * rng.choice([-1, 1], shape)).astype(np.float64)
    return dict(K=K, L=L, lam=2.0, T=T.reshape(K, 12), X=rng.integers(-20, 21, (L, 3)).astype(np.float64), dp=dp, dl=nz((L, 3)),
                bp=nz((K, 6)), bl=rng.integers(-5, 6, (L, 3)).astype(np.float64), fixed=fixed, rot=rot)


def candidate_exact(c):
    """(T' [K,12] for the poses that do not rotate, X' [L,3], the denominator as a Python integer over the NON-rotating free
    poses and all points, the mask of those poses).  The rotating poses' terms are added by the caller in f64: they are no
    integers."""
    K = c["K"]
    plain = np.ones(K, bool)
    plain[c["rot"]] = False
    Tn = c["T"].reshape(K, 3, 4).copy()
    step = ~c["fixed"] & plain
    Tn[step, :, 3] += c["dp"][step, 3:]
    lam = int(c["lam"])
    dpi, bpi, dli, bli = (np.asarray(c[n]).astype(np.int64, copy=True) for n in ("dp", "bp", "dl", "bl"))
    den = int((dpi[step] * (lam * dpi[step] - bpi[step])).sum()) + int((dli * (lam * dli - bli)).sum())
    return Tn.reshape(K, 12), c["X"] + c["dl"], den, plain


def update_bound(d, T12):
    """A rounding bound per entry of T' = exp(d) T (ba_apply_update) for ONE evaluation, from d and T alone.  With th = |w|,
    a = sin th / th, b = (1 - cos th) / th^2, c = (th - sin th) / th^3: th^2 takes 5 roundings (all terms positive), th 3.5,
    sin and cos of it (th + 1) each in units of their value's scale 1; a then 10; 1 - cos th and th - sin th cancel, which
    multiplies what their operands carry by 1 / (1 - cos th) and th / (th - sin th): b takes 6 + 5 / (1 - cos th), c
    8 + 9 th / (th - sin th).  An entry of R = I + a W + b W^2 (W^2: 3 roundings) then carries
    eps (1 + (na + 2) |a W| + (nb + 5) |b W^2|), V likewise with b, c; T' = R T adds 3 roundings on sum |R| |T| and the
    translation V v 3 on sum |V| |v| and one for the final sum."""
    w, v = np.asarray(d[:3]), np.asarray(d[3:])
    th = float(np.linalg.norm(w))
    a, b, c = np.sin(th) / th, (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    na, nb, nc = 10.0, 6.0 + 5.0 / (1 - np.cos(th)), 8.0 + 9.0 * th / (th - np.sin(th))
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    aW, aW2 = np.abs(W), np.abs(W) @ np.abs(W)
    I = np.eye(3)
    Rm, Vm = I + a * aW + b * aW2, I + b * aW + c * aW2
    dR = R.EPS * (I + (na + 2) * a * aW + (nb + 5) * b * aW2)
    dV = R.EPS * (I + (nb + 2) * b * aW + (nc + 5) * c * aW2)
    T = np.abs(np.asarray(T12).reshape(3, 4))
    out = dR @ T + 3 * R.EPS * (Rm @ T)
    out[:, 3] += dV @ np.abs(v) + 3 * R.EPS * (Vm @ np.abs(v)) + R.EPS * (Rm @ T)[:, 3] + R.EPS * (Vm @ np.abs(v))
    return out.reshape(12)


# ---- case 3: the bound of the general comparison ----------------------------------------------------------------------------
def linearize_bound(T12, X, op, ol, meas, intr, delta):
    """Per entry of Hpl, Hll, bl, Hpp, bp and the per-pose cost: (terms + CHAIN_ROUNDINGS) * 2^-52 * sum of |terms| for ONE
    evaluation, from the terms alone (no condition number).  The terms are the summands: two products w J J per observation
    for an entry of Hpp, Hll, Hpl, two products w J e for bp and bl, the two squares of rho for the cost.

    This counts the residual e as a given number.  It is itself a difference m - u of a measurement and a projection of some
    hundred pixels each, and its cancellation is NOT in this bound; the 40 roundings of the chain have covered it on every
    scene so far (the two evaluations form u by the same expression).  `expanded` holds, for the record and never asserted,
    the bound with the terms of the expanded sum instead: w J m and w J u, and w |e| (|m| + |u|) beside rho."""
    from oracle import oracle

    T12 = np.ascontiguousarray(T12, np.float64).reshape(-1, 12)
    K, L = len(T12), len(X)
    e, Jp, Jq = oracle.reproj_rj_c(T12, X, op, ol, meas, *intr, with_point=True)
    s = np.sqrt((e * e).sum(1))
    out = (delta > 0) & (s > delta)
    w = np.where(out, delta / np.where(out, s, 1.0), 1.0)
    rho = np.where(out, 2.0 * delta * s - delta * delta, (e * e).sum(1))
    meas = np.asarray(meas, np.float64)
    mu = np.abs(meas) + np.abs(meas - e)                                                  # |m| + |u|, u = m - e
    aJp, aJq, ae = np.abs(Jp), np.abs(Jq), np.abs(e)
    wm, wv = w[:, None, None], w[:, None]
    nK, nL = np.bincount(op, minlength=K).astype(np.float64), np.bincount(ol, minlength=L).astype(np.float64)
    acc = lambda n, idx, t: (lambda z: (np.add.at(z, idx, t), z)[1])(np.zeros((n,) + t.shape[1:]))
    C = R.CHAIN_ROUNDINGS
    pose = lambda t: (2 * nK + C).reshape((K,) + (1,) * (t.ndim - 1)) * R.EPS * acc(K, op, t)
    point = lambda t: (2 * nL + C).reshape((L,) + (1,) * (t.ndim - 1)) * R.EPS * acc(L, ol, t)
    return dict(Hpl=(2 + C) * R.EPS * wm * np.einsum("oia,oic->oac", aJp, aJq), Hpp=pose(wm * np.einsum("oia,oic->oac", aJp, aJp)),
                Hll=point(wm * np.einsum("oia,oic->oac", aJq, aJq)), bp=pose(wv * np.einsum("oia,oi->oa", aJp, ae)),
                bl=point(wv * np.einsum("oia,oi->oa", aJq, ae)), cost=pose(rho),
                expanded=dict(bp=pose(wv * np.einsum("oia,oi->oa", aJp, mu)), bl=point(wv * np.einsum("oia,oi->oa", aJq, mu)),
                              cost=pose(rho + w * (ae * mu).sum(1))))


# ---- case 9: the problem embedded among strangers -------------------------------------------------------------------------
def embed(w, extra_poses=40, extra_points=500, seed=9):
    """The window w among extra poses and points that see only each other, relabelled so that every list keeps its order:
    the maps of poses, points and observations are increasing.  -> (the larger window, pose map, point map, observation map)."""
    rng = np.random.default_rng(seed)
    K, L, O = len(w["T0"]), len(w["X0"]), len(w["op"])
    K2, L2 = K + extra_poses, L + extra_points
    pm = np.sort(rng.choice(np.arange(1, K2), K - 1, replace=False))
    pm = np.r_[0, pm]                                            # pose 0 stays the fixed pose 0
    lm = np.sort(rng.choice(L2, L, replace=False))
    xp, xl = np.setdiff1d(np.arange(K2), pm), np.setdiff1d(np.arange(L2), lm)
    tracks = [tuple(rng.choice(xp, int(rng.integers(1, 5)), replace=False)) for _ in xl]
    T, X = R.scene(rng, K2, L2)
    ex = R.window(rng, T, X, np.array([k for t in tracks for k in t]), np.array([l for l, t in zip(xl, tracks) for _ in t]), w["fixed"])
    O2 = O + len(ex["op"])
    om = np.sort(rng.choice(O2, O, replace=False))
    xo = np.setdiff1d(np.arange(O2), om)
    op, ol, meas = np.zeros(O2, np.int32), np.zeros(O2, np.int32), np.zeros((O2, 2))
    op[om], ol[om], meas[om] = pm[w["op"]], lm[w["ol"]], w["meas"]
    op[xo], ol[xo], meas[xo] = ex["op"], ex["ol"], ex["meas"]
    T0, X0 = ex["T0"].copy(), ex["X0"].copy()
    T0[pm], X0[lm] = w["T0"], w["X0"]
    return dict(T0=T0, X0=X0, op=op, ol=ol, meas=meas, fixed=tuple(int(pm[k]) for k in w["fixed"])), pm, lm, om
