"""Homography estimation (slam_hg_*) on the CPU: the host twin of csrc/homography.hip (tests/hg_twin.py: the kernel file's own
routines compiled for the host) against the numpy statement in tests/homography_ref.py, which takes another route (SVD of the
8x9 DLT matrix, SVD of K^-1 H K, SVD triangulation, float sums), and against exact rational arithmetic.

Tolerances: a bound on a minimal solver's error depends on the conditioning of random samples and cannot be derived, so the
numpy solver's own worst value on the same samples is the yardstick (the NUMPY_WORST constants below, asserted on numpy alone)
and the twin is allowed 16 x it, the rule of DESIGN.md 4b.  Samples on which numpy's own normalised 8x9 system has
s7 / s0 < 1e-4 may be left out; the exclusion is capped at 1 % of the samples, asserted.

Measured here (tools/homography_edges.py, profiles/homography_edges.log; 2000 samples, 10 left out), numpy / twin: worst transfer
error of the sample points 3.4e-13 / 1.6e-12 px, |H - H_true| 1.28e-11 / 1.14e-11, | |H| - 1 | 2.2e-16 / 2.2e-16.  Exact
quadrilaterals: numpy 8.0e-14, twin 9.6e-16 relative.  True pose among the candidates of the twin's RANSAC winner (the log's
"test figure" lines): planar/fronto 3.0e-15 / 1.6e-15, planar/tilt60 1.29e-14 / 1.30e-14.  R_H: 0.500 on the planar and rotation scenes, 0.053 - 0.213 on the general ones,
0.423 / 0.438 on the noisy planar scenes (where no decision is asserted)."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import geometry_sources
import hg_twin as tw
import homography_ref as hr
import two_view_ref as ref
from exact_geometry import F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = ref.EUROC
S = 2000
FACTOR = 16.0
CAP = 0.01
ILL = 1e-4
RATIO = 0.45
# numpy's own worst values (measured, rounded up)
NUMPY_WORST = dict(transfer=3.5e-13, truth=1.3e-11, norm=2.3e-16)
NUMPY_EXACT = 8.5e-14           # numpy's SVD against the exact homography of the integer quadrilaterals, relative
NUMPY_POSE = 1.5e-14            # |[R|t] - truth| of numpy's nearest candidate on the planar scenes
PLANAR = ("planar/fronto", "planar/tilt60")
ROTATION = ("pure_rotation/t0", "pure_rotation/b1e-6", "pure_rotation/b1e-3")
GENERAL = ("general/clean", "forward/unit", "sideways/unit", "integer_pixels/rounded")


# ------------------------------------------------------------------------------------------------ the solver
@pytest.fixture(scope="module")
def samples():
    p1, p2, Ht = hr.fourpoint_samples(0, S)
    res = [hr.fourpoint(a, b) for a, b in zip(p1, p2)]
    return dict(p1=p1, p2=p2, Ht=Ht, H=np.array([r[0] for r in res]), ok=np.array([r[1] for r in res]),
                cond=np.array([r[2] for r in res]))


def _worst(H, keep, sm):
    q = dict(transfer=0.0, truth=0.0, norm=0.0)
    for s in np.flatnonzero(keep):
        q["transfer"] = max(q["transfer"], float(np.abs(hr.transfer(H[s], sm["p1"][s]) - sm["p2"][s]).max()))
        q["truth"] = max(q["truth"], hr.common_distance(H[s], sm["Ht"]))
        q["norm"] = max(q["norm"], abs(float(np.linalg.norm(H[s])) - 1))
    return q


def test_numpy_solver_yardsticks(samples):
    sm = samples
    keep = sm["ok"] & (sm["cond"] >= ILL)
    assert (~keep).mean() <= CAP, (~keep).sum()
    q = _worst(sm["H"], keep, sm)
    print("numpy:", q, "left out", int((~keep).sum()))
    for k, v in NUMPY_WORST.items():
        assert q[k] <= v, (k, q[k], v)


def test_twin_solver_within_16x_of_the_numpy_solver(samples):
    sm = samples
    H, ok = tw.fourpoint(sm["p1"], sm["p2"])
    keep = sm["ok"] & (sm["cond"] >= ILL)
    assert np.isfinite(H).all() and np.array_equal(ok != 0, sm["ok"])
    q = _worst(H, keep, sm)
    print("twin:", q)
    for k, v in NUMPY_WORST.items():
        assert q[k] <= FACTOR * v, (k, q[k], v)
    w = np.einsum("sk,spk->sp", H[:, 6:8], sm["p1"]) + H[:, 8:9]             # the sign rule: positive weights at the sample
    assert (w[ok != 0] > 0).all()
    perm = [2, 0, 3, 1]                                                     # H does not depend on the order of the correspondences
    Hp, okp = tw.fourpoint(sm["p1"][:200, perm], sm["p2"][:200, perm])
    assert np.array_equal(okp, ok[:200]) and max(hr.common_distance(a, b) for a, b in zip(Hp, H[:200])) < FACTOR * NUMPY_WORST["truth"]


def _exact_null_vector(rows):
    """The null vector of an 8x9 system of Fractions by Gauss-Jordan elimination (any non-zero pivot), exact."""
    A = [list(r) for r in rows]
    piv, r = [], 0
    for c in range(9):
        k = next((i for i in range(r, 8) if A[i][c] != 0), None)
        if k is None:
            continue
        A[r], A[k] = A[k], A[r]
        A[r] = [v / A[r][c] for v in A[r]]
        for i in range(8):
            if i != r and A[i][c] != 0:
                A[i] = [a - A[i][c] * b for a, b in zip(A[i], A[r])]
        piv.append(c)
        r += 1
    assert r == 8
    free = next(c for c in range(9) if c not in piv)
    h = [Fraction(0)] * 9
    h[free] = Fraction(1)
    for i, c in enumerate(piv):
        h[c] = -A[i][free]
    return h


QUADS = [
    ([(100, 100), (600, 120), (580, 400), (90, 380)], [(120, 90), (610, 140), (560, 420), (110, 360)]),
    ([(10, 20), (700, 35), (650, 460), (40, 300)], [(300, 100), (500, 90), (640, 400), (200, 470)]),     # strong perspective
    ([(0, 0), (751, 0), (751, 479), (0, 479)], [(0, 0), (751, 0), (751, 479), (0, 479)]),                # the identity: h1 = h3 = 0 ...
    ([(5, 7), (405, 7), (405, 307), (5, 307)], [(307, 5), (307, 405), (7, 405), (7, 5)]),                # ... a quarter turn: h0 = h4 = 0
    ([(100, 200), (300, 100), (500, 300), (250, 400)], [(0, 10), (200, -90), (400, 110), (150, 210)]),   # a translation, off image
]


def test_exact_integer_quadrilaterals_third_route():
    worst_np = worst_tw = 0.0
    for q1, q2 in QUADS:
        rows = []
        for (x, y), (u, v) in zip(q1, q2):
            x, y, u, v = F(x), F(y), F(u), F(v)
            rows.append([-x, -y, F(-1), F(0), F(0), F(0), u * x, u * y, u])
            rows.append([F(0), F(0), F(0), -x, -y, F(-1), v * x, v * y, v])
        h = _exact_null_vector(rows)
        big = max(abs(v) for v in h)
        He = np.array([float(v / big) for v in h])
        He /= np.linalg.norm(He)
        p1, p2 = np.array(q1, float), np.array(q2, float)
        Hn, okn, _ = hr.fourpoint(p1, p2)
        Ht, okt = tw.fourpoint(p1, p2)
        assert okn and okt[0]
        worst_np = max(worst_np, hr.common_distance(Hn, He))
        worst_tw = max(worst_tw, hr.common_distance(Ht[0], He))
    print(f"exact quadrilaterals: numpy {worst_np:.2e} twin {worst_tw:.2e}")
    assert worst_np <= NUMPY_EXACT and worst_tw <= FACTOR * NUMPY_EXACT


# ------------------------------------------------------------------------------------------------ RANSAC
def test_draws_are_the_stated_generator():
    for seed, h, n in ((0, 0, 4), (0, 5, 4), (7, 255, 200), (2 ** 63 + 5, 1 << 19, 5), (1, 17, 1 << 20)):
        idx = hr.draw_sample(seed, h, n)
        assert idx == tw.draw_sample(seed, h, n) and len(set(idx)) == 4 and all(0 <= i < n for i in idx)
        assert n < 5 or idx == ref.draw_sample(seed, 0, h, n)[:4]           # the first four of the essential matrix's five draws
    assert hr.draw_sample(3, 9, 200)[0] == ((ref.draw_word(3, 9, 0) >> 32) * 200) >> 32


@pytest.fixture(scope="module")
def scenes():
    from oracle import oracle

    out = {}
    for name, sc in hr.family_scenes() + [(f"planar_noisy/{s['variant']}", s) for s in hr.scenes_planar_noisy()]:
        H, mask, st, counts = tw.ransac(sc["px1"], sc["px2"], 256, 3.0, 0, with_counts=True)
        E = oracle.tv_twin_ransac(sc["px1"], sc["px2"], sc["K"], 256, 1.0, 0)[0]
        out[name] = dict(sc=sc, H=H, mask=mask, st=st, counts=counts, E=E, dec=tw.decompose(sc["px1"], sc["px2"], sc["K"], H, mask),
                         score=tw.model_score(sc["px1"], sc["px2"], sc["K"], H, E))
    return out


@pytest.mark.parametrize("name", ["planar/fronto", "planar/tilt60", "pure_rotation/t0", "general/clean"])
def test_mask_is_the_stated_formula_and_the_winner_the_numpy_ransac_winner(scenes, name):
    s = scenes[name]
    sc = s["sc"]
    assert np.array_equal(s["mask"], hr.inlier_mask(s["H"], sc["px1"], sc["px2"], 3.0)) and s["st"][0] == s["mask"].sum()
    assert np.array_equal(s["mask"], tw.inlier(s["H"], sc["px1"], sc["px2"], 3.0))
    has = s["counts"] >= 0
    assert s["st"][3] == has.sum() and s["st"][0] == s["counts"].max() and s["st"][1] == int(np.argmax(s["counts"])) and s["st"][2] == 0
    Hn, mn, stn = hr.ransac(sc["px1"], sc["px2"], 256, 3.0, 0)
    print(name, "numpy", stn, "twin", s["st"])
    assert stn[0] == s["st"][0] and stn[1] == s["st"][1] and stn[3] == s["st"][3]
    assert abs(np.linalg.norm(s["H"]) - 1) < 1e-15 and hr.common_distance(Hn, s["H"]) < 1e-12
    if name != "general/clean":
        assert s["st"][0] == 200 and s["st"][1] == 0                        # noise-free: every match, already under hypothesis 0


# ------------------------------------------------------------------------------------------------ the decomposition
def _nearest(pose_all, sc):
    return min(float(np.linalg.norm(P - np.c_[sc["R"], sc["t"]])) for P in pose_all)


def _orthonormal(pose_all):
    for P in pose_all:
        R = P[:, :3]
        assert np.isfinite(P).all() and np.abs(R.T @ R - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(R) - 1) < 1e-14
        assert abs(np.linalg.norm(P[:, 3]) - 1) < 1e-14


@pytest.mark.parametrize("name", PLANAR)
def test_true_pose_is_among_the_candidates_on_the_planar_scenes(scenes, name):
    s = scenes[name]
    sc, d = s["sc"], s["dec"]
    n = hr.decompose(s["H"], sc["K"], sc["px1"], sc["px2"], s["mask"])
    en, et = _nearest(n["pose_all"], sc), _nearest(d["pose_all"], sc)
    print(name, "nearest candidate numpy", en, "twin", et, "votes", d["count"], "stats", d["stats"])
    assert en <= NUMPY_POSE and et <= FACTOR * NUMPY_POSE
    _orthonormal(d["pose_all"])
    assert np.array_equal(d["count"], n["count"]) and np.array_equal(d["stats"], n["stats"]) and np.array_equal(d["good"], n["good"])
    assert np.abs(d["pose_all"] - n["pose_all"]).max() < FACTOR * NUMPY_POSE and np.abs(d["normal_all"] - n["normal_all"]).max() < FACTOR * NUMPY_POSE
    assert np.allclose(d["sv"], n["sv"], rtol=1e-13, atol=0)
    # the order stated in the header: (Ra, ta, na), (Ra, -ta, -na), (Rb, tb, nb), (Rb, -tb, -nb); na, nb with the largest component positive
    P, N = d["pose_all"], d["normal_all"]
    assert np.array_equal(P[0, :, :3], P[1, :, :3]) and np.array_equal(P[2, :, :3], P[3, :, :3])
    assert np.array_equal(P[0, :, 3], -P[1, :, 3]) and np.array_equal(N[0], -N[1]) and np.array_equal(N[2], -N[3])
    assert N[0][np.argmax(np.abs(N[0]))] > 0 and N[2][np.argmax(np.abs(N[2]))] > 0
    # every candidate explains the homography: Hs = R + |T| t n^T with Hs = Hn / s2 (sign as voted)
    Hs = hr.normalised_homography(s["H"], sc["K"]) / d["sv"][1]
    for k in range(4):
        T = (Hs - P[k, :, :3]) @ N[k]
        assert np.abs(Hs - P[k, :, :3] - np.outer(T, N[k])).max() < 1e-12 and np.linalg.norm(np.cross(T, P[k, :, 3])) < 1e-12
    nrm, _ = sc["plane"]
    assert min(np.linalg.norm(N[k] - nrm) for k in range(4)) < 1e-12          # the true plane normal is among them
    if name == "planar/tilt60":
        assert d["stats"].tolist() == [200, 2, 94, 4] and et == float(np.linalg.norm(d["pose"] - np.c_[sc["R"], sc["t"]]))       # a unique winner: the truth
    else:
        assert d["stats"][0] == 200 and d["stats"][2] == 200 and d["stats"][3] == 4        # the two-fold ambiguity, reported
        other = [k for k in range(4) if d["count"][k] == 200]
        assert len(other) == 2
        ang = [ref.rotation_angle_deg(P[k, :, :3], sc["R"]) for k in other]
        print("fronto: the two tied candidates are", ang, "degrees from the true rotation")
        assert min(ang) < 1e-10 and 1.0 < max(ang) < 20.0


def test_pure_rotation_is_reported_as_rotation_only(scenes):
    s = scenes["pure_rotation/t0"]
    sc, d = s["sc"], s["dec"]
    n = hr.decompose(s["H"], sc["K"], sc["px1"], sc["px2"], s["mask"])
    spread = (d["sv"][0] - d["sv"][2]) / d["sv"][1]
    near = scenes["pure_rotation/b1e-6"]["dec"]
    spread_near = (near["sv"][0] - near["sv"][2]) / near["sv"][1]
    print("spread t0", spread, "numpy", n["spread"], "b1e-6", spread_near)
    assert spread < hr.ROTATION_ONLY / 1e3 and n["spread"] < hr.ROTATION_ONLY / 1e3 and spread_near > hr.ROTATION_ONLY * 1e2
    assert d["stats"].tolist() == [0, -2, 0, 1] and n["stats"].tolist() == [0, -2, 0, 1]
    R = d["pose"][:, :3]
    assert np.linalg.norm(R - sc["R"]) < FACTOR * 2e-15 and np.linalg.norm(n["pose"][:, :3] - sc["R"]) < 2e-15
    assert np.abs(R.T @ R - np.eye(3)).max() < 1e-15 and not d["pose"][:, 3].any()
    assert np.array_equal(d["pose_all"][0], d["pose"]) and not d["pose_all"][1:].any() and not d["normal_all"].any()
    assert not d["count"].any() and not d["good"].any()
    assert near["stats"][1] >= 0 and near["stats"][3] == 4                  # a baseline of 1e-6 depths is not a rotation
    # -H decomposes alike: the sign comes from the matches
    d2 = tw.decompose(sc["px1"], sc["px2"], sc["K"], -s["H"], s["mask"])
    assert np.array_equal(d2["pose"], d["pose"])


@pytest.mark.parametrize("name", GENERAL + ROTATION[1:] + ("planar_noisy/fronto", "planar_noisy/tilt60"))
def test_other_scenes_give_some_finite_orthonormal_answer_and_numpy_counts(scenes, name):
    s = scenes[name]
    sc, d = s["sc"], s["dec"]
    assert d["stats"][3] == 4 and d["stats"][1] in (0, 1, 2, 3)
    _orthonormal(d["pose_all"])
    n = hr.decompose(s["H"], sc["K"], sc["px1"], sc["px2"], s["mask"])
    assert np.array_equal(d["count"], n["count"]) and np.array_equal(d["stats"], n["stats"])
    assert d["stats"][0] == d["count"].max() == d["good"].sum() and not d["good"][~s["mask"]].any()
    assert np.array_equal(d["pose"], d["pose_all"][d["stats"][1]])


def test_private_copies_match_two_view_vote(scenes):
    """The vote is defined as 'triangulated as slam_tv_triangulate_f64': homography.hip's vote gives the bits of two_view.hip's
    routines (its host twin), and there are no private copies left to drift apart - the Jacobi sweeps, the triangulation and
    the cheirality test (with the sampler and the range clamp) are defined once, in csrc/geometry_common.h, and in none of the
    four kernel files."""
    from oracle import oracle

    s = scenes["general/clean"]
    sc, d = s["sc"], s["dec"]
    x1, x2 = ref.normalise(sc["px1"], sc["K"]), ref.normalise(sc["px2"], sc["K"])
    for k in range(4):
        good = oracle.tv_twin_cheirality(d["pose_all"][k][:, :3], d["pose_all"][k][:, 3], x1, x2, 50.0)
        assert (good & s["mask"]).sum() == d["count"][k]
    geometry_sources.assert_one_copy()


# ------------------------------------------------------------------------------------------------ the scores
def test_scores_are_numpys_fixed_point_sums_and_decide_where_the_margin_allows(scenes):
    for name, s in scenes.items():
        sc = s["sc"]
        score, ratio = s["score"]
        sh, se = hr.fixed_point_scores(s["H"], s["E"], sc["K"], sc["px1"], sc["px2"])      # elementwise, in the header's order
        fh, fe, fr = hr.model_scores(s["H"], s["E"], sc["K"], sc["px1"], sc["px2"])
        print(f"{name:28s} S_H {score[0]} S_E {score[1]} R_H {ratio:.4f} | numpy fixed {sh} {se} float {fh:.3f} {fe:.3f} {fr:.4f}")
        assert (int(score[0]), int(score[1])) == (sh, se), name
        assert ratio == (score[0] / (score[0] + score[1]) if score[0] + score[1] else 0.0)
        assert abs(score[0] / hr.FIXED - fh) < 1e-3 and abs(score[1] / hr.FIXED - fe) < 1e-3 and abs(ratio - fr) < 1e-6
        if abs(fr - RATIO) >= 0.05:                                         # the decision only where numpy's ratio is clear of 0.45
            assert (ratio > RATIO) == (fr > RATIO)
    for name in PLANAR + ROTATION[:2]:
        assert abs(scenes[name]["score"][1] - 0.5) < 1e-3 and scenes[name]["score"][1] > RATIO, name
    for name in GENERAL:
        assert scenes[name]["score"][1] < 0.25, name
    for name in ("planar_noisy/fronto", "planar_noisy/tilt60"):             # the value only: 0.42 - 0.44 straddles any threshold near 0.45
        assert 0.3 < scenes[name]["score"][1] < 0.6


def test_scores_exact_integers_in_the_headers_order():
    """The fixed-point rule restated operation by operation in Python floats (IEEE doubles, no fused operations): equal integers."""
    s = hr.scenes_planar_noisy()[1]
    H = tw.ransac(s["px1"], s["px2"], 64, 3.0, 0)[0]
    E = ref.essential_from_pose(s["R"], s["t"])
    fx, fy, cx, cy = K
    h = [float(v) for v in H]
    a = [h[4] * h[8] - h[5] * h[7], h[2] * h[7] - h[1] * h[8], h[1] * h[5] - h[2] * h[4], h[5] * h[6] - h[3] * h[8], h[0] * h[8] - h[2] * h[6],
         h[2] * h[3] - h[0] * h[5], h[3] * h[7] - h[4] * h[6], h[1] * h[6] - h[0] * h[7], h[0] * h[4] - h[1] * h[3]]
    A = [0.0] * 9
    f = [0.0] * 9
    for i in range(3):
        A[3 * i], A[3 * i + 1] = float(E[3 * i]) / fx, float(E[3 * i + 1]) / fy
        A[3 * i + 2] = float(E[3 * i + 2]) - (cx * A[3 * i] + cy * A[3 * i + 1])
    for j in range(3):
        f[j], f[3 + j] = A[j] / fx, A[3 + j] / fy
        f[6 + j] = A[6 + j] - (cx * f[j] + cy * f[3 + j])

    def tr(m, x, y, u, v):
        w = (m[6] * x + m[7] * y) + m[8]
        du, dv = ((m[0] * x + m[1] * y) + m[2]) / w - u, ((m[3] * x + m[4] * y) + m[5]) / w - v
        return du * du + dv * dv

    def term(c, gate):
        return int((5.991 - c) * 1048576.0) if c < gate else 0

    sh = se = 0
    for (x, y), (u, v) in zip(s["px1"].tolist(), s["px2"].tolist()):
        sh += term(tr(h, x, y, u, v) / 1.0, 5.991) + term(tr(a, u, v, x, y) / 1.0, 5.991)
        l0, l1, l2 = (f[0] * x + f[1] * y) + f[2], (f[3] * x + f[4] * y) + f[5], (f[6] * x + f[7] * y) + f[8]
        m0, m1 = (f[0] * u + f[3] * v) + f[6], (f[1] * u + f[4] * v) + f[7]
        r = (u * l0 + v * l1) + l2
        se += term((r * r / (l0 * l0 + l1 * l1)) / 1.0, 3.841) + term((r * r / (m0 * m0 + m1 * m1)) / 1.0, 3.841)
    score, ratio = tw.model_score(s["px1"], s["px2"], K, H, E)
    assert (int(score[0]), int(score[1])) == (sh, se) and sh > 0 and se > 0 and ratio == sh / (sh + se)


# ------------------------------------------------------------------------------------------------ edge cases
# A bad offsets table is not among the cases below: the offsets are read by the kernels alone (hg_range clamps a pair's slice
# into [0, M) and counts it), the twin's entries take one pair at a time and have no table.  That case is
# tests/test_homography_gpu.py::test_bad_offsets_never_leave_the_arrays_and_are_counted, which asks for the twin's result on the
# clamped slices; what Python refuses before the device (no entries, too many pairs) is in the bindings test at the end.
def _sample(kind):
    p1 = np.array([[100.0, 100], [600, 120], [580, 400], [90, 380]])
    p2 = np.array([[120.0, 90], [610, 140], [560, 420], [110, 360]])
    if kind == "duplicate":
        p1[2] = p1[0]
    elif kind == "duplicate2":
        p2[3] = p2[1]
    elif kind == "collinear":
        p1[2] = 0.5 * (p1[0] + p1[1])
    elif kind == "collinear2":
        p2[:, 1] = 3.0 * p2[:, 0] + 1.0
    elif kind == "flip":
        p2[[0, 1]] = p2[[1, 0]]
    elif kind == "nan":
        p1[1, 0] = np.nan
    elif kind == "inf":
        p2[3, 1] = -np.inf
    elif kind == "huge":
        p1[0] = [1e150, -1e150]
    elif kind == "all_equal":
        p1[:] = p1[0]
    return p1, p2


EDGE_SAMPLES = ("duplicate", "duplicate2", "collinear", "collinear2", "flip", "nan", "inf", "huge", "all_equal")


def test_solver_edge_samples_give_no_model():
    for kind in EDGE_SAMPLES:
        p1, p2 = _sample(kind)
        H, ok = tw.fourpoint(p1, p2)
        assert ok[0] == 0 and not H.any(), kind
        assert not hr.sample_ok(p1, p2), kind
    H, ok = tw.fourpoint(*_sample("fine"))
    assert ok[0] == 1 and abs(np.linalg.norm(H) - 1) < 1e-15
    big = tw.fourpoint(_sample("fine")[0] * 1e90, _sample("fine")[1] * 1e-90)      # inside the range: solved, finite
    assert big[1][0] == 1 and np.isfinite(big[0]).all()


def _edge_scenes():
    fam = {f"{s['family']}/{s['variant']}": s for f in ("duplicates", "collinear", "non_finite", "off_image") for s in ref.FAMILIES[f]()}
    return fam


def test_ransac_and_decomposition_edge_scenes():
    for name, sc in _edge_scenes().items():
        H, mask, st, counts = tw.ransac(sc["px1"], sc["px2"], 64, 3.0, 0, with_counts=True)
        d = tw.decompose(sc["px1"], sc["px2"], sc["K"], H, mask)
        score, ratio = tw.model_score(sc["px1"], sc["px2"], sc["K"], H, sc["E"])
        print(name, st, d["stats"], score, ratio)
        assert (int(score[0]), int(score[1])) == hr.fixed_point_scores(H, sc["E"], sc["K"], sc["px1"], sc["px2"]), name
        assert np.isfinite(H).all() and np.isfinite(d["pose_all"]).all() and np.isfinite(d["pose"]).all() and np.isfinite(ratio)
        assert st[0] == mask.sum() and st[3] == (counts >= 0).sum()
        if name in ("duplicates/1distinct", "collinear/both", "collinear/frame1"):
            assert st.tolist() == [0, -1, -1, 0] and not H.any() and not mask.any()        # no sample is in general position
            assert d["stats"].tolist() == [0, -1, 0, 0] and np.array_equal(d["pose"], np.eye(3, 4)) and not d["sv"].any()
            assert score[0] == 0
        if "bad" in sc and len(sc["bad"]):
            assert not mask[sc["bad"]].any() and not d["good"][sc["bad"]].any()            # a non-finite / far match is never an inlier
            assert st[1] >= 0
    sc = ref.scenes_planar()[1]
    for n in (0, 3):
        H, mask, st = tw.ransac(sc["px1"][:n], sc["px2"][:n], 64, 3.0, 0)
        assert st.tolist() == [0, -1, -1, 0] and not H.any() and len(mask) == n and not mask.any()
        d = tw.decompose(sc["px1"][:n], sc["px2"][:n], K, H)
        assert d["stats"].tolist() == [0, -1, 0, 0] and np.array_equal(d["pose"], np.eye(3, 4))
        assert tw.model_score(sc["px1"][:n], sc["px2"][:n], K, H, sc["E"])[0][0] == 0           # H = 0 scores nothing
    H, mask, st = tw.ransac(sc["px1"][:4], sc["px2"][:4], 64, 3.0, 0)
    assert st[0] == 4 and st[1] == 0 and mask.all() and st[3] == 64
    for bad in (np.full(9, np.nan), np.zeros(9), np.full(9, 1e200), np.full(9, 1e-200), np.r_[1.0, np.zeros(8)]):       # the last: rank 1
        d = tw.decompose(sc["px1"], sc["px2"], K, bad)
        assert d["stats"].tolist() == [0, -1, 0, 0] and np.array_equal(d["pose"], np.eye(3, 4)) and not d["pose_all"].any(), bad
    sh = tw.model_score(sc["px1"], sc["px2"], K, np.full(9, np.nan), np.full(9, np.nan))
    assert sh[0].tolist() == [0, 0] and sh[1] == 0.0                       # NaN terms contribute nothing


# ------------------------------------------------------------------------------------------------ the sanitized program
def test_sanitized_program_runs_the_same_jobs_clean_and_gives_the_same_bytes(samples, scenes):
    p1 = np.concatenate([samples["p1"][:500]] + [_sample(k)[0][None] for k in EDGE_SAMPLES])
    p2 = np.concatenate([samples["p2"][:500]] + [_sample(k)[1][None] for k in EDGE_SAMPLES])
    H, ok = tw.fourpoint(p1, p2)
    Hs, oks = tw.san_fourpoint(p1, p2)
    assert np.array_equal(ok, oks) and np.array_equal(H.view(np.uint64), Hs.view(np.uint64))
    jobs = [(n, s["sc"], s["E"]) for n, s in scenes.items() if n in ("planar/fronto", "pure_rotation/t0", "general/clean", "planar_noisy/tilt60")]
    jobs += [(n, sc, sc["E"]) for n, sc in _edge_scenes().items()]
    empty = dict(px1=np.zeros((0, 2)), px2=np.zeros((0, 2)), K=K)
    jobs += [("empty", empty, np.zeros(9))]
    for name, sc, E in jobs:
        r = tw.san_pair(sc["px1"], sc["px2"], sc["K"], 64, 3.0, 0, E)
        H, mask, st = tw.ransac(sc["px1"], sc["px2"], 64, 3.0, 0)
        d = tw.decompose(sc["px1"], sc["px2"], sc["K"], H, mask)
        score, ratio = tw.model_score(sc["px1"], sc["px2"], sc["K"], H, E)
        assert np.array_equal(r["H"].view(np.uint64), H.view(np.uint64)) and np.array_equal(r["mask"], mask) and np.array_equal(r["stats"], st), name
        for k in ("pose_all", "normal_all", "pose", "sv"):
            assert np.array_equal(r[k].view(np.uint64), d[k].view(np.uint64)), (name, k)
        assert np.array_equal(r["count"], d["count"]) and np.array_equal(r["dstats"], d["stats"]) and np.array_equal(r["good"], d["good"]), name
        assert np.array_equal(r["score"], score) and np.float64(r["ratio"]).view(np.uint64) == np.float64(ratio).view(np.uint64), name


# ------------------------------------------------------------------------------------------------ the bindings
def test_python_arguments_are_checked_before_anything_reaches_the_device(built):
    import slamhip
    from slamhip import homography as hg

    sc = ref.scenes_planar()[0]
    a, b = sc["px1"], sc["px2"]
    bad = [
        lambda: slamhip.fourpoint_homography_arrays(np.zeros((3, 5, 2)), np.zeros((3, 5, 2))),
        lambda: slamhip.fourpoint_homography_arrays(np.zeros((3, 4, 2)), np.zeros((2, 4, 2))),
        lambda: slamhip.find_homography_arrays(a, b[:-1]),
        lambda: slamhip.find_homography_arrays(a[:, :1], b),
        lambda: slamhip.find_homography_arrays(a, b, hypotheses=0),
        lambda: slamhip.find_homography_arrays(a, b, hypotheses=(1 << 20) + 1),
        lambda: slamhip.find_homography_arrays(a, b, threshold=0.0),
        lambda: slamhip.find_homography_arrays(a, b, threshold=np.nan),
        lambda: slamhip.find_homography_offsets(a, b, []),
        lambda: slamhip.find_homography_offsets(a, b, np.zeros(65537 + 1, np.int32)),
        lambda: slamhip.find_homography_batch([(a, b, a)]),
        lambda: slamhip.decompose_homography_arrays(np.eye(3), a, b, (1.0, 2.0, 3.0)),
        lambda: slamhip.decompose_homography_arrays(np.eye(3), a, b, (-1.0, 2.0, 3.0, 4.0)),
        lambda: slamhip.decompose_homography_arrays(np.eye(3), a, b, K, distance_thresh=0.0),
        lambda: slamhip.decompose_homography_arrays(np.eye(3), a, b, K, inlier=np.ones(3)),
        lambda: slamhip.decompose_homography_offsets(np.zeros((2, 9)), a, b, [0, len(a)], K),
        lambda: slamhip.decompose_homography_batch(np.zeros((1, 9)), [(a, b)], K, inliers=[]),
        lambda: slamhip.model_scores_offsets(np.zeros(9), np.zeros(8), a, b, [0, len(a)], K),
        lambda: slamhip.model_scores_offsets(np.zeros(9), np.zeros(9), a, b, [0, len(a)], K, sigma=0.0),
        lambda: slamhip.model_scores_offsets(np.zeros(9), np.zeros(9), a, b, [0, len(a)], K, sigma=1e-170),
        lambda: slamhip.estimate_two_view_auto(a, b, K, ratio=1.5),
        lambda: slamhip.estimate_two_view_auto(a, b, K, threshold_h=-1.0),
        lambda: slamhip.estimate_two_view_auto(a, b, K, ambiguity=0.0),
        lambda: slamhip.estimate_two_view_auto(a, b[:5], K),
        lambda: slamhip.verify_pairs_auto([(a, b)], np.eye(2)),
    ]
    for i, fn in enumerate(bad):
        with pytest.raises(ValueError):
            fn()
        assert i >= 0
    with pytest.raises(TypeError):
        slamhip.find_homography_arrays(a, b, hypotheses=2.5)
    with pytest.raises(TypeError):
        slamhip.estimate_two_view_auto(a, b, K, seed="x")
    # nothing to do: answered on the host
    assert slamhip.fourpoint_homography_arrays(np.zeros((0, 4, 2)), np.zeros((0, 4, 2)))[0].shape == (0, 3, 3)
    assert slamhip.find_homography_batch([])[0].shape == (0, 3, 3) and slamhip.verify_pairs_auto([], K) == []
    assert slamhip.model_scores_offsets(np.zeros(0), np.zeros(0), a, b, [0], K)[0].shape == (0, 2)
    assert hg.DEFAULT_THRESHOLD_H == 3.0 and hg.DEFAULT_RATIO == 0.45 and hg.DEFAULT_AMBIGUITY == 0.75


def test_abi_table_header_and_kernel_file_agree(built):
    from slamhip import _lib

    header = open(os.path.join(ROOT, "include", "slamhip.h")).read()
    src = open(os.path.join(ROOT, "slam-experiments_amd", "csrc", "homography.hip")).read()
    names = sorted(n for n in _lib.SIGNATURES if n.startswith("slam_hg_"))
    assert names == ["slam_hg_decompose_f64", "slam_hg_fourpoint_f64", "slam_hg_model_score_f64", "slam_hg_ransac_f64"]
    ctype = {"slam_ctx*": "c_void_p", "int64_t": "c_long", "int": "c_int", "double": "c_double", "uint64_t": "c_ulong"}
    for n in names:
        decl = re.search(r"SLAM_API int %s\((.*?)\);" % n, header, re.S).group(1)
        impl = re.search(r'extern "C" int %s\((.*?)\) \{' % n, src, re.S).group(1)
        norm = [re.sub(r"\s+", " ", d).strip() for d in (decl, impl)]
        assert norm[0] == norm[1], n
        args = [a.strip() for a in norm[0].split(",")]
        restype, argtypes = _lib.SIGNATURES[n]
        assert restype.__name__ == "c_int" and len(args) == len(argtypes), n
        for a, t in zip(args, argtypes):
            base = a.rsplit(" ", 1)[0].replace("const ", "")
            want = "c_void_p" if base.endswith("*") else ctype[base]
            assert t.__name__ == want, (n, a, t.__name__)
    assert "#pragma clang fp contract(off)" in src and "HG_HOST_ONLY" in src
    assert "#pragma clang fp contract(off)" in geometry_sources.HEADER
    for word in ("acos", "atan", "cbrt", "pow(", "exp(", "log(", "fma("):      # + - * / sqrt only, in the file and in the header it includes
        assert word not in re.sub(r"//[^\n]*", "", src + geometry_sources.HEADER), word
    lib = _lib.load()
    for n in names:
        assert hasattr(lib, n)
    mk = open(os.path.join(ROOT, "slam-experiments_amd", "csrc", "Makefile")).read()
    assert "homography.hip" in mk
