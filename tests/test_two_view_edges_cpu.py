"""Two-view geometry at its edges, without a device: the host twin of csrc/two_view.hip (oracle/two_view_twin.cpp - the
kernel file's own routines compiled for the host with contraction off) on the scene families of tests/two_view_ref.py,
once more through the same code under the undefined-behaviour and address sanitizers, and the exact-mask / exact-argmax
checks of tests/test_two_view_edges_gpu.py proven on the twin's sequential RANSAC before a device sees them.

Yardsticks: the numpy solver's own worst values per family (FAMILY_WORST of tests/test_two_view_cpu.py, asserted there on
numpy alone); the kernel's arithmetic is allowed FACTOR = 16 over them.  A sample is left out of a comparison only where
numpy's own completeness is above ILL_CONDITIONED or its own roots are closer than DOUBLE_ROOT, at most CAP of a family.
The numpy solver is only given samples whose coordinates are finite and below 1e100: LAPACK does not return on others.

FOUND BY THIS FILE and fixed in csrc/two_view.hip (figures of the host twin before the fix, 4 seeds x 256 draws):
  test_true_matrix_is_among_the_roots[sideways]  R = I, t along x.  On 7 % of the samples the true E had no component
      along the fourth vector of the Householder null-space basis; the solver fixes that component to 1, the degree-10
      polynomial lost its leading coefficient and NO root was returned (completeness inf against numpy's 2.2e-10).
      The basis is now turned by a fixed orthogonal matrix in general position: 1.2e-12.
  test_true_matrix_is_among_the_roots[planar]    one sample in 1024 met a pivot of 5e-7 in the elimination and returned six
      roots none of which was the true matrix (0.090 against 6.7e-8; tilted plane 8.9e-7 against 6.3e-9).  A sample whose
      smallest pivot is below 1e-4 is now eliminated again in a second basis: 3.0e-11 and 6.2e-12."""
import time

import numpy as np
import pytest

import two_view_ref as tv
from oracle import oracle
from test_two_view_cpu import CAP, DOUBLE_ROOT, FAMILY_WORST, ILL_CONDITIONED, finite_samples, root_gaps

FACTOR = 16.0
SEEDS = range(4)
DRAWS = 256
EPS = np.finfo(np.float64).eps
H_SWEEP = (1, 2, 63, 64, 65, 257, 1000)


def _samples(sc):
    parts = [tv.family_samples(sc, seed, DRAWS) for seed in SEEDS]
    return np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts])


def check_solver_contract(E, n, tag):
    """What every call of the solver owes its caller, whatever the input: 0 - 10 roots, each finite with Frobenius norm 1
    to 4 eps, unused slots zero."""
    assert n.min() >= 0 and n.max() <= 10, tag
    used = np.arange(10)[None, :] < n[:, None]
    assert np.isfinite(E).all(), (tag, "non-finite matrix returned")
    assert not E[~used].any(), (tag, "unused slot not zero")
    nrm = np.linalg.norm(E[used], axis=1)
    assert nrm.size == 0 or np.abs(nrm - 1).max() <= 4 * EPS, (tag, np.abs(nrm - 1).max())


def sample_epipolar(E, n, x1, x2):
    """Per sample the worst |x2^T E x1| over its five points and its returned roots (0 where there is none)."""
    h1 = np.concatenate([x1, np.ones(x1.shape[:2] + (1,))], -1)
    h2 = np.concatenate([x2, np.ones(x2.shape[:2] + (1,))], -1)
    r = np.abs(np.einsum("sni,srij,snj->srn", h2, E.reshape(len(E), 10, 3, 3), h1)).max(2)
    return np.where(np.arange(10)[None, :] < n[:, None], r, 0.0).max(1)


@pytest.mark.parametrize("family", list(tv.FAMILIES))
def test_solver_contract_on_the_twin_and_under_the_sanitizers(family):
    general = np.median(oracle.tv_twin_solve(*_samples(tv.scenes_general()[0]), timed=True)[2])
    for sc in tv.FAMILIES[family]():
        tag = (family, sc["variant"])
        x1, x2 = _samples(sc)
        t0 = time.perf_counter()
        E, n, sec = oracle.tv_twin_solve(x1, x2, timed=True)
        assert time.perf_counter() - t0 < len(x1) * 1.0             # a second per sample is the issue's limit for a device launch
        print(f"{family}/{sc['variant']}: slowest solve {sec.max() * 1e6:.0f} us, median of the general family {general * 1e6:.0f} us,"
              f" mean roots {n.mean():.2f}")
        check_solver_contract(E, n, tag)
        E2, n2 = oracle.tv_twin_solve(x1, x2, fill=float("nan"))   # nothing is read before it is written
        assert np.array_equal(n, n2) and np.array_equal(E, E2), tag
        rc, report, Es, ns = oracle.tv_twin_san_solve(x1, x2)
        assert rc == 0 and report == "", (tag, rc, report[:2000])
        assert ns.tobytes() == n.tobytes() and Es.tobytes() == E.tobytes(), tag
        if family == "non_finite":                                  # a sample that drew a NaN / inf coordinate yields no model
            assert not n[~(np.isfinite(x1).all((1, 2)) & np.isfinite(x2).all((1, 2)))].any(), tag
        if tv.is_degenerate(sc):
            continue                                                # no accuracy is claimed, on any sample
        fin = finite_samples(x1, x2)
        with np.errstate(all="ignore"):
            En, nn, _ = tv.fivepoint(x1[fin], x2[fin])
        got = sample_epipolar(E[fin], n[fin], x1[fin], x2[fin])[nn > 0]
        worst = FAMILY_WORST[f"{family}/{sc['variant']}"]["epipolar"]
        assert got.size and got.max() <= FACTOR * worst, (tag, got.max(), worst)


@pytest.mark.parametrize("family", tv.COMPLETE)
def test_true_matrix_is_among_the_roots(family):
    """The two faults this test found are described in the module docstring."""
    for sc in tv.FAMILIES[family]():
        worst = FAMILY_WORST[f"{family}/{sc['variant']}"].get("completeness")
        x1, x2 = _samples(sc)
        Eg = np.tile(sc["E"], (len(x1), 1))
        E, n = oracle.tv_twin_solve(x1, x2)
        En, nn, zn = tv.fivepoint(x1, x2)
        _, comp = tv.solver_quantities(E, n, x1, x2, Eg)
        _, compn = tv.solver_quantities(En, nn, x1, x2, Eg)
        out = (compn > ILL_CONDITIONED) | (root_gaps(zn) < DOUBLE_ROOT)
        if worst is None:                                           # far/all_far: numpy is outside the cap, see scenes_far
            assert out.mean() > CAP                                 # (if it ever is inside, the variant gets a yardstick)
            print(f"{family}/{sc['variant']}: numpy leaves out {out.mean():.3f}; of the other {int((~out).sum())} samples the twin misses"
                  f" the true matrix (above {FACTOR * ILL_CONDITIONED:g}) on {int((comp[~out] > FACTOR * ILL_CONDITIONED).sum())}")
            continue
        assert out.mean() <= CAP, (family, sc["variant"], out.mean())
        print(f"{family}/{sc['variant']}: completeness twin {comp[~out].max():.3e} numpy {compn[~out].max():.3e}, left out {int(out.sum())},"
              f" root-count mismatches {int((n != nn)[~out].sum())}")
        assert comp[~out].max() <= FACTOR * worst, (family, sc["variant"], comp[~out].max(), worst)


# ------------------------------------------------------------------------------------------------ exact scoring and argmax
def exact_mask(E, sc, threshold=1.0):
    x1, x2 = tv.normalise(sc["px1"], sc["K"]), tv.normalise(sc["px2"], sc["K"])
    with np.errstate(all="ignore"):
        return tv.sampson_sq(E, x1, x2) < tv.threshold_sq(threshold, sc["K"])          # a NaN score is an outlier


def check_ransac_result_exactly(E, mask, st, sc, H, seed, solve, threshold=1.0):
    """The result of a RANSAC call against the header, to the bit: mask and count are the stated formula on the returned
    matrix, and the winner is the max over (count, -hypothesis, -root) of the exact counts of every root of every
    reproduced draw, solved by ``solve`` (the solver entry of whatever ran the RANSAC)."""
    tag = (sc["family"], sc["variant"], H, seed)
    n = len(sc["px1"])
    assert np.array_equal(mask, exact_mask(E, sc, threshold) if np.any(E) else np.zeros(n, bool)), tag
    assert st[0] == mask.sum(), tag
    assert np.isfinite(E).all(), tag
    x1, x2 = tv.normalise(sc["px1"], sc["K"]), tv.normalise(sc["px2"], sc["K"])
    idx = np.array([tv.draw_sample(seed, 0, h, n) for h in range(H)])
    Es, nr = solve(x1[idx], x2[idx])
    assert st[3] == nr.sum(), (tag, st[3], nr.sum())
    t2 = tv.threshold_sq(threshold, sc["K"])
    keys = []
    with np.errstate(all="ignore"):
        for h in range(H):
            for r in range(nr[h]):
                keys.append((int((tv.sampson_sq(Es[h, r], x1, x2) < t2).sum()), -h, -r))
    if not keys:
        assert not E.any() and st.tolist() == [0, -1, -1, 0], tag
        return
    cnt, h, r = max(keys)
    assert st[:3].tolist() == [cnt, -h, -r], (tag, st, (cnt, -h, -r))
    assert Es[-h, -r].tobytes() == np.ascontiguousarray(E, np.float64).tobytes(), tag
    assert abs(np.linalg.norm(E) - 1) <= 4 * EPS, tag


@pytest.mark.parametrize("family", list(tv.FAMILIES))
def test_twin_ransac_mask_and_winner_are_exact_on_every_family(family):
    for sc in tv.FAMILIES[family]():
        E, mask, st = oracle.tv_twin_ransac(sc["px1"], sc["px2"], sc["K"], 64, 1.0, 3)
        check_ransac_result_exactly(E, mask, st, sc, 64, 3, oracle.tv_twin_solve)
        if family == "non_finite":
            assert not mask[sc["bad"]].any()                        # a match with a NaN / inf coordinate is never an inlier
        pose, good, ps, votes = oracle.tv_twin_recover_pose(E, sc["px1"], sc["px2"], sc["K"])
        assert np.isfinite(pose).all() and ps[0] == good.sum() and (ps[0] == votes.max() or ps[1] < 0)
        if ps[1] >= 0:
            assert np.abs(pose[:, :3].T @ pose[:, :3] - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(pose[:, :3]) - 1) < 1e-12
            assert abs(np.linalg.norm(pose[:, 3]) - 1) < 1e-12
        rc, report, res = oracle.tv_twin_san_pair(sc["px1"], sc["px2"], sc["K"], 64, 1.0, 3)
        assert rc == 0 and report == "", (family, sc["variant"], report[:2000])
        assert res["E"].tobytes() == E.tobytes() and res["stats"].tolist() == st.tolist() and np.array_equal(res["mask"].astype(bool), mask)
        assert res["pose"].tobytes() == pose.tobytes() and res["pose_stats"].tolist() == ps.tolist()


def test_twin_ransac_commits_exactly_the_first_H_hypotheses():
    sc = tv.scenes_general(1, 200)[0]
    for H in H_SWEEP:
        E, mask, st = oracle.tv_twin_ransac(sc["px1"], sc["px2"], sc["K"], H, 1.0, 9)
        check_ransac_result_exactly(E, mask, st, sc, H, 9, oracle.tv_twin_solve)
        assert 0 <= st[1] < H


def test_twin_draws_are_the_header_generator_for_every_seed_width():
    for seed in (0, 7, 2 ** 32 + 5, 2 ** 63, 2 ** 64 - 1):
        for n in (5, 6, 200, 2 ** 20):
            for h in (0, 1, 63, 64, 1000, 2 ** 20 - 1):
                assert oracle.tv_twin_draw_sample(seed, h, n) == tv.draw_sample(seed, 0, h, n), (seed, n, h)


def test_twin_scoring_is_the_stated_expression_to_the_bit():
    rng = np.random.default_rng(5)
    for sc in tv.all_family_scenes():
        x1, x2 = tv.normalise(sc["px1"], sc["K"]), tv.normalise(sc["px2"], sc["K"])
        for E in (sc["E"], rng.normal(size=9)):
            assert np.array_equal(oracle.tv_twin_sampson_sq(E, x1, x2), tv.sampson_sq(E, x1, x2), equal_nan=True)
    sc = tv.scenes_epipole_match()[1]                                # forward motion: the epipoles are exact, the score is 0 / 0
    d = oracle.tv_twin_sampson_sq(sc["E"], tv.normalise(sc["px1"], sc["K"]), tv.normalise(sc["px2"], sc["K"]))
    assert np.isnan(d[sc["at_epipole"]]).all()


def test_recover_pose_vote_of_the_twin_against_numpy():
    """Masks given, ties, and distance limits: counts and masks equal tv.recover_pose's outside a 1e-9 relative band of the
    depth bounds (at most 0.5 % of the points, as the Sampson band)."""
    sc = tv.scenes_far(0, 400)[1]                                    # near and far points
    rng = np.random.default_rng(8)
    for inl in (None, rng.uniform(size=400) < 0.5, np.zeros(400, bool), np.ones(400, bool)):
        for dist in (0.5, 5.0, 50.0, 1e6):
            pose, good, ps, votes = oracle.tv_twin_recover_pose(sc["E"], sc["px1"], sc["px2"], sc["K"], inl, dist)
            R, t, gn, sn = tv.recover_pose(sc["E"], sc["px1"], sc["px2"], sc["K"], inl, dist)
            x1, x2 = tv.normalise(sc["px1"], sc["K"]), tv.normalise(sc["px2"], sc["K"])
            X, _ = tv.triangulate(np.eye(4)[:3], np.c_[R, t], x1, x2)
            z = np.stack([X[:, 2], X @ R[2] + t[2]])
            near = (np.abs(z) <= 1e-9).any(0) | (np.abs(z - dist) <= 1e-9 * dist).any(0)
            assert near.mean() <= 0.005
            if sn[0] == 0:
                assert ps.tolist() == [0, 0] and not good.any()    # nothing good anywhere: the tie goes to candidate 0
                continue
            assert np.abs(pose[:, :3] - R).max() < 1e-9 and np.abs(pose[:, 3] - t).max() < 1e-9
            assert np.array_equal(good[~near], gn[~near]) and abs(int(ps[0]) - int(sn[0])) <= near.sum()
    a = oracle.tv_twin_recover_pose(sc["E"], sc["px1"], sc["px2"], sc["K"], None, 50.0)
    b = oracle.tv_twin_recover_pose(sc["E"], sc["px1"], sc["px2"], sc["K"], np.ones(400, bool), 50.0)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))          # an all-one mask is no mask
    lo = oracle.tv_twin_recover_pose(sc["E"], sc["px1"], sc["px2"], sc["K"], None, 50.0)[2][0]
    hi = oracle.tv_twin_recover_pose(sc["E"], sc["px1"], sc["px2"], sc["K"], None, 1e6)[2][0]
    assert lo < hi == 400                                            # the distance filter works: far points only count without it


NOT_ESSENTIAL = dict(
    unequal=lambda R: R @ np.diag([1.0, 0.5, 0.0]) @ R.T, rank1=lambda R: np.outer(R[0], R[1]), rank3=lambda R: R @ np.diag([1.0, 0.7, 0.4]),
    tiny=lambda R: 1e-200 * (R @ np.diag([1.0, 1.0, 0.0])), huge=lambda R: 1e200 * (R @ np.diag([1.0, 1.0, 0.0])),
    one_nan=lambda R: np.where(np.arange(9).reshape(3, 3) == 4, np.nan, R @ np.diag([1.0, 1.0, 0.0])))


def check_pose_or_no_model(pose, good, ps, tag):
    """recoverPose on any 3x3 input: a finite orthonormal pose with |t| = 1, or the documented no-model answer - never NaN."""
    assert np.isfinite(pose).all(), (tag, pose)
    if ps[1] < 0:
        assert np.array_equal(pose, np.eye(4)[:3]) and not good.any() and ps[0] == 0, tag
    else:
        R = pose[:, :3]
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12 and abs(np.linalg.norm(pose[:, 3]) - 1) < 1e-12, tag
        assert ps[0] == good.sum(), tag


def test_recover_pose_of_the_twin_on_matrices_that_are_not_essential():
    sc = tv.scenes_general(2, 100)[0]
    for name, fn in NOT_ESSENTIAL.items():
        E = fn(sc["R"])
        pose, good, ps, _ = oracle.tv_twin_recover_pose(E, sc["px1"], sc["px2"], sc["K"])
        print(name, "-> candidate", ps[1], "good", ps[0])
        check_pose_or_no_model(pose, good, ps, name)
        if name in ("tiny", "huge", "one_nan"):                     # |E|^2 under- / overflows or is NaN: the no-model answer
            assert ps[1] == -1, name


def test_triangulation_of_the_twin_on_general_cameras_and_parallel_rays():
    sc = tv.make_scene(np.random.default_rng(61), 257, 0.5, 0.0)
    Ra = tv._rodrigues(np.array([1.0, 2.0, 3.0]), 0.3)
    Pa = np.c_[Ra, [0.3, -0.2, 0.1]]
    Pb = np.c_[sc["R"] @ Ra, sc["R"] @ Pa[:, 3] + sc["t"]]
    x1, x2 = tv._project(sc["X"] @ Pa[:, :3].T + Pa[:, 3], (1, 1, 0, 0)), tv._project(sc["X"] @ Pb[:, :3].T + Pb[:, 3], (1, 1, 0, 0))
    x1 = x1 + np.random.default_rng(1).normal(0, 1e-3, x1.shape)
    for s in (1.0, 1e3):
        X, w = oracle.tv_twin_triangulate(s * Pa, s * Pb, x1, x2)
        Xs, ws = tv.triangulate(s * Pa, s * Pb, x1, x2)
        Xe, we = tv.triangulate_eig(s * Pa, s * Pb, x1, x2)
        scale = np.linalg.norm(Xs, axis=1)
        own, got = (np.linalg.norm(Xe - Xs, axis=1) / scale).max(), (np.linalg.norm(X - Xs, axis=1) / scale).max()
        print(f"general cameras x {s:g}: twin vs SVD {got:.3e}, numpy eigh vs SVD {own:.3e}")
        assert got <= FACTOR * own and np.abs(w - ws).max() <= FACTOR * max(np.abs(we - ws).max(), 1e-16)
    P1 = np.eye(4)[:3]
    xs = tv.normalise(sc["px1"], tv.EUROC)
    for P2 in (np.c_[np.eye(3), [1.0, 0, 0]], P1):                  # parallel rays (a point at infinity); identical cameras
        X, w = oracle.tv_twin_triangulate(P1, P2, xs, xs)
        Xs, ws = tv.triangulate(P1, P2, xs, xs)
        Xe, we = tv.triangulate_eig(P1, P2, xs, xs)
        assert np.isfinite(w).all() and (w >= 0).all()
        if P2 is not P1:                                            # identical cameras: a two-dimensional null space, any unit v
            assert np.abs(w - ws).max() <= FACTOR * max(np.abs(we - ws).max(), 1e-16)
            assert (np.isfinite(X).all(1) | (ws < 1e-12)).all()
