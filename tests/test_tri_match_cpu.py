"""The epipolar node search and new-map-point creation without a device: the fundamental matrix and epipole of
the Python layer, the host twin of csrc/tri_point.h (also under AddressSanitizer and UndefinedBehaviorSanitizer) against the numpy
reference - the gates bit for bit, the geometry against the SVD route within a measured tolerance - one hand-built match per
status, the condition the GPU chain test puts on its scene, and the limits, plan and argument checks."""
import ctypes
import os

import numpy as np
import pytest

import tri_match_cases as C
import tri_match_ref as R
import tri_match_twin as TW

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# the largest relative difference |X_twin - X_svd| / |X_svd| the twin showed against the SVD route on the 300-match scene and
# the hand-built cases on the development CPU (printed by test_geometry_twin_against_the_svd_route); the gate is 16 times it
X_REL_MEASURED = 9.773e-14
X_REL_GATE = 16 * X_REL_MEASURED


@pytest.fixture(scope="module")
def tm(built):
    from slamhip import tri_match as module
    return module


@pytest.fixture(autouse=True)
def _the_feature_is_there(tm):
    """Every test of this file, the ones on the reference and the twin included, needs the module it is about."""
    return tm


# ---- fundamental matrix and epipole --------------------------------------------------------------------------------------------

def test_fundamental_matrix_and_epipole(tm):
    rng = np.random.default_rng(5)
    T1, T2 = C.POSES[0], C.POSES[1]
    F = tm.fundamental_from_poses(T1, T2, C.CAMERA)
    assert np.allclose(F, R.fundamental(T1, T2, C.CAMERA), rtol=1e-12, atol=1e-18)
    px = np.stack([rng.uniform(0, 640, 400), rng.uniform(0, 480, 400)], 1)
    z = rng.uniform(2.0, 8.0, 400)
    W = (np.stack([(px[:, 0] - 320) / 256 * z, (px[:, 1] - 240) / 256 * z, z], 1) - T1[:, 3]) @ T1[:, :3]
    p1, _ = R.project(T1, W, C.CAMERA)
    p2, d2 = R.project(T2, W, C.CAMERA)
    assert (d2 > 0).all()
    a, b, c = (p1[:, 0] * F[0, k] + p1[:, 1] * F[1, k] + F[2, k] for k in range(3))
    num, den = a * p2[:, 0] + b * p2[:, 1] + c, a * a + b * b
    dist = np.abs(num) / np.sqrt(den)
    print("largest distance of a projected point from its epipolar line: %.3e px" % dist.max())
    assert (dist < 1e-6).all()
    h1, h2 = np.c_[p1, np.ones(400)], np.c_[p2, np.ones(400)]
    assert np.abs(np.einsum("ni,ij,nj->n", h1, F, h2)).max() < 1e-6 * np.sqrt(den).max()
    # the epipole: camera 1's centre projected into image 2; the backwards pair sees it behind
    e = tm.epipole_in_second(T1, T2, C.CAMERA)
    want, depth = R.project(T2, R.centre(T1)[None], C.CAMERA)
    assert depth[0] < 0 and np.isnan(e).all()
    Tb = C.pose(np.eye(3), [0.1, 0.0, -2.0])                 # camera 2 two units behind camera 1: it sees camera 1's centre
    e = tm.epipole_in_second(T1, Tb, C.CAMERA)
    want, depth = R.project(Tb, R.centre(T1)[None], C.CAMERA)
    assert depth[0] > 0 and np.allclose(e, want[0], rtol=1e-12)
    # every epipolar line of image 2 passes through it
    F = tm.fundamental_from_poses(T1, Tb, C.CAMERA)
    l = np.c_[p1, np.ones(400)] @ F
    assert (np.abs(l @ np.r_[e, 1.0]) / np.hypot(l[:, 0], l[:, 1]) < 1e-6).all()
    for bad in (np.zeros((3, 3)), np.zeros(12)):
        with pytest.raises(ValueError):
            tm.fundamental_from_poses(bad, T2, C.CAMERA)


# ---- the gates: twin against reference, bit for bit --------------------------------------------------------------------------------

@pytest.mark.parametrize("san", [False, True])
def test_gates_twin_equals_the_reference_on_a_scene(san):
    s1, s2, _, truth = C.make_scene(11, 150, 300)
    F = R.fundamental(C.POSES[0], C.POSES[1], C.CAMERA)
    for epipole in (C.NO_EPIPOLE, np.array([300.0, 200.0])):                            # (a radius of 100 px at level 0)
        off, on = R.gates(F, epipole, s1["xy"], s2["xy"], s2["level"], C.SCALE, C.SIGMA2, epipole_r2=1e4)
        toff, ton = TW.gates(F, epipole, s1["xy"], s2["xy"], s2["level"], C.SCALE, C.SIGMA2, epipole_r2=1e4, san=san)
        assert np.array_equal(ton, on) and np.array_equal(toff, np.broadcast_to(off[None, :], toff.shape))
        assert on[truth["rows1"], truth["rows2"]].mean() > 0.95 and on.mean() < 0.1      # the true pairs pass, few others do
    assert 0 < off.sum() < len(off)                          # the epipole gate removes some rows of this scene, not all


@pytest.mark.parametrize("san", [False, True])
def test_gates_on_the_exact_edge_set(san):
    xy1, xy2, level2, scale, sigma2, chi2, cases = C.edge_gates()
    for F, epipole, want in cases:
        off, on = R.gates(F, epipole, xy1, xy2, level2, scale, sigma2, chi2, 100.0)
        toff, ton = TW.gates(F, epipole, xy1, xy2, level2, scale, sigma2, chi2, 100.0, san=san)
        assert np.array_equal(on, want) and np.array_equal(ton, want)
        assert np.array_equal(toff, np.broadcast_to(off[None, :], toff.shape))
        if np.isnan(epipole).any():
            assert off.all()
    # the epipole (7, 92) at r2 = 100: (7, 102) is at exactly 10 px on level 0 (scale 1): equality is NOT inside, it stays;
    # (9, 98) at sqrt(40) px goes; on level 1 (scale 2, r2 = 200) (3, 104) at sqrt(160) px goes
    off, _ = R.gates(cases[0][0], np.array([7.0, 92.0]), xy1, xy2, level2, scale, sigma2, chi2, 100.0)
    assert off.tolist() == [False, True, False, False, False, False]


# ---- the geometry: twin against the SVD route ----------------------------------------------------------------------------------------

def _scene_matches(seed=11):
    s1, s2, _, truth = C.make_scene(seed, 300, 300)
    return s1["xy"][truth["rows1"]], s2["xy"][truth["rows2"]], s1["level"][truth["rows1"]], s2["level"][truth["rows2"]], truth["X"]


@pytest.mark.parametrize("san", [False, True])
def test_geometry_twin_against_the_svd_route(san):
    xy1, xy2, l1, l2, X = _scene_matches()
    l2 = l2.copy()
    l2[::9] += 4                                              # some scale-inconsistent matches
    xy2 = xy2.copy()
    xy2[::7, 1] += 8.0                                        # some matches off their epipolar plane
    T1, T2 = C.POSES[0], C.POSES[1]
    margins = []
    m12 = np.arange(300)
    want = R.triangulate(T1, T2, C.CAMERA, C.SCALE, C.SIGMA2, xy1, xy2, l1, l2, m12, margins=margins)
    assert min(margins) > 1e-6, "a checked quantity lies within a relative 1e-6 of its threshold: the scene has no margin"
    got = TW.triangulate(T1, T2, C.CAMERA, C.SCALE, C.SIGMA2, xy1, xy2, l1, l2, san=san)
    assert got["status"].tolist() == want["status"].tolist()
    assert {0, 6, 8} <= set(want["status"].tolist()) and (want["status"] == 0).sum() > 200
    ok = want["status"] == 0
    rel = np.linalg.norm(got["X"][ok] - want["X"][ok], axis=1) / np.linalg.norm(want["X"][ok], axis=1)
    print("largest relative difference of X, twin against the SVD route: %.3e" % rel.max())
    assert rel.max() <= X_REL_GATE
    assert np.allclose(got["normal"][ok], want["normal"][ok], rtol=0, atol=64 * X_REL_GATE)
    assert np.allclose(got["dmin2"][ok], want["dmin2"][ok], rtol=64 * X_REL_GATE) and np.allclose(got["dmax2"][ok], want["dmax2"][ok], rtol=64 * X_REL_GATE)
    for k in ("X", "normal", "dmin2", "dmax2"):
        assert np.isnan(got[k][~ok]).all() and np.isfinite(got[k][ok]).all()
    # the triangulated points are the scene's, to the pixel noise
    clean = ok & (np.arange(300) % 7 != 0)
    assert np.linalg.norm(got["X"][clean] - X[clean], axis=1).max() < 0.5


@pytest.mark.parametrize("san", [False, True])
def test_one_hand_built_match_for_every_status(san):
    seen = []
    for T1, T2, p1, p2, l1, l2, status in C.status_cases():
        got = TW.triangulate_centres(T1, T2, R.centre(T1) if np.isfinite(T1).all() else np.zeros(3),
                                     R.centre(T2) if np.isfinite(T2).all() else np.array([np.inf, 0.0, 0.0]), C.CAMERA, C.SCALE, C.SIGMA2,
                                     [p1], [p2], [l1], [l2], san=san)
        assert got["status"][0] == status, (status, got)
        ref = R.triangulate(T1, T2, C.CAMERA, C.SCALE, C.SIGMA2, [p1], [p2], [l1], [l2], [0])
        assert ref["status"][0] == status
        assert np.isnan(got["X"][0]).all() == (status != 0)
        seen.append(status)
    assert seen == [0, 2, 3, 4, 5, 6, 7, 8]
    got = TW.triangulate(C.status_cases()[0][0], C.status_cases()[0][1], C.CAMERA, C.SCALE, C.SIGMA2, [(352.0, 240.0)], [(288.0, 240.0)], [2], [2])
    assert np.allclose(got["X"][0], [0.5, 0.0, 4.0], atol=1e-12)
    d1, d2 = np.sqrt(16.25), np.sqrt(16.25)
    assert np.allclose(got["dmax2"][0], (d1 * C.SCALE[2]) ** 2) and np.allclose(got["dmin2"][0], (d1 * C.SCALE[2] / C.SCALE[7]) ** 2)
    n = np.array([0.5, 0, 4]) / d1 + np.array([-0.5, 0, 4]) / d2
    assert np.allclose(got["normal"][0], n / np.linalg.norm(n))


# ---- the scene of the GPU chain test ---------------------------------------------------------------------------------------------

def test_scene_condition_of_the_chain_test():
    """The reference alone creates at least 90 % of the points both keyframes see in the scene the GPU chain test uses."""
    s1, s2, _, truth = C.make_scene(3, 150, 200)
    T1, T2 = C.POSES[0], C.POSES[1]
    F = R.fundamental(T1, T2, C.CAMERA)
    m12, count, _ = R.search(s1, s2, F, C.NO_EPIPOLE, C.SCALE, C.SIGMA2)
    pts = R.triangulate(T1, T2, C.CAMERA, C.SCALE, C.SIGMA2, s1["xy"], s2["xy"], s1["level"], s2["level"], m12)
    right = (m12[truth["rows1"]] == truth["rows2"]) & (pts["status"][truth["rows1"]] == 0)
    print("created %d of %d common points (%d matches)" % (right.sum(), len(right), count))
    assert right.sum() >= 0.9 * 150
    assert np.linalg.norm(pts["X"][truth["rows1"]][right] - truth["X"][right], axis=1).max() < 0.5


def test_reference_search_against_plain_loops():
    s1, s2 = C.random_pair(2, 40, 50, n_nodes=3)
    idx, dist = R.tables(s1, s2, C.F_RECT, C.EPIPOLE_RECT, C.SCALE, C.SIGMA2, th_low=60)
    off, on = R.gates(C.F_RECT, C.EPIPOLE_RECT, s1["xy"], s2["xy"], s2["level"], C.SCALE, C.SIGMA2)
    d = R.PR.hamming(s1["desc"], s2["desc"])
    for i in range(40):
        cand = sorted((int(d[i, j]), j) for j in range(50) if s1["nodes"][i] == s2["nodes"][j] >= 0 and not s1["taken"][i] and not s2["taken"][j]
                      and d[i, j] <= 60 and off[j] and on[i, j])
        want = cand[:2] + [(R.NONE_DIST, R.NONE_IDX)] * (2 - len(cand[:2]))
        assert [(int(dist[i, k]), int(idx[i, k])) for k in range(2)] == want
    assert (idx[:, 0] >= 0).sum() > 5 and (idx[:, 1] >= 0).sum() > 0


# ---- ABI, limits, plan, argument checks -----------------------------------------------------------------------------------------

def test_abi_limits_and_plan(tm):
    from slamhip import _lib, bow_match
    names = ["slam_tri_match_limits", "slam_tri_match_plan_describe", "slam_tri_match_search", "slam_tri_match_triangulate"]
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "slamhip.h")).read()
    for n in names:
        assert n in _lib.SIGNATURES and hasattr(lib, n) and f"SLAM_API int {n}(" in header
    assert "ORBmatcher::SearchForTriangulation" in header and "LocalMapping::CreateNewMapPoints" in header
    assert ctypes.sizeof(_lib.TriViews) == 24 and ctypes.sizeof(_lib.TriParams) == 96
    lim = tm.limits()
    assert lim["rows_per_image"] == tm.ROWS_MAX == bow_match.ROWS_MAX == 8192 and lim["pairs_per_call"] == tm.PAIRS_MAX == 4096
    assert lim["levels"] == 16 and lim["scan_lanes"] == 64 and lim["bins"] == 32
    assert lim["search_pair_bytes"] == 136 and lim["triangulate_pair_bytes"] == 288
    plan = tm.plan_describe(256, 2000)
    assert plan["scan_blocks"] == 256 * 32 and plan["triangulate_blocks"] == 256 * 8 and plan["finish_blocks"] == 256
    assert plan["search_workspace_bytes"] >= lim["params_bytes"] + 256 * 136 + 2 * 8 * 256 * 2000 + 4 * 256 * 2000
    assert lim["params_bytes"] + 256 * 288 <= plan["triangulate_workspace_bytes"] < plan["search_workspace_bytes"]
    for args in ((4097, 10), (1, 8193), (-1, 1)):
        with pytest.raises(_lib.SlamHipError):
            tm.plan_describe(*args)
    assert lib.slam_tri_match_limits(None) == _lib.SLAM_ERR_INVALID
    assert lib.slam_tri_match_search(*[None] * 6, 0, *[None] * 3, 0, *[None] * 4) == _lib.SLAM_ERR_INVALID
    assert lib.slam_tri_match_triangulate(None, None, 0, None, 0, None, None, None, 0, *[None] * 11) == _lib.SLAM_ERR_INVALID


def test_python_argument_checks(tm):
    with pytest.raises(ValueError):
        tm.search_for_triangulation(None, None, [(0, 0)], None, None, np.eye(3), C.NO_EPIPOLE)
    for bad in (dict(th_low=257), dict(th_low=-1), dict(th_low=1.5), dict(chi2=float("nan")), dict(scale=(np.ones(17), np.ones(17)))):
        kw = dict(camera=C.CAMERA, scale=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            tm._params(**kw)
    prm, keep = tm._params(C.CAMERA, None)
    assert prm.n_levels == 8 and prm.th_low == 50 and prm.ratio_factor == 1.5 * keep[0][1] and prm.chi2 == 3.84
    with pytest.raises(ValueError):
        tm._pair_f64(np.zeros((2, 3, 3)), 3, (3, 3), "F")
    with pytest.raises(ValueError):
        tm.epi_match_arrays(np.zeros((1, 32), np.uint8), np.zeros((1, 32), np.uint8), [0], [0], [[0, 0]], [[0, 0]], [0], np.eye(3), k=3)
