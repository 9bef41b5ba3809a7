"""CPU suite of the pose-graph optimisation: the numpy reference checks itself, the yardsticks the GPU tests use are measured
here (constants below, with the code that measures them), and the product code that needs no GPU (g2o text, argument
checks, loop-closure edges, the Backend glue) is exercised."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_ref as R  # noqa: E402

# ---- yardsticks (measured by the tests below on the committed scenes and seeds; the GPU tests import them) -----------------
# (a) linearisation: largest difference between the reference's closed-form path and its series path over the small scenes,
#     with and without Huber, each relative to the largest magnitude of the quantity
YARD_LIN = {"cost": 3.4e-16, "grad": 4.9e-14, "Hdiag": 3.7e-15, "W": 2.5e-14}
# scipy's CSR product against a dense numpy product of the same matrix (relative to the largest entry of the result)
YARD_HMUL = 2.8e-15
# true residual of the reference PCG's solution over the residual of its recurrence (the recomputation factor)
YARD_PCG_RECOMPUTE = 1.0000005
# (b) solve, per scene: reference-PCG LM against reference-direct LM after 15 iterations at PCG_TOL / PCG_MAX_ITER
#     (relative chi2, radians, fraction of the extent)
YARD_SOLVE = {
    "sphere": {"chi2": 3.1e-11, "rotation": 7.3e-6, "translation": 3.9e-6},
    "loop_closure": {"chi2": 3.7e-14, "rotation": 5.7e-9, "translation": 3.1e-9},
    "hub": {"chi2": 5.9e-16, "rotation": 1.8e-10, "translation": 8.5e-11},
}
ANGLE_CAP = 3.0
LIN_MARGIN, HMUL_MARGIN, SOLVE_MARGIN = 16.0, 16.0, 4.0


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(float(np.abs(b).max()), 1e-300))


@functools.lru_cache(maxsize=None)
def scene(name):
    return R.SMALL_SCENES[name]()


@functools.lru_cache(maxsize=None)
def solved(name, solver):
    """reference LM on a scene: (poses, stats, largest residual angle over every visited state)"""
    s = scene(name)
    angles = []
    P, st = R.optimize(s.init, s.edges, s.meas, s.info, s.fixed, solver=solver,
                       visit=lambda p: angles.append(R.max_residual_angle(p, s.edges, s.meas)))
    return P, st, max(angles)


def honest(measured, constant):
    """the committed constant bounds the measurement and is not padded"""
    assert measured <= constant, f"measured {measured:.3e} exceeds the committed yardstick {constant:.3e}"
    assert constant <= 4 * max(measured, 1e-300), f"yardstick {constant:.3e} is padded: measured {measured:.3e}"


# ---------------------------------------------------------------- the reference checks itself --------------------------------
def test_jacobians_against_central_differences():
    rng = np.random.default_rng(0)
    V = 4
    poses = R.exp_se3(np.concatenate([rng.normal(0, 0.8, (V, 3)), rng.normal(0, 2, (V, 3))], 1))
    edges = np.array([[0, 1], [1, 2], [2, 3], [3, 0]], np.int32)
    Z = R.exp_se3(np.concatenate([rng.normal(0, 0.8, (4, 3)), rng.normal(0, 2, (4, 3))], 1))
    r0, A = R.residuals(poses, edges, Z)
    Jj = R.jl_inv_closed(r0)
    Ji = -Jj @ R.adjoint(A)
    h, worst = 1e-6, 0.0
    for e, (i, j) in enumerate(edges):
        for which, J in ((i, Ji[e]), (j, Jj[e])):
            num = np.zeros((6, 6))
            for a in range(6):
                d = np.zeros(6)
                d[a] = h
                pp, pm = poses.copy(), poses.copy()
                pp[which] = R.mul(R.exp_se3(d), poses[which])
                pm[which] = R.mul(R.exp_se3(-d), poses[which])
                num[:, a] = (R.residuals(pp, edges, Z)[0][e] - R.residuals(pm, edges, Z)[0][e]) / (2 * h)
            worst = max(worst, np.abs(num - J).max())
    assert worst < 1e-7, worst          # h^2 truncation + eps / h rounding of a central difference


def test_closed_form_against_bernoulli_series():
    rng = np.random.default_rng(1)
    for scale in (1e-6, 1e-3, 0.05, 0.5, 2.0, 3.0):
        w = rng.normal(size=(50, 3))
        w *= scale * rng.uniform(0.2, 1.0, (50, 1)) / np.linalg.norm(w, axis=1, keepdims=True)
        xi = np.concatenate([w, rng.normal(0, 3, (50, 3))], 1)
        a, b = R.jl_inv_closed(xi), R.jl_inv_series(xi)
        assert np.abs(a - b).max() < 1e-12 * max(1.0, np.abs(b).max()), scale
        assert np.abs(R.log_se3(R.exp_se3(xi)) - xi).max() < 1e-12 * max(1.0, np.abs(xi).max()), scale
        assert np.abs(R.log_se3(R.exp_se3(xi), series=True) - xi).max() < 1e-12 * max(1.0, np.abs(xi).max()), scale


@pytest.mark.parametrize("name", sorted(R.SMALL_SCENES))
def test_reference_lm_lowers_chi2_and_stays_under_the_angle_cap(name):
    """The condition on the generators: every state the reference LM visits has every residual's rotation below 3.0 rad."""
    for solver in ("direct", "pcg"):
        P, st, angle = solved(name, solver)
        assert st["chi2_final"] < 0.1 * st["chi2_initial"], (solver, st)
        assert st["trials"] >= st["iterations"] >= 1
        assert angle < ANGLE_CAP, (solver, angle)
        assert R.trajectory_error(P, scene(name).gt) < R.trajectory_error(scene(name).init, scene(name).gt)


def test_scene_sizes():
    s = scene("sphere")
    assert (s.V, s.fixed.sum(), s.fixed[0]) == (2500, 1, 1) and 9500 < s.E < 10500
    s = scene("loop_closure")
    assert s.V == 512 and 24 <= s.E - 511 <= 60
    s = scene("hub")
    assert np.bincount(s.edges.ravel())[0] == 1000 and s.fixed[1] == 1 and s.fixed.sum() == 1


# ---------------------------------------------------------------- the yardsticks ----------------------------------------------
def test_yardstick_linearisation():
    worst = dict.fromkeys(YARD_LIN, 0.0)
    for name in R.SMALL_SCENES:
        s = scene(name)
        for huber in (0.0, 3.0):
            a = R.linearize(s.init, s.edges, s.meas, s.info, huber, series=False)
            b = R.linearize(s.init, s.edges, s.meas, s.info, huber, series=True)
            worst["cost"] = max(worst["cost"], abs(a[0] - b[0]) / a[0])
            for key, k in (("grad", 1), ("Hdiag", 2), ("W", 3)):
                worst[key] = max(worst[key], rel(a[k], b[k]))
    print("yardstick (a):", worst)
    for key in YARD_LIN:
        honest(worst[key], YARD_LIN[key])


def test_yardstick_product_and_pcg_recomputation():
    rng = np.random.default_rng(7)
    worst_mul, worst_ratio = 0.0, 0.0
    for name in R.SMALL_SCENES:
        s = scene(name)
        _, b, Hd, W = R.linearize(s.init, s.edges, s.meas, s.info)
        H = R.assemble(s.V, s.edges, Hd, W)
        dense = H.toarray()
        for _ in range(4):
            x = rng.normal(size=6 * s.V)
            worst_mul = max(worst_mul, rel(H @ x, dense @ x))
        f = R.free_index(s.fixed)
        Hff, bf, lam = H[f][:, f].tocsr(), b.ravel()[f], 1e-3 * np.abs(Hd).max()
        x, it, rr = R.pcg(Hff, bf, lam, R.PCG_TOL, 5000)
        assert it < 5000 and rr <= R.PCG_TOL
        worst_ratio = max(worst_ratio, float(np.linalg.norm(Hff @ x + lam * x + bf) / np.linalg.norm(bf)) / rr)
    print("csr vs dense:", worst_mul, "true / recurrence residual:", worst_ratio)
    honest(worst_mul, YARD_HMUL)
    honest(worst_ratio - 1.0, YARD_PCG_RECOMPUTE - 1.0)      # the quantity of interest is the excess over 1


def test_yardstick_solve_pcg_lm_against_direct_lm():
    assert sorted(YARD_SOLVE) == sorted(R.SMALL_SCENES)
    for name in R.SMALL_SCENES:
        Pd, sd, _ = solved(name, "direct")
        Pp, sp_, _ = solved(name, "pcg")
        ang, dist = R.pose_gap(Pp, Pd)
        got = {"chi2": abs(sp_["chi2_final"] - sd["chi2_final"]) / sd["chi2_final"], "rotation": ang,
               "translation": dist / R.extent(scene(name).gt)}
        assert sp_["cg_iterations"] <= sp_["trials"] * R.PCG_MAX_ITER
        print("yardstick (b):", name, got)
        for key in got:
            honest(got[key], YARD_SOLVE[name][key])


def test_huber_helps_against_wrong_closures_in_the_reference():
    """the claim the GPU test makes, checked on the reference for the committed seed: 10 % wrong closures, Huber on / off"""
    s = R.loop_closure(outlier_fraction=0.1)
    angles = []
    visit = lambda p: angles.append(R.max_residual_angle(p, s.edges, s.meas))
    plain, _ = R.optimize(s.init, s.edges, s.meas, s.info, s.fixed, huber=0.0, visit=visit)
    robust, _ = R.optimize(s.init, s.edges, s.meas, s.info, s.fixed, huber=3.0, visit=visit)
    assert max(angles) < ANGLE_CAP
    assert R.trajectory_error(robust, s.gt) < R.trajectory_error(plain, s.gt)


# ---------------------------------------------------------------- product code without a GPU ---------------------------------
HAND_G2O = """VERTEX_SE3:QUAT 10 0 0 0 0 0 0 1
VERTEX_SE3:QUAT 11 1 0 0 0 0 0.7071067811865476 0.7071067811865476
VERTEX_SE3:QUAT 12 1 2 0 0 0 1 0
EDGE_SE3:QUAT 10 11 1 0 0 0 0 0.7071067811865476 0.7071067811865476 1 2 3 4 5 6 7 8 9 10 11 12 13 14 15 16 17 18 19 20 21
EDGE_SE3:QUAT 11 12 2 0 0 0 0 0.7071067811865476 0.7071067811865476 100 0 0 0 0 0 100 0 0 0 0 100 0 0 0 400 0 0 400 0 400
FIX 10
"""


def test_read_g2o_hand_written_graph():
    from slamhip import read_g2o

    g = read_g2o(HAND_G2O)
    assert g["ids"].tolist() == [10, 11, 12] and g["edges"].tolist() == [[0, 1], [1, 2]]
    # vertex 11: camera-to-world = (Rz(90 deg), centre (1, 0, 0)); the project's pose is its inverse
    Rz = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    assert np.allclose(g["poses"][1][:, :3], Rz.T, atol=1e-15) and np.allclose(g["poses"][1][:, 3], -Rz.T @ [1, 0, 0], atol=1e-15)
    assert np.allclose(R.centres(g["poses"]), [[0, 0, 0], [1, 0, 0], [1, 2, 0]], atol=1e-15)
    # the measurements are exact for these vertices: Z = T_j T_i^-1, residual zero
    r, _ = R.residuals(g["poses"], g["edges"], g["meas"])
    assert np.abs(r).max() < 1e-14          # a few ulp of coordinates of magnitude 2
    # information: [t, q] upper triangle -> [w, v] with Omega_ww = Omega_qq / 4, Omega_wv = Omega_qv / 2
    M = np.zeros((6, 6))
    M[np.triu_indices(6)] = np.arange(1, 22)
    M = M + np.triu(M, 1).T
    I0 = g["info"][0]
    assert np.allclose(I0[:3, :3], M[3:, 3:] / 4) and np.allclose(I0[3:, 3:], M[:3, :3]) and np.allclose(I0[:3, 3:], M[3:, :3] / 2)
    assert np.allclose(I0, I0.T)
    assert np.allclose(g["info"][1], np.diag([100.0] * 6))


def test_g2o_round_trip():
    from slamhip import read_g2o, write_g2o

    s = scene("loop_closure")
    rng = np.random.default_rng(3)
    A = rng.normal(size=(s.E, 6, 6))
    info = A @ np.swapaxes(A, 1, 2) + 6 * np.eye(6)
    ids = np.arange(s.V) * 3 + 5
    g = read_g2o(write_g2o(s.init, s.edges, s.meas, info, ids=ids))
    assert np.array_equal(g["ids"], ids) and np.array_equal(g["edges"], s.edges)
    assert np.abs(g["poses"] - s.init).max() < 1e-13 * 25 and np.abs(g["meas"] - s.meas).max() < 1e-13
    assert rel(g["info"], info) < 1e-15
    assert write_g2o(g["poses"], g["edges"], g["meas"], g["info"], ids=g["ids"]).count("EDGE_SE3:QUAT") == s.E


def test_read_g2o_refuses_malformed_text(tmp_path):
    from slamhip import read_g2o, write_g2o

    with pytest.raises(ValueError):
        read_g2o("VERTEX_SE3:QUAT 0 0 0 0 0 0 0\n")
    with pytest.raises(ValueError):
        read_g2o("VERTEX_SE3:QUAT 0 0 0 0 0 0 0 1\nEDGE_SE3:QUAT 0 5 " + " ".join(["1"] * 28) + "\n")
    with pytest.raises(ValueError):
        read_g2o("VERTEX_SE3:QUAT 0 0 0 0 0 0 0 1\nVERTEX_SE3:QUAT 0 0 0 0 0 0 0 1\n")
    path = tmp_path / "tiny.g2o"
    write_g2o(np.eye(4)[None], np.zeros((0, 2), np.int32), np.zeros((0, 12)), np.zeros((0, 6, 6)), path=str(path))
    assert read_g2o(str(path))["poses"].shape == (1, 3, 4)


def test_bad_arguments_raise_before_the_ffi_call(monkeypatch):
    import slamhip
    from slamhip import pose_graph as pg

    def boom(*a, **k):
        raise AssertionError("the FFI was reached")

    monkeypatch.setattr(pg, "default_context", boom)
    s = scene("loop_closure")
    ok = (s.init, s.edges, s.meas, s.info, s.fixed)
    bad = [
        (s.init.reshape(-1, 6), s.edges, s.meas, s.info, s.fixed),              # pose shape
        (s.init.astype(object), s.edges, s.meas, s.info, s.fixed),              # pose dtype
        (s.init, s.edges.astype(np.float64), s.meas, s.info, s.fixed),          # edge dtype
        (s.init, s.edges[:, :1], s.meas, s.info, s.fixed),                      # edge shape
        (s.init, s.edges, s.meas[:-1], s.info, s.fixed),                        # one measurement per edge
        (s.init, s.edges, s.meas, s.info.reshape(-1, 36)[:, :21], s.fixed),     # information shape
        (s.init, s.edges, s.meas, s.info, s.fixed[:-1]),                        # mask length
        (s.init, s.edges, s.meas, s.info, np.zeros(s.V, np.uint8)),             # no fixed vertex
        (s.init, s.edges, s.meas, s.info, None),
    ]
    for args in bad:
        with pytest.raises(ValueError):
            slamhip.optimize_pose_graph(*args)
    for kw in (dict(iterations=-1), dict(huber_delta=-1.0), dict(pcg_tol=0.0), dict(pcg_tol=1.5), dict(pcg_max_iter=0), dict(iterations=1.5)):
        with pytest.raises(ValueError):
            slamhip.optimize_pose_graph(*ok, **kw)
    with pytest.raises(ValueError):
        slamhip.pose_graph_linearize(s.init, s.edges, s.meas[:-1], s.info)
    with pytest.raises(ValueError):
        slamhip.pose_graph_hmul(s.edges, s.fixed, np.zeros((s.V, 6, 6)), np.zeros((s.E, 6, 6)), 0.0, np.zeros(5))
    with pytest.raises(ValueError):
        slamhip.pose_graph_pcg(s.edges, s.fixed, np.zeros((s.V, 6, 6)), np.zeros((s.E - 1, 6, 6)), np.zeros((s.V, 6)), 0.0)
    # all three pose formats are accepted (an empty graph never reaches the device)
    for shape in ((0, 12), (0, 3, 4), (0, 4, 4)):
        P, st = slamhip.optimize_pose_graph(np.zeros(shape), np.zeros((0, 2), np.int32), np.zeros((0, 12)), np.zeros((0, 6, 6)), np.zeros(0))
        assert P.shape == shape and st["trials"] == 0


def test_read_g2o_takes_paths_explicitly(tmp_path):
    import pathlib

    from slamhip import read_g2o, write_g2o

    spaced = tmp_path / "a graph with spaces.g2o"
    write_g2o(np.eye(4)[None], np.zeros((0, 2), np.int32), np.zeros((0, 12)), np.zeros((0, 6, 6)), path=str(spaced))
    assert len(read_g2o(str(spaced))["ids"]) == 1 and len(read_g2o(pathlib.Path(spaced))["ids"]) == 1
    with pytest.raises(FileNotFoundError):                   # a mistyped path is not an empty graph
        read_g2o(str(tmp_path / "no such file.g2o"))
    with pytest.raises(TypeError):
        read_g2o(17)


def test_hooks_refuse_non_integer_edges():
    import slamhip

    s = scene("loop_closure")
    Hd, W = np.zeros((s.V, 6, 6)), np.zeros((s.E, 6, 6))
    for bad in (s.edges.astype(np.float64), s.edges.astype(np.int64) + 2**31, s.edges.reshape(-1)):
        with pytest.raises(ValueError):
            slamhip.pose_graph_hmul(bad, s.fixed, Hd, W, 0.0, np.zeros((s.V, 6)))
        with pytest.raises(ValueError):
            slamhip.pose_graph_pcg(bad, s.fixed, Hd, W, np.zeros((s.V, 6)), 0.0)


def test_multi_hub_scene():
    s = R.multi_hub()
    deg = np.bincount(s.edges.ravel(), minlength=s.V)
    assert (deg[:70] == 140).all() and deg[70:].max() <= 72 and s.fixed[70] == 1 and s.fixed.sum() == 1
    assert R.max_residual_angle(s.init, s.edges, s.meas) < ANGLE_CAP


def test_vertex_lists_are_stable_and_skip_bad_indices():
    from slamhip.pose_graph import vertex_lists

    edges = np.array([[0, 1], [2, 1], [1, 0], [7, 2], [-1, 0]], np.int32)
    ptr, adj = vertex_lists(3, edges)
    assert ptr.tolist() == [0, 3, 6, 8]
    assert adj.tolist()[:8] == [0, 5, 9, 1, 3, 4, 2, 7] and adj.tolist()[8:] == [-1, -1]


def test_loop_edges_from_two_view():
    from slamhip import loop_edges_from_two_view

    pairs = np.array([[3, 40], [5, 77], [9, 9], [12, 90]])
    Rm = np.tile(np.eye(3), (4, 1, 1))
    t = np.tile([0.0, 0.6, 0.8], (4, 1))
    counts = np.array([80, 10, 200, 40])
    edges, meas, info = loop_edges_from_two_view(pairs, Rm, t, counts, min_inliers=20, rotation_sigma=0.01)
    assert edges.dtype == np.int32 and edges.tolist() == [[3, 40], [12, 90]]          # too few inliers and the self-pair are dropped
    assert meas.shape == (2, 3, 4) and info.shape == (2, 6, 6)
    assert np.all(info[:, 3:, :] == 0) and np.all(info[:, :, 3:] == 0)               # unknown scale: no translation information
    assert np.allclose(info[0, :3, :3], np.eye(3) * 4e4) and np.allclose(info[1, :3, :3], np.eye(3) * 2e4)
    edges, meas, info = loop_edges_from_two_view(pairs, Rm, t, counts, scale=[2.0, 1.0, 1.0, 0.5], translation_sigma=0.1)
    assert np.allclose(meas[:, :, 3], [[0, 1.2, 1.6], [0, 0.3, 0.4]]) and np.allclose(info[:, 3:, 3:], np.eye(3) * 100)
    with pytest.raises(ValueError):
        loop_edges_from_two_view(pairs, Rm[:3], t, counts)
    with pytest.raises(ValueError):
        loop_edges_from_two_view(pairs.astype(float), Rm, t, counts)
    e0, m0, i0 = loop_edges_from_two_view(np.zeros((0, 2), int), np.zeros((0, 3, 3)), np.zeros((0, 3)), np.zeros(0, int))
    assert e0.shape == (0, 2) and m0.shape == (0, 3, 4) and i0.shape == (0, 6, 6)


def test_backend_pose_graph_glue_without_gpu(monkeypatch):
    import backend
    from slamhip import pose_graph as pg

    seen = {}

    def fake(poses, edges, meas, info, fixed, iterations, huber_delta, pcg_tol, pcg_max_iter, ctx=None):
        seen.update(fixed=np.asarray(fixed).copy(), iterations=iterations, huber=huber_delta, tol=pcg_tol, max_iter=pcg_max_iter, ctx=ctx)
        return poses, {"status": 0}

    monkeypatch.setattr(pg, "optimize_pose_graph", fake)
    monkeypatch.setattr(backend.Backend, "ctx", property(lambda self: "the-context"))
    be = backend.Backend()                                   # still zero-argument constructible
    poses = np.tile(np.eye(4), (5, 1, 1))
    out, st = be.optimize_pose_graph(poses, [[0, 1]], np.eye(4)[None], np.eye(6)[None])
    assert out is poses and st == {"status": 0}
    assert seen["fixed"].tolist() == [1, 0, 0, 0, 0] and seen["fixed"].dtype == np.uint8          # the example fixes vertex 0
    assert (seen["iterations"], seen["huber"], seen["tol"], seen["max_iter"]) == (15, 0.0, pg.DEFAULT_PCG_TOL, pg.DEFAULT_PCG_MAX_ITER)
    assert seen["ctx"] == "the-context"
    be.optimize_pose_graph(poses, [[0, 1]], np.eye(4)[None], np.eye(6)[None], fixed=[1, 4], iterations=3, huber_delta=2.0)
    assert seen["fixed"].tolist() == [0, 1, 0, 0, 1] and seen["iterations"] == 3 and seen["huber"] == 2.0
    be.optimize_pose_graph(poses, [[0, 1]], np.eye(4)[None], np.eye(6)[None], fixed=np.array([False, False, True, False, False]))
    assert seen["fixed"].tolist() == [0, 0, 1, 0, 0]


def test_reference_defaults_match_the_product():
    from slamhip import pose_graph as pg

    assert (pg.DEFAULT_PCG_TOL, pg.DEFAULT_PCG_MAX_ITER, pg.DEFAULT_ITERATIONS) == (R.PCG_TOL, R.PCG_MAX_ITER, 15)


def test_plan_and_workspace_need_no_device(built):
    from slamhip import pose_graph as pg

    p = pg.plan(2500, 9849)
    assert p["launches_per_cg_iteration"] <= 3 and p["product_blocks"] == 63 and p["edge_blocks"] == 154
    big = pg.plan(100_000, 400_000)
    assert big["product_blocks"] == 512 and big["workspace_bytes"] > p["workspace_bytes"] > 0
    import ctypes
    import slamhip
    lib = slamhip.load()
    n = ctypes.c_uint64()
    assert lib.slam_pg_workspace(-1, 0, ctypes.byref(n)) == -1 and lib.slam_pg_workspace((1 << 24) + 1, 0, ctypes.byref(n)) == -1
    assert lib.slam_pg_workspace(1, (1 << 25) + 1, ctypes.byref(n)) == -1 and lib.slam_pg_workspace(1, 1, None) == -1
    assert lib.slam_pg_plan(0, 0, None) == -1
