"""GPU: the Sim(3) pose-graph kernels against the numpy reference of tests/sim3_graph_ref.py within the yardsticks that
tests/test_sim3_graph_cpu.py measures (linearisation and product 16x, the run of SOLVE_ITERATIONS iterations 4x), against the 80-digit truth
and the host twin on the truth file's edges, and at zero tolerance on the exactly-stated graphs of tests/sim3_graph_exact.py."""
import ctypes
import functools
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_ref as P  # noqa: E402
import sim3_graph_exact as X  # noqa: E402
import sim3_graph_ref as R  # noqa: E402
import sim3_graph_twin as TW  # noqa: E402
from test_pose_graph_cpu import HMUL_MARGIN, LIN_MARGIN, SOLVE_MARGIN, YARD_PCG_RECOMPUTE, rel  # noqa: E402
from test_pose_graph_cpu import YARD_SOLVE as YARD_SOLVE_SE3  # noqa: E402
from test_sim3_graph_cpu import (BAND_CUTS, GROUPS, QUANTITIES, SOLVE_ITERATIONS, YARD_HMUL, YARD_LIN, YARD_SOLVE, fixture, scene, truth_bound,  # noqa: E402
                                 twin_edges)

pytestmark = pytest.mark.gpu
SCENES = sorted(R.SMALL_SCENES)


@functools.lru_cache(maxsize=None)
def direct(name):
    s = scene(name)
    return R.optimize(s.init, s.edges, s.meas, s.info, s.fixed, iterations=SOLVE_ITERATIONS[name], solver="direct")


def run(s, ctx, **kw):
    import slamhip

    return slamhip.optimize_sim3_graph(s.init, s.edges, s.meas, s.info, s.fixed, ctx=ctx, **kw)


# ---------------------------------------------------------------- against the reference ------------------------------------------
@pytest.mark.parametrize("huber", [0.0, 3.0])
@pytest.mark.parametrize("name", SCENES)
def test_linearize_against_reference(gpu_ctx, name, huber):
    import slamhip

    s = scene(name)
    cost, b, Hd, W, status = slamhip.sim3_graph_linearize(s.init, s.edges, s.meas, s.info, huber, ctx=gpu_ctx)
    rc, rb, rHd, rW = R.linearize(s.init, s.edges, s.meas, s.info, huber)
    got = {"cost": abs(cost - rc) / rc, "grad": rel(b, rb), "Hdiag": rel(Hd, rHd), "W": rel(W, rW)}
    print(name, huber, got)
    assert status == 0
    for key, v in got.items():
        assert v <= LIN_MARGIN * YARD_LIN[key], (key, v)
    assert np.array_equal(Hd, np.swapaxes(Hd, 1, 2))


@pytest.mark.parametrize("name", SCENES)
def test_hmul_against_sparse_reference(gpu_ctx, name):
    import slamhip

    s = scene(name)
    _, _, Hd, W = R.linearize(s.init, s.edges, s.meas, s.info)
    H = R.assemble(s.V, s.edges, Hd, W)
    rng = np.random.default_rng(21)
    fixed_sets = [s.fixed, np.zeros(s.V, np.uint8), (rng.random(s.V) < 0.3).astype(np.uint8)]
    if name == "hub":
        only_hub = np.zeros(s.V, np.uint8)
        only_hub[0] = 1
        fixed_sets.append(only_hub)                       # the hub's row and column leave the system
    for fixed in fixed_sets:
        for lam in (0.0, 1e-3 * np.abs(Hd).max()):
            x = rng.normal(size=(s.V, 7))
            y = slamhip.sim3_graph_hmul(s.edges, fixed, Hd, W, lam, x, ctx=gpu_ctx)
            ry = R.hmul(H, fixed, lam, x)
            assert rel(y, ry) <= HMUL_MARGIN * YARD_HMUL, (name, int(fixed.sum()), lam, rel(y, ry))
            assert not y[fixed != 0].any()


@pytest.mark.parametrize("name", SCENES)
def test_pcg_meets_the_tolerance_it_was_asked_for(gpu_ctx, name):
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    import slamhip

    s = scene(name)
    _, b, Hd, W = R.linearize(s.init, s.edges, s.meas, s.info)
    H = R.assemble(s.V, s.edges, Hd, W)
    f = R.free_index(s.fixed)
    lam, tol = 1e-3 * np.abs(Hd).max(), 1e-8
    x, st = slamhip.sim3_graph_pcg(s.edges, s.fixed, Hd, W, b, lam, tol, 5000, ctx=gpu_ctx)
    bf = b.ravel()[f]
    res = float(np.linalg.norm(R.hmul(H, s.fixed, lam, x).ravel()[f] + bf) / np.linalg.norm(bf))
    print(name, st, "recomputed residual", res)
    assert st["converged"] and st["status"] == 0 and 0 < st["iterations"] < 5000
    assert res <= tol * YARD_PCG_RECOMPUTE
    assert not x[s.fixed != 0].any()
    exact = spla.spsolve((H[f][:, f] + lam * sp.identity(len(f))).tocsc(), -bf)
    assert np.linalg.norm(x.ravel()[f] - exact) <= (tol * YARD_PCG_RECOMPUTE + 1e-12) * np.linalg.norm(bf) / lam
    _, st2 = slamhip.sim3_graph_pcg(s.edges, s.fixed, Hd, W, b, lam, 1e-12, 3, ctx=gpu_ctx)
    assert st2["iterations"] == 3 and not st2["converged"]


@pytest.mark.parametrize("name", SCENES)
def test_full_run_against_reference_direct_lm(gpu_ctx, name):
    s = scene(name)
    S, st = run(s, gpu_ctx, iterations=SOLVE_ITERATIONS[name])
    Sd, sd = direct(name)
    ang, dist, ls = R.sim_gap(S, Sd)
    got = {"chi2": abs(st["chi2_final"] - sd["chi2_final"]) / sd["chi2_final"], "rotation": ang, "translation": dist / P.extent(s.gt),
           "log_scale": ls}
    print(name, st, got)
    for key, v in got.items():
        assert v <= SOLVE_MARGIN * YARD_SOLVE[name][key], (key, v)
    assert st["chi2_final"] < st["chi2_initial"] and abs(st["chi2_initial"] - sd["chi2_initial"]) <= 1e-12 * sd["chi2_initial"]
    assert st["trials"] == st["iterations"] == sd["iterations"] and st["cg_iterations"] <= st["trials"] * R.PCG_MAX_ITER
    assert st["status"] == 0 and abs(st["lam"] - sd["lam"]) <= 1e-6 * sd["lam"]
    assert np.array_equal(S[s.fixed != 0], s.init[s.fixed != 0])          # fixed vertices: bits unchanged
    assert S.shape == s.init.shape


# ---------------------------------------------------------------- against the truth and the twin ---------------------------------
def device_edges(ctx, fx, fam, delta):
    """the truth file's edges as one graph with a vertex pair per edge, so that the diagonal blocks and the gradient ARE the
    edges' shares; the cost of a single edge takes a call of its own and is sampled at every seventh edge (NaN elsewhere)"""
    import slamhip

    N = len(fx["r"])
    sims = np.concatenate([fx["Si"], fx["Sj"]])
    edges = np.stack([np.arange(N), N + np.arange(N)], 1).astype(np.int32)
    _, b, Hd, W, status = slamhip.sim3_graph_linearize(sims, edges, fx["Z"], fx["info_" + fam], delta, ctx=ctx)
    assert status == 0
    cost = np.full(N, np.nan)
    for n in range(0, N, 7):
        cost[n] = slamhip.sim3_graph_linearize(sims[[n, N + n]], np.array([[0, 1]], np.int32), fx["Z"][n:n + 1], fx["info_" + fam][n:n + 1], delta,
                                               ctx=ctx)[0]
    return dict(cost=cost, grad=np.concatenate([b[:N], b[N:]], 1), Hdiag=np.stack([Hd[:N], Hd[N:]], 1), W=W)


def test_device_against_truth_and_twin(gpu_ctx):
    """the truth file's edges: the device within 16x the reference's own distance to the 80-digit truth per angle band (the
    bound the host twin is held to on the CPU); and device against twin - the same source with different sin / cos / atan2 /
    log / exp underneath, so by tolerance - within that same bound of each other"""
    import test_sim3_graph_cpu as C

    fx = fixture()
    b = C.bands(fx)
    for g, fams in GROUPS.items():
        for fam in fams:
            for hub, delta in (("", 0.0), ("_huber", float(fx["delta_" + fam]))):
                got, truth, twin = device_edges(gpu_ctx, fx, fam, delta), C.truth_of(fx, fam, hub), twin_edges(fx, fam, delta)
                for q in QUANTITIES:
                    sel = ~np.isnan(got["cost"]) if q == "cost" else np.ones(len(b), bool)
                    t_, g_, w_ = (d[q][sel].reshape(sel.sum(), -1) for d in (truth, got, twin))
                    size = np.maximum(np.abs(t_).max(1), 1e-300)
                    err_truth, err_twin = np.abs(g_ - t_).max(1) / size, np.abs(g_ - w_).max(1) / size
                    for k in range(len(BAND_CUTS) + 1):
                        m = b[sel] == k
                        if m.any():
                            assert err_truth[m].max() <= truth_bound(g, q, k), (fam, hub, q, k, err_truth[m].max())
                            assert err_twin[m].max() <= truth_bound(g, q, k), (fam, hub, q, k, err_twin[m].max())


# ---------------------------------------------------------------- exactly-stated graphs, zero tolerance -----------------------------
@functools.lru_cache(maxsize=None)
def exact():
    return {g.name: g for g in X.exact_graphs()}


@pytest.mark.parametrize("name", [g.name for g in X.exact_graphs(big=False)] + ["chain18431", "chain18432", "chain18433"])
def test_exact_graphs_bit_for_bit(gpu_ctx, name):
    import slamhip

    g = exact()[name]
    cost, b, Hd, W, status = slamhip.sim3_graph_linearize(g.sims, g.edges, g.meas, g.info, ctx=gpu_ctx)
    ci, bi, Hi, Wi = g.linearize_int()
    assert status == 0 and cost == ci
    assert np.array_equal(b, bi) and np.array_equal(Hd, Hi) and np.array_equal(W, Wi)
    rng = np.random.default_rng(len(name))
    for fixed in g.masks:
        for lam in (0, 3):
            x = rng.integers(-4, 5, (g.V, 7))
            y = slamhip.sim3_graph_hmul(g.edges, fixed, Hi, Wi, float(lam), x.astype(float), ctx=gpu_ctx)
            assert np.array_equal(y, g.hmul_int(fixed, lam, x)), (name, int(fixed.sum()), lam)


def test_exact_graph_plan_boundaries():
    import slamhip.sim3_graph as G

    assert [G.plan(v, 1)["product_blocks"] for v in (9, 36, 37, 512 * 36 - 1, 512 * 36, 512 * 36 + 1)] == [1, 1, 2, 512, 512, 512]


# ---------------------------------------------------------------- fix_scale -----------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_fix_scale_returns_every_scale_bit_for_bit(gpu_ctx, name):
    s = scene(name)
    S, st = run(s, gpu_ctx, fix_scale=True)
    assert st["status"] == 0 and st["iterations"] >= 1 and st["chi2_final"] < st["chi2_initial"]
    assert np.array_equal(S[:, 12], s.init[:, 12])
    assert not np.array_equal(S[:, :12], s.init[:, :12])


def test_fix_scale_on_the_lifted_sphere_is_the_se3_optimiser(gpu_ctx):
    """the SE(3) suite's own sphere through lift_se3_graph with the scales frozen is the SE(3) problem (sigma's row and column are empty
    and the information is block diagonal): the poses agree with optimize_pose_graph on the unlifted graph within 4x the
    SE(3) suite's own sphere yardstick"""
    import slamhip

    s6 = P.sphere()                                                        # 2500 poses: the graph YARD_SOLVE["sphere"] was measured on
    sims, e, Z, info = slamhip.lift_se3_graph(s6.init, s6.edges, s6.meas, s6.info, scale_sigma=0.05)
    s7 = scene("sphere_s1")
    assert np.array_equal(sims, s7.init) and np.array_equal(Z, s7.meas) and np.array_equal(info, s7.info)      # the scene IS the lift
    S, st = slamhip.optimize_sim3_graph(sims, e, Z, info, s6.fixed, fix_scale=True, ctx=gpu_ctx)
    T6, st6 = slamhip.optimize_pose_graph(s6.init, s6.edges, s6.meas, s6.info, s6.fixed, ctx=gpu_ctx)
    ang, dist = P.pose_gap(S[:, :12], T6)
    got = {"chi2": abs(st["chi2_final"] - st6["chi2_final"]) / st6["chi2_final"], "rotation": ang, "translation": dist / P.extent(s6.gt)}
    print(st, st6, got)
    assert np.all(S[:, 12] == 1.0) and st["chi2_initial"] == st6["chi2_initial"] and st["status"] == 0
    for key, v in got.items():
        assert v <= SOLVE_MARGIN * YARD_SOLVE_SE3["sphere"][key], (key, v)


# ---------------------------------------------------------------- the feature, end to end -------------------------------------------
def test_drift_loop_through_the_public_api_and_the_gap_it_closes(gpu_ctx):
    """The tracker's SE(3) keyframe poses (its scale drifting by e^0.4 round the ring) lifted by lift_se3_graph, and all 66
    candidates - odometry, skip and closing edges - as estimate_sim3_batch reports them, (s, R, t) between the local maps of the
    two keyframes.  sim3_edges_from_sim3 keeps every one, and the 7-DoF graph brings the trajectory error below 1e-6 of its
    start.  loop_edges_from_sim3 on the same candidates drops the closing edge for its scale and flattens the others; the
    6-DoF graph over its output leaves more than half of the error.  (Odometry lifted with s = 1 cannot state this scene
    exactly: an edge (1, R, a t) against the true (e^eps, R, a t) leaves t_D = (1 - e^eps) a t at the truth.)"""
    import slamhip
    from backend import Backend

    s = R.drift_loop()
    poses0 = R.to_poses(s.init)                                            # every s = 1: the tracker's SE(3) keyframe poses
    none = (np.zeros((0, 2), np.int32), np.zeros((0, 3, 4)), np.zeros((0, 6, 6)))
    sims, e0, Z0, I0 = slamhip.lift_se3_graph(poses0, *none)
    sc, Rc, tc = slamhip.sim3_graph.split(s.meas)                          # (s, R, t) with X_j = s R X_i + t
    counts = np.full(s.E, 60)
    e7, Z7, I7 = slamhip.sim3_edges_from_sim3(s.edges, (sc, Rc, tc), counts)
    assert len(e7) == s.E and np.abs(np.log(Z7[:, 12])).max() > 0.35
    out, st = Backend().optimize_essential_graph(sims, np.concatenate([e0, e7]), np.concatenate([Z0, Z7]), np.concatenate([I0, I7]), fixed=(0,))
    before = P.trajectory_error(poses0, s.gt)
    after = P.trajectory_error(slamhip.sims_to_poses(out), s.gt)
    print(st, before, after)
    assert st["status"] == 0 and after < 1e-6 * before
    # the 6-DoF chain on the same candidates
    e6, Z6, I6, scales = slamhip.loop_edges_from_sim3(s.edges, (sc, Rc, tc), counts)
    assert len(e6) == s.E - 1 and np.abs(np.log(scales)).max() > 0.35
    T6, st6 = slamhip.optimize_pose_graph(poses0, e6, Z6, I6, s.fixed, ctx=gpu_ctx)
    after6 = P.trajectory_error(T6, s.gt)
    print(st6, after6)
    assert st6["status"] == 0 and after6 > 0.5 * before
    # map points follow their reference keyframes
    rng = np.random.default_rng(2)
    pts, ref = rng.normal(0, 4, (50, 3)), rng.integers(0, s.V, 50)
    moved = slamhip.correct_points(pts, ref, sims, out)
    want = R.parts(R.inv(out[ref]))
    cam = np.einsum("nij,nj->ni", sims[ref, :12].reshape(-1, 3, 4)[:, :, :3], pts) + sims[ref, :12].reshape(-1, 3, 4)[:, :, 3]
    assert np.allclose(moved, want[0][:, None] * np.einsum("nij,nj->ni", want[1], cam) + want[2], rtol=1e-12, atol=1e-12)


def test_input_forms(gpu_ctx):
    import slamhip

    s = scene("drift_loop")
    a, sa = run(s, gpu_ctx)
    parts = slamhip.sim3_graph.split(s.init)
    (s_, R_, t_), sb = slamhip.optimize_sim3_graph(parts, s.edges, slamhip.sim3_graph.split(s.meas), s.info, s.fixed, ctx=gpu_ctx)
    assert sa == sb and np.array_equal(s_, a[:, 12]) and np.array_equal(R_, a[:, :12].reshape(-1, 3, 4)[:, :, :3])
    assert np.array_equal(t_, a[:, :12].reshape(-1, 3, 4)[:, :, 3])


# ---------------------------------------------------------------- status and errors ---------------------------------------------------
def one_edge(ctx, Si=None, Sj=None, Z=None, Om=None, huber=0.0):
    import slamhip

    ident = R.pack(1.0, np.eye(4)[:3])
    sims = np.stack([ident if Si is None else Si, R.phi(np.array([0.1, 0.2, 0.0, 1, 2, 3, 0.3])) if Sj is None else Sj])
    return slamhip.sim3_graph_linearize(sims, np.array([[0, 1]], np.int32), (ident if Z is None else Z)[None],
                                        (np.eye(7) if Om is None else Om)[None], huber, ctx=ctx)


def finite_zeros(out):
    cost, b, Hd, W, _ = out
    return cost == 0.0 and not b.any() and not Hd.any() and not W.any()


def test_scale_status_for_every_bad_scale(gpu_ctx):
    ident = R.pack(1.0, np.eye(4)[:3])
    assert one_edge(gpu_ctx)[4] == 0
    for bad in (0.0, -2.0, np.inf, np.nan):
        S = ident.copy()
        S[12] = bad
        for kw in (dict(Si=S), dict(Sj=S), dict(Z=S)):                     # s_Z = NaN is among them
            out = one_edge(gpu_ctx, **kw)
            assert out[4] == 32 and finite_zeros(out), (bad, kw)
    big, tiny = ident.copy(), ident.copy()
    big[12], tiny[12] = 1e200, 1e-200
    out = one_edge(gpu_ctx, Si=tiny, Sj=big)                               # s_D overflows although every input scale is fine
    assert out[4] == 32 and finite_zeros(out)


def test_angle_and_nonfinite_status(gpu_ctx):
    ident = R.pack(1.0, np.eye(4)[:3])
    out = one_edge(gpu_ctx, Sj=ident, Z=R.phi(np.array([0.0, 0.0, 3.13, 0.1, 0.2, 0.3, 0.1])))
    assert out[4] == 2 and finite_zeros(out)
    for bad in (np.inf, np.nan):
        Om = np.eye(7)
        Om[2, 5] = Om[5, 2] = bad
        out = one_edge(gpu_ctx, Om=Om)
        assert out[4] == 16 and finite_zeros(out)


def test_precond_breakdown_and_index_status(gpu_ctx):
    import slamhip

    s = scene("drift_loop")
    _, b, Hd, W = R.linearize(s.init, s.edges, s.meas, s.info)
    bad = Hd.copy()
    bad[5] = -np.eye(7)                                                    # not positive definite: identity used, reported
    _, st = slamhip.sim3_graph_pcg(s.edges, s.fixed, bad, W, b, 0.0, 1e-8, 50, ctx=gpu_ctx)
    assert st["status"] & 4
    _, st = slamhip.sim3_graph_pcg(s.edges, s.fixed, -Hd, -W, b, 0.0, 1e-8, 50, ctx=gpu_ctx)      # negative definite: p.Ap <= 0
    assert st["status"] & 8 and not st["converged"]
    nb = b.copy()
    nb[7, 3] = np.nan
    _, st = slamhip.sim3_graph_pcg(s.edges, s.fixed, Hd, W, nb, 1.0, 1e-8, 50, ctx=gpu_ctx)
    assert st["status"] & 16 and not st["converged"]
    e = s.edges.copy()
    e[4, 1] = s.V
    with pytest.raises(slamhip.SlamHipError):                              # the index bit: refused
        slamhip.sim3_graph_linearize(s.init, e, s.meas, s.info, ctx=gpu_ctx)


def test_errors_through_the_abi(gpu_ctx):
    import slamhip
    from slamhip.pose_graph import vertex_lists

    lib, ctx = gpu_ctx.lib, gpu_ctx
    s = scene("drift_loop")
    V, E = s.V, s.E
    S, Z = np.ascontiguousarray(s.init), np.ascontiguousarray(s.meas)
    stats = np.zeros(8)
    p = lambda a: a.ctypes.data

    def host(edges, fixed, sims=S, V_=V, E_=E, out=None, it=15, tol=1e-8, mx=500):
        out = S.copy() if out is None else out
        rc = lib.slam_s3g_optimize_host_f64(ctx.handle, V_, E_, p(sims) if sims is not None else None, p(edges), p(Z), p(s.info), p(fixed), it, 0.0,
                                            tol, mx, 0, p(out), p(stats))
        return rc, out

    for where, value in (((17, 1), V), ((3, 0), -2)):                      # out of range, found on the device
        bad = s.edges.copy()
        bad[where] = value
        rc, out = host(bad, s.fixed)
        assert rc == -1 and b"edge index" in lib.slam_last_error() and np.array_equal(out, S)
    bad = s.edges.copy()
    bad[10] = (7, 7)                                                       # self-edge
    rc, out = host(bad, s.fixed)
    assert rc == -1 and np.array_equal(out, S)
    rc, out = host(s.edges, np.zeros(V, np.uint8))                         # no fixed vertex: before any launch
    assert rc == -1 and b"fixed vertex" in lib.slam_last_error() and np.array_equal(out, S)
    assert host(s.edges, s.fixed, sims=None)[0] == -1
    assert host(s.edges, s.fixed, V_=-1)[0] == -1 and host(s.edges, s.fixed, E_=-1)[0] == -1
    assert host(s.edges, s.fixed, V_=(1 << 24) + 1)[0] == -1 and host(s.edges, s.fixed, E_=(1 << 25) + 1)[0] == -1
    assert host(s.edges, s.fixed, it=-1)[0] == -1 and host(s.edges, s.fixed, tol=0.0)[0] == -1 and host(s.edges, s.fixed, mx=0)[0] == -1
    # V = 0 and E = 0 are not errors
    assert lib.slam_s3g_optimize_host_f64(ctx.handle, 0, 0, None, None, None, None, None, 15, 0.0, 1e-8, 500, 0, None, p(stats)) == 0
    rc, out = host(s.edges, s.fixed, E_=0, out=np.zeros_like(S))
    assert rc == 0 and np.array_equal(out, S) and stats[3] == 0
    out, st = slamhip.optimize_sim3_graph(np.zeros((0, 13)), np.zeros((0, 2), np.int32), np.zeros((0, 13)), np.zeros((0, 7, 7)), np.zeros(0))
    assert out.shape == (0, 13) and st["trials"] == 0
    # the device form: a vertex list that does not match the edges is refused, the output untouched
    ptr, adj = vertex_lists(V, s.edges)
    wrong = adj.copy()
    wrong[40] = wrong[41]
    bufs = [ctx.upload(a) for a in (S, s.edges, Z, s.info, s.fixed, ptr, wrong, adj)]
    dS, de, dZ, dO, df, dp, dbad, dgood = bufs
    dout = ctx.upload(np.zeros_like(S))
    try:
        args = lambda da, nf: (ctx.handle, V, E, dS.ptr, de.ptr, dZ.ptr, dO.ptr, df.ptr, nf, dp.ptr, da.ptr, 15, 0.0, 1e-8, 500, 0, dout.ptr, p(stats))
        assert lib.slam_s3g_optimize_f64(*args(dbad, 1)) == -1 and not dout.download(np.float64, S.shape).any()
        assert lib.slam_s3g_optimize_f64(*args(dgood, 2)) == -1 and b"n_fixed" in lib.slam_last_error()
        assert lib.slam_s3g_optimize_f64(*args(dgood, 0)) == -1
        assert lib.slam_s3g_optimize_f64(*args(dgood, 1)) == 0
        ref, _ = run(s, gpu_ctx)
        assert np.array_equal(dout.download(np.float64, S.shape), ref)                                    # device form == host form
        status = ctypes.c_int32(0)
        assert lib.slam_s3g_linearize_f64(ctx.handle, V, E, dS.ptr, de.ptr, dZ.ptr, dO.ptr, dp.ptr, dgood.ptr, -1.0, dout.ptr, dout.ptr, dout.ptr,
                                          dout.ptr, ctypes.byref(status)) == -1
        assert lib.slam_s3g_hmul_f64(ctx.handle, V, E, de.ptr, dp.ptr, dgood.ptr, df.ptr, None, dout.ptr, 0.0, dout.ptr, dout.ptr) == -1
        assert lib.slam_s3g_pcg_f64(ctx.handle, V, E, de.ptr, dp.ptr, dgood.ptr, df.ptr, dout.ptr, dout.ptr, dout.ptr, 0.0, 0.0, 10, dout.ptr, p(stats)) == -1
    finally:
        for b_ in bufs + [dout]:
            b_.free()
    with pytest.raises(slamhip.SlamHipError):
        slamhip.optimize_sim3_graph(s.init, bad, s.meas, s.info, s.fixed, ctx=gpu_ctx)


# ---------------------------------------------------------------- determinism ---------------------------------------------------------
def lift_multi_hub():
    base = P.multi_hub()
    return R._lift(base, "multi_hub", np.random.default_rng(31), 0.05)


def test_determinism_two_runs_two_contexts_and_seventy_hubs():
    import slamhip

    s, h = scene("drift_loop"), lift_multi_hub()
    _, b, Hd, W = R.linearize(h.init, h.edges, h.meas, h.info)
    lam = 1e-3 * np.abs(Hd).max()
    x = np.random.default_rng(4).normal(size=(h.V, 7))
    runs, prods = [], []
    for _ in range(2):
        ctx = slamhip.Context(0)
        try:
            for _ in range(2):
                runs.append(run(s, ctx) + run(h, ctx))
            for _ in range(5):
                prods.append(slamhip.sim3_graph_hmul(h.edges, h.fixed, Hd, W, lam, x, ctx=ctx))
        finally:
            ctx.close()
    for r_ in runs[1:]:
        assert np.array_equal(r_[0], runs[0][0]) and r_[1] == runs[0][1] and np.array_equal(r_[2], runs[0][2]) and r_[3] == runs[0][3]
    assert len(prods) == 10 and all(np.array_equal(y, prods[0]) for y in prods[1:])
    H = R.assemble(h.V, h.edges, Hd, W)
    assert rel(prods[0], R.hmul(H, h.fixed, lam, x)) <= HMUL_MARGIN * YARD_HMUL
    # the run ends at the scene's optimum (the reference: 7 accepted iterations, then ten trials turned down), where chi2 is
    # stationary: what is left between two correct runs is the rounding of a sum of E terms
    _, ref = R.optimize(h.init, h.edges, h.meas, h.info, h.fixed)
    st = runs[0][3]
    print(st, ref)
    assert st["status"] == 0 and st["chi2_final"] < st["chi2_initial"]
    for key in ("chi2_initial", "chi2_final"):
        assert abs(st[key] - ref[key]) <= h.E * 2.0 ** -53 * ref[key], key


def test_one_context_two_threads():
    import slamhip

    ctx = slamhip.Context(0)
    try:
        graphs = [scene("drift_loop"), scene("hub")]
        alone = [run(g, ctx) for g in graphs]
        results, errors = [None, None], []

        def work(k):
            try:
                for _ in range(3):
                    results[k] = run(graphs[k], ctx)
                    slamhip.sim3_graph_hmul(graphs[k].edges, graphs[k].fixed, np.tile(np.eye(7), (graphs[k].V, 1, 1)),
                                            np.zeros((graphs[k].E, 7, 7)), 0.5, np.ones((graphs[k].V, 7)), ctx=ctx)
            except Exception as exc:      # noqa: BLE001
                errors.append(exc)

        threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        for k in range(2):
            assert np.array_equal(results[k][0], alone[k][0]) and results[k][1] == alone[k][1]
    finally:
        ctx.close()
