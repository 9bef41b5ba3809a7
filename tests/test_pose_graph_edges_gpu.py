"""GPU: the pose-graph kernels over their whole contract against truth that shares none of their formulas
(tests/pose_graph_truth.py): 80-digit linearisations per angle band and information family, integer graphs at zero tolerance
across every launch boundary, all five status bits, degenerate graphs, and the CG loop's bookkeeping.  The bounds are the
yardsticks tests/test_pose_graph_edges_cpu.py measures, times the margins of tests/test_pose_graph_cpu.py."""
import functools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_ref as R  # noqa: E402
import pose_graph_truth as T  # noqa: E402
from test_pose_graph_cpu import HMUL_MARGIN, LIN_MARGIN, SOLVE_MARGIN, rel  # noqa: E402
from test_pose_graph_edges_cpu import (CG_STEPS, EDGE_PCG_MAX_ITER, K_RANGES, YARD_CG, YARD_SOLVE_EDGES, YARD_TRUTH, cg_system,  # noqa: E402
                                       edge_scene, edge_solved, fixture, k_system, yard_group)

pytestmark = pytest.mark.gpu
NB = len(T.BAND_CUTS) + 1


def pcg(ctx, edges, fixed, Hd, W, b, lam, tol, max_iter):
    """pose_graph_pcg, with the promise every call in this file is held to: converged <=> a finite relres <= tol"""
    import slamhip

    x, st = slamhip.pose_graph_pcg(edges, fixed, Hd, W, b, lam, tol, max_iter, ctx=ctx)
    met = bool(np.isfinite(st["relres"]) and st["relres"] <= tol)
    assert st["converged"] == met, (st, tol)
    return x, st


@functools.lru_cache(maxsize=None)
def graphs():
    return T.exact_graphs()


# ---------------------------------------------------------------- 1. linearisation against truth --------------------------------
def check_bands(g, b, Hd, W, tag, family):
    yard = YARD_TRUTH[yard_group(family)]
    errs = T.edge_errors(g, b, Hd, W)
    live = ~g["dead"]
    for key, err in errs.items():
        worst = T.band_max(g["angle"], err, live)
        print(tag, key, " ".join(f"{v:.2e}" for v in worst))
        for band in range(NB):
            assert worst[band] <= LIN_MARGIN * yard[key][band], (tag, key, band, worst[band])


@pytest.mark.parametrize("huber", [0, 1])
@pytest.mark.parametrize("family", T.FAMILIES)
def test_linearize_against_mpmath_truth(gpu_ctx, family, huber):
    import slamhip

    fx = fixture()
    g = T.truth_graph(fx, family, huber)
    cost, b, Hd, W, status = slamhip.pose_graph_linearize(g["poses"], g["edges"], g["meas"], g["info"], g["huber"], ctx=gpu_ctx)
    assert status == 0
    check_bands(g, b, Hd, W, f"{family} huber={g['huber']:g}", family)
    assert np.array_equal(Hd, np.swapaxes(Hd, 1, 2))
    live = np.flatnonzero(~fx["beyond"])
    bands = np.array([T.band_of(a) for a in g["angle"]])
    for band in range(NB):                                            # the cost, per band: the graph of that band's edges
        gb = T.truth_graph(fx, family, huber, live[bands == band])
        c, _, _, _, st = slamhip.pose_graph_linearize(gb["poses"], gb["edges"], gb["meas"], gb["info"], gb["huber"], ctx=gpu_ctx)
        err = abs(c - gb["cost"]) / gb["cost"]
        print(f"{family} huber={g['huber']:g} cost band {band}: {err:.2e}")
        assert st == 0 and err <= LIN_MARGIN * YARD_TRUTH[yard_group(family)]["cost"][band], (band, err)


@pytest.mark.parametrize("family", ["spd1e4", "rot_only"])
def test_edges_beyond_the_contract_leave_the_sums(gpu_ctx, family):
    import slamhip

    fx = fixture()
    g = T.truth_graph(fx, family, 1, np.arange(len(fx["xi"])))       # every sample: the 18 beyond 3.1 rad mixed in
    dead = g["dead"]
    assert dead.sum() == 18
    cost, b, Hd, W, status = slamhip.pose_graph_linearize(g["poses"], g["edges"], g["meas"], g["info"], g["huber"], ctx=gpu_ctx)
    assert status == 2
    d = np.flatnonzero(dead)
    for a in (W[d], Hd[2 * d], Hd[2 * d + 1], b[2 * d], b[2 * d + 1]):
        assert not a.any() and np.isfinite(a).all()                   # exactly zero
    check_bands(g, b, Hd, W, f"{family} mixed", family)
    err = abs(cost - g["cost"]) / g["cost"]
    print(family, "mixed cost", err)
    assert err <= LIN_MARGIN * max(YARD_TRUTH[yard_group(family)]["cost"])


# ---------------------------------------------------------------- 2. exact graphs, zero tolerance ------------------------------
def test_exact_graphs_linearize_and_product_bit_for_bit(gpu_ctx):
    import slamhip

    for g in graphs():
        cost, b, Hd, W, status = slamhip.pose_graph_linearize(g.poses, g.edges, g.meas, g.info, 0.0, ctx=gpu_ctx)
        tc, tb, tH, tW = g.linearize_int()
        assert status == 0 and cost == tc, g.name
        assert np.array_equal(b, tb) and np.array_equal(Hd, tH) and np.array_equal(W, tW), g.name
        pH, pW, x, lam = g.product_inputs()
        for k, fixed in enumerate(g.masks):
            y = slamhip.pose_graph_hmul(g.edges, fixed, pH, pW, lam, x, ctx=gpu_ctx)
            assert np.array_equal(y, g.hmul_int(fixed, pH, pW, lam, x)), (g.name, k)
        print(g.name, "V", g.V, "E", g.E, "cost", cost, "masks", len(g.masks), "exact")


def test_exact_graphs_solve_and_optimize_repeat_bit_for_bit(gpu_ctx):
    import slamhip

    for g in graphs():
        _, tb, tH, tW = g.linearize_int()
        fixed = g.masks[0]
        for k, mask in enumerate(g.masks):             # every mask through the CG vector kernels: fixed hubs, hubs with fixed neighbours
            a = pcg(gpu_ctx, g.edges, mask, tH, tW, tb, 1.0, 1e-8, 200)
            c = pcg(gpu_ctx, g.edges, mask, tH, tW, tb, 1.0, 1e-8, 200)
            assert np.array_equal(a[0], c[0]) and a[1] == c[1] and np.isfinite(a[0]).all() and not a[0][mask != 0].any(), (g.name, k)
            if 0 < mask.sum() < g.V and k in (0, len(g.masks) - 2):
                Pm, sm = slamhip.optimize_pose_graph(g.poses, g.edges, g.meas, g.info, mask, iterations=2, ctx=gpu_ctx)
                Pm2, sm2 = slamhip.optimize_pose_graph(g.poses, g.edges, g.meas, g.info, mask, iterations=2, ctx=gpu_ctx)
                assert np.array_equal(Pm, Pm2) and sm == sm2 and np.array_equal(Pm[mask != 0], g.poses[mask != 0]), (g.name, k)
        P, st = slamhip.optimize_pose_graph(g.poses, g.edges, g.meas, g.info, fixed, iterations=3, ctx=gpu_ctx)
        P2, st2 = slamhip.optimize_pose_graph(g.poses, g.edges, g.meas, g.info, fixed, iterations=3, ctx=gpu_ctx)
        assert np.array_equal(P, P2) and st == st2 and st["status"] == 0 and np.isfinite(P).all(), g.name
        assert st["chi2_final"] <= st["chi2_initial"] and np.array_equal(P[0], g.poses[0])
        print(g.name, a[1], st)


# ---------------------------------------------------------------- 3. status bits ----------------------------------------------
def test_status_precond(gpu_ctx):
    from slamhip import pose_graph as pg

    Hd = np.tile(np.eye(6), (3, 1, 1))
    Hd[1] = np.diag([1.0, 1, 1, 0, 0, 0])                             # positive semi-definite, singular
    b = np.ones((3, 6))
    b[1, 3:] = 0                                                      # consistent: the system has a solution
    e = np.zeros((0, 2), np.int32)
    x, st = pcg(gpu_ctx, e, np.zeros(3, np.uint8), Hd, np.zeros((0, 6, 6)), b, 0.0, 1e-8, 50)
    print("precond, free vertex:", st)
    assert st["status"] & 4 and pg.status_names(st["status"]) == ["precond"] and np.isfinite(x).all() and st["converged"]
    assert np.allclose(x[[0, 2]], -1) and np.allclose(x[1], [-1, -1, -1, 0, 0, 0])
    x, st = pcg(gpu_ctx, e, np.array([0, 1, 0], np.uint8), Hd, np.zeros((0, 6, 6)), b, 0.0, 1e-8, 50)
    print("precond, fixed vertex:", st)
    assert st["status"] == 0 and st["converged"] and not x[1].any()


def test_status_breakdown(gpu_ctx):
    Hd = np.tile(np.eye(6), (2, 1, 1))
    W = 2 * np.eye(6)[None]                                          # A = [[I, 2I], [2I, I]]: eigenvalues 3 and -1
    r = np.concatenate([np.arange(1.0, 7), -np.arange(1.0, 7)]).reshape(2, 6)      # r^T A r = -|r|^2
    x, st = pcg(gpu_ctx, np.array([[0, 1]], np.int32), np.zeros(2, np.uint8), Hd, W, -r, 0.0, 1e-8, 50)
    print("breakdown:", st)
    assert st["status"] == 8 and st["iterations"] == 0 and np.isfinite(x).all() and not st["converged"] and st["relres"] == 1.0


def test_status_nonfinite(gpu_ctx):
    import slamhip

    fx = fixture()
    g = T.truth_graph(fx, "spd1e4", 0)
    info = g["info"].copy()
    e0 = 40
    info[e0, 2, 3] = info[e0, 3, 2] = np.inf
    cost, b, Hd, W, status = slamhip.pose_graph_linearize(g["poses"], g["edges"], g["meas"], info, 0.0, ctx=gpu_ctx)
    print("inf in Omega: status", status)
    assert status == 16
    # the reported edge leaves the sums like one beyond the angle contract: finite zeros, and the cost excludes it
    for a in (W[e0], Hd[2 * e0], Hd[2 * e0 + 1], b[2 * e0], b[2 * e0 + 1]):
        assert not a.any() and np.isfinite(a).all()
    g["dead"] = np.arange(len(g["dead"])) == e0
    check_bands(g, b, Hd, W, "inf in Omega", "spd1e4")
    want = math.fsum(np.delete(g["rho"], e0))
    assert abs(cost - want) / want <= LIN_MARGIN * max(YARD_TRUTH["general"]["cost"])
    # a NaN in b
    s, Hd, W, b, lam = k_system("k32")
    bad = b.copy()
    bad[7, 2] = np.nan
    x, st = pcg(gpu_ctx, s.edges, s.fixed, Hd, W, bad, lam, 1e-8, 50)
    print("NaN in b:", st)
    assert st["status"] & 16 and not st["converged"] and st["iterations"] == 0 and not np.isfinite(st["relres"])
    # a NaN pose
    P0 = s.init.copy()
    P0[5, 1, 2] = np.nan
    P, st = slamhip.optimize_pose_graph(P0, s.edges, s.meas, s.info, s.fixed, ctx=gpu_ctx)
    print("NaN pose:", st)
    assert st["trials"] == 0 and st["iterations"] == 0 and st["status"] != 0 and P.tobytes() == P0.tobytes()


# ---------------------------------------------------------------- 4. degenerate graphs -----------------------------------------
def test_degenerate_graphs(gpu_ctx):
    import slamhip
    from slamhip.pose_graph import vertex_lists

    s = R.loop_closure(n=40, closures=4)
    run = lambda fixed, **kw: slamhip.optimize_pose_graph(s.init, s.edges, s.meas, s.info, fixed, ctx=gpu_ctx, **kw)
    P, st = run(np.ones(s.V, np.uint8))                               # all fixed
    print("all fixed:", st)
    assert P.tobytes() == s.init.tobytes() and st["status"] == 0 and st["iterations"] == 0 and st["chi2_final"] == st["chi2_initial"]
    P, st = run(s.fixed, iterations=0)
    assert P.tobytes() == s.init.tobytes() and st["chi2_final"] == st["chi2_initial"] > 0 and st["trials"] == 0 and st["status"] == 0
    # an isolated free vertex (no edge names it) comes back as it went in, while the rest moves
    poses = np.concatenate([s.init, R.exp_se3(np.array([[0.3, -0.2, 0.5, 1.5, -2.5, 3.5]]))])
    P, st = slamhip.optimize_pose_graph(poses, s.edges, s.meas, s.info, np.append(s.fixed, 0), ctx=gpu_ctx)
    P1, st1 = run(s.fixed)
    print("isolated vertex:", st)
    assert np.array_equal(P[-1], poses[-1]) and st["status"] == 0 and st["chi2_final"] < 0.1 * st["chi2_initial"]
    assert np.array_equal(P[:-1], P1) and st == st1                   # and changes nothing for the others
    # V = 2, E = 1: the free pose lands on the measurement
    Z = R.exp_se3(np.array([[0.4, 0.1, -0.3, 1.0, 2.0, -1.0]]))
    two = np.tile(np.eye(4)[:3], (2, 1, 1))
    P, st = slamhip.optimize_pose_graph(two, np.array([[0, 1]], np.int32), Z, np.eye(6)[None], np.array([1, 0], np.uint8), ctx=gpu_ctx)
    print("V=2:", st)
    assert st["status"] == 0 and np.abs(P[1] - Z[0]).max() < 1e-9 and np.array_equal(P[0], two[0]) and st["chi2_final"] < 1e-18
    # E = 0 through the device form
    V = 11
    T12 = np.ascontiguousarray(s.init[:V].reshape(V, 12))
    fixed = np.zeros(V, np.uint8)
    fixed[3] = 1
    ptr, _ = vertex_lists(V, np.zeros((0, 2), np.int32))
    bufs = [gpu_ctx.upload(a) for a in (T12, fixed, ptr, np.zeros_like(T12))]
    stats = np.ones(8)
    try:
        rc = gpu_ctx.lib.slam_pg_optimize_f64(gpu_ctx.handle, V, 0, bufs[0].ptr, None, None, None, bufs[1].ptr, 1, bufs[2].ptr, None, 15, 0.0,
                                              1e-8, 500, bufs[3].ptr, stats.ctypes.data)
        assert rc == 0 and not stats.any()
        assert bufs[3].download(np.float64, T12.shape).tobytes() == T12.tobytes()
    finally:
        for b_ in bufs:
            b_.free()


@pytest.mark.parametrize("name", sorted(YARD_SOLVE_EDGES))
def test_full_run_with_realistic_information(gpu_ctx, name):
    import slamhip

    s = edge_scene(name)
    P, st = slamhip.optimize_pose_graph(s.init, s.edges, s.meas, s.info, s.fixed, pcg_max_iter=EDGE_PCG_MAX_ITER[name], ctx=gpu_ctx)
    Pd, sd, _ = edge_solved(name, "direct")
    got = {"chi2": abs(st["chi2_final"] - sd["chi2_final"]) / sd["chi2_final"]}
    if name == "full_info":
        ang, dist = R.pose_gap(P, Pd)
        got.update(rotation=ang, translation=dist / R.extent(s.gt))
    print(name, st, got)
    assert st["status"] == 0 and abs(st["chi2_initial"] - sd["chi2_initial"]) <= 1e-12 * sd["chi2_initial"]
    for key, v in got.items():
        assert v <= SOLVE_MARGIN * YARD_SOLVE_EDGES[name][key], (key, v)
    assert np.array_equal(P[s.fixed != 0], s.init[s.fixed != 0])


# ---------------------------------------------------------------- 5. CG bookkeeping --------------------------------------------
def test_cg_iteration_counts_and_iterates_against_longdouble(gpu_ctx):
    s, Hd, W, b, lam = cg_system()
    _, _, _, ref = T.pcg_blocks(s.edges, s.fixed, Hd, W, b, lam, 1e-30, max(CG_STEPS), np.longdouble, CG_STEPS)
    for m in CG_STEPS:
        x, st = pcg(gpu_ctx, s.edges, s.fixed, Hd, W, b, lam, 1e-30, m)
        ex, er = rel(x, ref[m][0].astype(np.float64)), abs(st["relres"] - ref[m][1]) / ref[m][1]
        print(f"m={m}: {st} x {ex:.2e} relres {er:.2e}")
        assert st["iterations"] == m and not st["converged"] and st["status"] == 0
        assert ex <= HMUL_MARGIN * YARD_CG["x"] and er <= HMUL_MARGIN * YARD_CG["relres"], (m, ex, er)


@pytest.mark.parametrize("which", sorted(K_RANGES))
def test_cg_converging_next_to_a_read_back_point(gpu_ctx, which):
    """k iterations to 1e-8 with k next to 32 or 64, where the host reads the done flag: the launches queued behind the
    converging iteration must be no-ops, and a cap of exactly k must give the same bits"""
    s, Hd, W, b, lam = k_system(which)
    f = R.free_index(s.fixed)
    _, k_ref, _ = R.pcg(R.assemble(s.V, s.edges, Hd, W)[f][:, f].tocsr(), b.ravel()[f], lam, 1e-8, 5000)
    x, st = pcg(gpu_ctx, s.edges, s.fixed, Hd, W, b, lam, 1e-8, 5000)
    k = st["iterations"]
    print(which, "reference k", k_ref, "device", st)
    assert st["converged"] and st["status"] == 0 and abs(k - k_ref) <= 1 and K_RANGES[which][0] <= k_ref <= K_RANGES[which][1]
    x2, st2 = pcg(gpu_ctx, s.edges, s.fixed, Hd, W, b, lam, 1e-8, k)
    assert np.array_equal(x, x2) and st2 == st
    for cap in (k + 1, 32 * ((k + 31) // 32), 32 * ((k + 31) // 32) + 1):
        x3, st3 = pcg(gpu_ctx, s.edges, s.fixed, Hd, W, b, lam, 1e-8, cap)
        assert np.array_equal(x, x3) and st3 == st, cap
    _, st4 = pcg(gpu_ctx, s.edges, s.fixed, Hd, W, b, lam, 1e-8, k - 1)
    assert st4["iterations"] == k - 1 and not st4["converged"]
