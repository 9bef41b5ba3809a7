"""GPU: the pose-graph kernels against the numpy reference of tests/pose_graph_ref.py, within the yardsticks that
tests/test_pose_graph_cpu.py measures (linearisation and product 16x, the 15-iteration run 4x)."""
import ctypes
import functools
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_ref as R  # noqa: E402
from test_pose_graph_cpu import (HMUL_MARGIN, LIN_MARGIN, SOLVE_MARGIN, YARD_HMUL, YARD_LIN, YARD_PCG_RECOMPUTE,  # noqa: E402
                                 YARD_SOLVE, rel, scene)

pytestmark = pytest.mark.gpu
SCENES = sorted(R.SMALL_SCENES)


@functools.lru_cache(maxsize=None)
def direct(name):
    s = scene(name)
    return R.optimize(s.init, s.edges, s.meas, s.info, s.fixed, solver="direct")


def run(s, ctx, **kw):
    import slamhip

    return slamhip.optimize_pose_graph(s.init, s.edges, s.meas, s.info, s.fixed, ctx=ctx, **kw)


@pytest.mark.parametrize("huber", [0.0, 3.0])
@pytest.mark.parametrize("name", SCENES)
def test_linearize_against_reference(gpu_ctx, name, huber):
    import slamhip

    s = scene(name)
    cost, b, Hd, W, status = slamhip.pose_graph_linearize(s.init, s.edges, s.meas, s.info, huber, ctx=gpu_ctx)
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
            x = rng.normal(size=(s.V, 6))
            y = slamhip.pose_graph_hmul(s.edges, fixed, Hd, W, lam, x, ctx=gpu_ctx)
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
    x, st = slamhip.pose_graph_pcg(s.edges, s.fixed, Hd, W, b, lam, tol, 5000, ctx=gpu_ctx)
    bf = b.ravel()[f]
    res = float(np.linalg.norm(R.hmul(H, s.fixed, lam, x).ravel()[f] + bf) / np.linalg.norm(bf))
    print(name, st, "recomputed residual", res)
    assert st["converged"] and st["status"] == 0 and 0 < st["iterations"] < 5000
    assert res <= tol * YARD_PCG_RECOMPUTE
    assert not x[s.fixed != 0].any()
    exact = spla.spsolve((H[f][:, f] + lam * sp.identity(len(f))).tocsc(), -bf)
    # |x - x*| <= |A^-1| |residual| and |A^-1| <= 1 / lam: the distance to the direct solve in units of |b| / lam
    assert np.linalg.norm(x.ravel()[f] - exact) <= (tol * YARD_PCG_RECOMPUTE + 1e-12) * np.linalg.norm(bf) / lam
    # an iteration cap that is too small is reported, not hidden
    _, st2 = slamhip.pose_graph_pcg(s.edges, s.fixed, Hd, W, b, lam, 1e-12, 3, ctx=gpu_ctx)
    assert st2["iterations"] == 3 and not st2["converged"]


@pytest.mark.parametrize("name", SCENES)
def test_full_run_against_reference_direct_lm(gpu_ctx, name):
    s = scene(name)
    P, st = run(s, gpu_ctx)
    Pd, sd = direct(name)
    ang, dist = R.pose_gap(P, Pd)
    got = {"chi2": abs(st["chi2_final"] - sd["chi2_final"]) / sd["chi2_final"], "rotation": ang, "translation": dist / R.extent(s.gt)}
    print(name, st, got)
    for key, v in got.items():
        assert v <= SOLVE_MARGIN * YARD_SOLVE[name][key], (key, v)
    assert st["chi2_final"] < st["chi2_initial"] and abs(st["chi2_initial"] - sd["chi2_initial"]) <= 1e-12 * sd["chi2_initial"]
    assert st["trials"] >= st["iterations"] >= 1 and st["cg_iterations"] <= st["trials"] * R.PCG_MAX_ITER
    assert st["status"] == 0 and st["lam"] > 0
    assert np.array_equal(P[s.fixed != 0], s.init[s.fixed != 0])          # fixed poses: bits unchanged
    assert P.shape == s.init.shape


def test_pose_formats_and_backend(gpu_ctx):
    import slamhip
    from backend import Backend

    s = scene("loop_closure")
    P34, st = run(s, gpu_ctx)
    P12, _ = slamhip.optimize_pose_graph(s.init.reshape(-1, 12), s.edges, s.meas.reshape(-1, 12), s.info, s.fixed, ctx=gpu_ctx)
    full = np.tile(np.eye(4), (s.V, 1, 1))
    full[:, :3] = s.init
    Zf = np.tile(np.eye(4), (s.E, 1, 1))
    Zf[:, :3] = s.meas
    P44, st44 = Backend().optimize_pose_graph(full, s.edges, Zf, s.info)
    assert P12.shape == (s.V, 12) and P44.shape == (s.V, 4, 4)
    assert np.array_equal(P12.reshape(-1, 3, 4), P34) and np.array_equal(P44[:, :3], P34) and np.array_equal(P44[:, 3], full[:, 3])
    assert st44 == st


def test_determinism_and_workspace_growth():
    """the same call twice, and the same graph after a larger one has grown (and dirtied) the workspace: identical bits"""
    import slamhip

    ctx = slamhip.Context(0)
    try:
        small, big = scene("loop_closure"), scene("sphere")
        a, sa = run(small, ctx)
        b, sb = run(small, ctx)
        grown_from = ctx.block_bytes()["workspace"]
        run(big, ctx)
        assert ctx.block_bytes()["workspace"] > grown_from
        c, sc = run(small, ctx)
        assert np.array_equal(a, b) and np.array_equal(a, c) and sa == sb == sc
        h, sh = run(scene("hub"), ctx)
        h2, sh2 = run(scene("hub"), ctx)
        assert np.array_equal(h, h2) and sh == sh2
    finally:
        ctx.close()


def test_many_hubs_same_bits_every_run():
    """70 hub vertices (more than the 64 waves that walk the hub list, so the grid stride is covered): the hub list is in
    vertex order whatever order the set-up's lanes finish in, so p.q, the iteration counts and the poses repeat bit for bit,
    on one context and across fresh ones.  The product and the solve are also held to the reference here."""
    import slamhip

    s = R.multi_hub()
    _, b, Hd, W = R.linearize(s.init, s.edges, s.meas, s.info)
    H = R.assemble(s.V, s.edges, Hd, W)
    lam = 1e-3 * np.abs(Hd).max()
    rng = np.random.default_rng(4)
    x = rng.normal(size=(s.V, 6))
    runs = []
    for _ in range(3):
        ctx = slamhip.Context(0)
        try:
            for _ in range(2):
                P, st = run(s, ctx)
                xs, ps = slamhip.pose_graph_pcg(s.edges, s.fixed, Hd, W, b, lam, 1e-8, 5000, ctx=ctx)
                y = slamhip.pose_graph_hmul(s.edges, s.fixed, Hd, W, lam, x, ctx=ctx)
                runs.append((P, st, xs, ps, y))
        finally:
            ctx.close()
    P0, st0, xs0, ps0, y0 = runs[0]
    for P, st, xs, ps, y in runs[1:]:
        assert np.array_equal(P, P0) and st == st0 and np.array_equal(xs, xs0) and ps == ps0 and np.array_equal(y, y0)
    print(st0, ps0, rel(y0, R.hmul(H, s.fixed, lam, x)))
    assert st0["status"] == 0 and st0["chi2_final"] < 0.1 * st0["chi2_initial"] and st0["cg_iterations"] > 0
    assert rel(y0, R.hmul(H, s.fixed, lam, x)) <= HMUL_MARGIN * YARD_HMUL
    f = R.free_index(s.fixed)
    bf = b.ravel()[f]
    assert ps0["converged"] and ps0["status"] == 0
    assert np.linalg.norm(R.hmul(H, s.fixed, lam, xs0).ravel()[f] + bf) / np.linalg.norm(bf) <= 1e-8 * YARD_PCG_RECOMPUTE


@pytest.mark.parametrize("name", SCENES)
def test_graph_at_its_optimum_stays_there(gpu_ctx, name):
    s = R.noise_free(scene(name))
    P, st = run(s, gpu_ctx)
    ang, dist = R.pose_gap(P, s.init)
    chi2_scale = float(np.abs(s.info).max()) * s.E          # chi2 of residuals of size 1
    print(name, st, ang, dist)
    assert st["status"] == 0
    # residuals of exact measurements are rounding (1e-16 * coordinates of the size of the extent): chi2 stays at that level
    assert st["chi2_final"] <= st["chi2_initial"] <= chi2_scale * (1e-15 * R.extent(s.gt)) ** 2 * 1e4
    assert ang <= LIN_MARGIN * YARD_LIN["grad"] and dist <= LIN_MARGIN * YARD_LIN["grad"] * R.extent(s.gt)
    assert np.array_equal(P[s.fixed != 0], s.init[s.fixed != 0])


def test_huber_resists_wrong_closures(gpu_ctx):
    s = R.loop_closure(outlier_fraction=0.1)
    plain, st0 = run(s, gpu_ctx, huber_delta=0.0)
    robust, st1 = run(s, gpu_ctx, huber_delta=3.0)
    e0, e1 = R.trajectory_error(plain, s.gt), R.trajectory_error(robust, s.gt)
    print("trajectory error without / with Huber:", e0, e1)
    assert st0["status"] == 0 and st1["status"] == 0
    assert e1 < e0


def test_errors_through_the_abi(gpu_ctx):
    import slamhip

    lib, ctx = gpu_ctx.lib, gpu_ctx
    s = scene("loop_closure")
    V, E = s.V, s.E
    T = np.ascontiguousarray(s.init.reshape(V, 12))
    Z = np.ascontiguousarray(s.meas.reshape(E, 12))
    stats = np.zeros(8)
    p = lambda a: a.ctypes.data

    def host(edges, fixed, poses=T, V_=V, E_=E, out=None, it=15, tol=1e-8, mx=500):
        out = T.copy() if out is None else out
        rc = lib.slam_pg_optimize_host_f64(ctx.handle, V_, E_, p(poses) if poses is not None else None, p(edges), p(Z), p(s.info), p(fixed), it, 0.0,
                                           tol, mx, p(out), p(stats))
        return rc, out

    bad = s.edges.copy()
    bad[17, 1] = V                                           # out of range, found on the device
    rc, out = host(bad, s.fixed)
    assert rc == -1 and b"edge index" in lib.slam_last_error() and np.array_equal(out, T)
    bad = s.edges.copy()
    bad[3, 0] = -2
    rc, out = host(bad, s.fixed)
    assert rc == -1 and np.array_equal(out, T)
    bad = s.edges.copy()
    bad[100] = (7, 7)                                        # self-edge
    rc, out = host(bad, s.fixed)
    assert rc == -1 and np.array_equal(out, T)
    rc, out = host(s.edges, np.zeros(V, np.uint8))           # no fixed vertex: before any launch
    assert rc == -1 and b"fixed vertex" in lib.slam_last_error() and np.array_equal(out, T)
    assert host(s.edges, s.fixed, poses=None)[0] == -1       # null pointer
    assert lib.slam_pg_optimize_host_f64(None, V, E, p(T), p(s.edges), p(Z), p(s.info), p(s.fixed), 15, 0.0, 1e-8, 500, p(T.copy()), p(stats)) == -1
    assert host(s.edges, s.fixed, V_=-1)[0] == -1 and host(s.edges, s.fixed, E_=-1)[0] == -1
    assert host(s.edges, s.fixed, V_=(1 << 24) + 1)[0] == -1 and host(s.edges, s.fixed, E_=(1 << 25) + 1)[0] == -1
    assert host(s.edges, s.fixed, it=-1)[0] == -1 and host(s.edges, s.fixed, tol=0.0)[0] == -1 and host(s.edges, s.fixed, mx=0)[0] == -1
    # V = 0 and E = 0 are not errors
    assert lib.slam_pg_optimize_host_f64(ctx.handle, 0, 0, None, None, None, None, None, 15, 0.0, 1e-8, 500, None, p(stats)) == 0
    rc, out = host(s.edges, s.fixed, E_=0, out=np.zeros_like(T))
    assert rc == 0 and np.array_equal(out, T) and stats[3] == 0
    # the device form: a vertex list that does not match the edges is refused, the output untouched
    from slamhip.pose_graph import vertex_lists
    ptr, adj = vertex_lists(V, s.edges)
    wrong = adj.copy()
    wrong[40] = wrong[41]                                    # one slot named twice, one never
    bufs = [ctx.upload(a) for a in (T, s.edges, Z, s.info, s.fixed, ptr, wrong, adj)]
    dT, de, dZ, dO, df, dp, dbad, dgood = bufs
    dout = ctx.upload(np.zeros_like(T))
    try:
        args = lambda da, nf: (ctx.handle, V, E, dT.ptr, de.ptr, dZ.ptr, dO.ptr, df.ptr, nf, dp.ptr, da.ptr, 15, 0.0, 1e-8, 500, dout.ptr, p(stats))
        assert lib.slam_pg_optimize_f64(*args(dbad, 1)) == -1 and not dout.download(np.float64, T.shape).any()
        assert lib.slam_pg_optimize_f64(*args(dgood, 2)) == -1 and b"n_fixed" in lib.slam_last_error()      # mask and count disagree
        assert lib.slam_pg_optimize_f64(*args(dgood, 0)) == -1
        assert lib.slam_pg_optimize_f64(*args(dgood, 1)) == 0
        ref, _ = run(s, gpu_ctx)
        assert np.array_equal(dout.download(np.float64, T.shape).reshape(-1, 3, 4), ref)                  # device form == host form
        status = ctypes.c_int32(0)
        assert lib.slam_pg_linearize_f64(ctx.handle, V, E, dT.ptr, de.ptr, dZ.ptr, dO.ptr, dp.ptr, dgood.ptr, -1.0, dout.ptr, dout.ptr, dout.ptr,
                                         dout.ptr, ctypes.byref(status)) == -1
        assert lib.slam_pg_hmul_f64(ctx.handle, V, E, de.ptr, dp.ptr, dgood.ptr, df.ptr, None, dout.ptr, 0.0, dout.ptr, dout.ptr) == -1
        assert lib.slam_pg_pcg_f64(ctx.handle, V, E, de.ptr, dp.ptr, dgood.ptr, df.ptr, dout.ptr, dout.ptr, dout.ptr, 0.0, 0.0, 10, dout.ptr, p(stats)) == -1
    finally:
        for b_ in bufs + [dout]:
            b_.free()
    # the wrapper raises, with the library's message
    with pytest.raises(slamhip.SlamHipError):
        slamhip.optimize_pose_graph(s.init, bad, s.meas, s.info, s.fixed, ctx=gpu_ctx)


def test_angle_beyond_the_contract_is_reported_not_nan(gpu_ctx):
    import slamhip

    T = np.tile(np.eye(4)[:3], (2, 1, 1))
    Z = R.exp_se3(np.array([[0.0, 0.0, 3.13, 0.1, 0.2, 0.3]]))          # the residual's angle is 3.13 rad
    cost, b, Hd, W, status = slamhip.pose_graph_linearize(T, np.array([[0, 1]], np.int32), Z, np.eye(6)[None], ctx=gpu_ctx)
    assert status & 2 and np.isfinite(cost) and np.isfinite(b).all() and np.isfinite(Hd).all() and np.isfinite(W).all()


def test_large_graph_runs_and_improves(gpu_ctx):
    """10^5 poses, about 4 * 10^5 edges.  Left out at this size: the comparison with the reference's direct solver (its
    factorisation takes minutes); what is checked is that the run ends without status bits, lowers chi2 to the level the
    noise explains and moves the trajectory towards the truth."""
    s = R.large()
    assert s.V == 100_000 and 380_000 < s.E < 420_000
    P, st = run(s, gpu_ctx)
    print(st)
    assert st["status"] == 0 and st["iterations"] >= 1 and st["trials"] >= st["iterations"]
    assert st["cg_iterations"] <= st["trials"] * R.PCG_MAX_ITER
    assert st["chi2_final"] < 0.01 * st["chi2_initial"]
    assert st["chi2_final"] < 2.0 * 6 * s.E                                   # chi2 of 6 E unit-variance residuals is about 6 E
    assert R.trajectory_error(P, s.gt) < 0.5 * R.trajectory_error(s.init, s.gt)
    assert np.array_equal(P[0], s.init[0])


def test_one_context_two_threads():
    """the call lock covers the new entry points: two threads optimising different graphs on ONE context get the bits of
    their single-threaded runs"""
    import slamhip

    ctx = slamhip.Context(0)
    try:
        graphs = [scene("loop_closure"), scene("hub")]
        alone = [run(g, ctx) for g in graphs]
        results, errors = [None, None], []

        def work(k):
            try:
                for _ in range(3):
                    results[k] = run(graphs[k], ctx)
                    x = np.ones((graphs[k].V, 6))
                    slamhip.pose_graph_hmul(graphs[k].edges, graphs[k].fixed, np.tile(np.eye(6), (graphs[k].V, 1, 1)),
                                            np.zeros((graphs[k].E, 6, 6)), 0.5, x, ctx=ctx)
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
