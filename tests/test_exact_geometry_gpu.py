"""GPU: the f64 geometry kernels against exact rational arithmetic (tests/exact_geometry.py) on the named geometry set.

Tolerance rule (exact_geometry.C): |kernel - exact| <= C 2^-53 bound, per element, where the bound is the same expression
evaluated on absolute values; an element with a zero bound must match exactly.  The iterative solvers are held to the
existing oracle drivers (pose_lm_np, ba_lm_np) with the tolerances the existing tests assert."""
import numpy as np
import pytest

import exact_geometry as eg

pytestmark = pytest.mark.gpu
SCHUR_CASES = tuple(c for c in eg.CASES if c != "tiny_z")   # why: test_exact_geometry_cpu.SCHUR_CASES


@pytest.mark.parametrize("with_point", [True, False])
@pytest.mark.parametrize("O", [1, 257, 300])
@pytest.mark.parametrize("name", eg.CASES)
def test_reproj_kernel_is_exact(gpu_ctx, name, O, with_point):
    """slam_reproj_rj_f64 on the case's observations cycled to O rows (1: a lone partial block, 257 and 300: a partial
    last block of 256)."""
    import slamhip

    c = eg.case(name)
    rows = np.resize(np.arange(c.O), O)
    e, Jp, Jq = slamhip.build_linearization(c.poses12, c.points, c.obs_pose[rows], c.obs_point[rows], c.meas[rows], *c.cam,
                                            with_point=with_point, ctx=gpu_ctx)
    lins = [eg.exact_lins(name)[o] for o in rows]
    eg.assert_exact(e, [q.e for q in lins], f"{name} e")
    eg.assert_exact(Jp, [q.Jp for q in lins], f"{name} Jpose")
    if with_point:
        eg.assert_exact(Jq, [q.Jq for q in lins], f"{name} Jpoint")
    else:
        assert Jq is None


def test_reproj_kernel_at_z_zero_matches_the_oracle_bit_for_bit(gpu_ctx):
    """Points at Z == 0 exactly have no exact residual (+-inf or NaN): there the kernel equals the C oracle bit for bit,
    inf and NaN in the same places, and the rows beside them in the same 256-row block, transposed through the same LDS
    tile, keep their exact values."""
    import slamhip
    from oracle import oracle

    c = eg.case("benign")
    O = 300
    rows = np.resize(np.arange(c.O), O)
    poses = np.concatenate([c.poses12, [[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]]])      # the identity: Z = the point's z
    pts = np.concatenate([c.points, [[1.5, -2.0, 0.0], [0.0, 0.0, 0.0], [-3.0, 0.0, 0.0]]])
    op, ol, meas = c.obs_pose[rows].copy(), c.obs_point[rows].copy(), c.meas[rows].copy()
    zrows = np.array([0, 100, 101, 255, 256, 299])
    op[zrows] = c.K
    ol[zrows] = c.L + np.arange(len(zrows)) % 3
    e, Jp, Jq = slamhip.build_linearization(poses, pts, op, ol, meas, *c.cam, ctx=gpu_ctx)
    re, rJp, rJq = oracle.reproj_rj_c(poses, pts, op, ol, meas, *c.cam)
    for got, ref in ((e, re), (Jp, rJp), (Jq, rJq)):
        g, r = got[zrows], ref[zrows]
        assert np.array_equal(np.isnan(g), np.isnan(r))            # a NaN's sign bit is not specified: compared as NaN
        assert np.array_equal(g[~np.isnan(g)].view(np.uint64), r[~np.isnan(r)].view(np.uint64))
    assert not np.isfinite(e[zrows]).all() and np.isnan(e[zrows]).any() and np.isinf(e[zrows]).any()
    keep = np.setdiff1d(np.arange(O), zrows)
    lins = [eg.exact_lins("benign")[o] for o in rows[keep]]
    eg.assert_exact(e[keep], [q.e for q in lins], "e beside Z == 0")
    eg.assert_exact(Jp[keep], [q.Jp for q in lins], "Jpose beside Z == 0")
    eg.assert_exact(Jq[keep], [q.Jq for q in lins], "Jpoint beside Z == 0")


@pytest.mark.parametrize("name", eg.CASES)
def test_pose_normal_equations_kernel_is_exact(gpu_ctx, name):
    """slam_pose_normal_eq_f64 on each pose's observations: no kernel and the case's delta (huber_edge: delta = 5 2^-k
    with rows exactly at it and one ulp either side), every row active, a mixed mask, and no row active."""
    import slamhip

    c = eg.case(name)
    for k in range(c.K):
        sel = np.flatnonzero(c.obs_pose == k)
        lins = [eg.exact_lins(name)[o] for o in sel]
        n = len(sel)
        prob = slamhip.PoseOnlyProblem(gpu_ctx, c.points[c.obs_point[sel]], c.meas[sel], c.cam)
        try:
            masks = (np.ones(n, np.uint8), (np.arange(n) % 3 != 1).astype(np.uint8), np.zeros(n, np.uint8))
            for delta in (0.0, c.delta):
                for act in masks:
                    prob.set_active(act)
                    H, b, chi2 = prob.normal_equations(c.poses12[k], delta)
                    rH, rb, rchi2 = eg.pose_normal_eq(lins, act, delta)
                    eg.assert_exact(H, rH, f"{name} pose {k} H delta={delta}")
                    eg.assert_exact(b, rb, f"{name} pose {k} b delta={delta}")
                    eg.assert_exact(chi2, rchi2, f"{name} pose {k} chi2")
                    assert np.array_equal(H, H.T)
                    if not act.any():
                        assert not H.any() and not b.any()
        finally:
            prob.free()


def test_pose_normal_equations_nan_on_an_inactive_row(gpu_ctx):
    """A NaN measurement on an inactive row: H and b are bit for bit those of the same rows with that measurement finite,
    and within the bound of the exact equations without the row; that row's chi2 is NaN (the kernel writes chi2 before
    it tests the active flag).  (Bit identity with a problem that drops the row does not hold: the rows behind it move to
    other lanes of the fixed-order reduction tree.)"""
    import slamhip

    c = eg.case("benign")
    sel = np.flatnonzero(c.obs_pose == 0)
    pts, meas = c.points[c.obs_point[sel]], c.meas[sel].copy()
    n = len(sel)
    act = (np.arange(n) % 3 != 1).astype(np.uint8)
    bad = meas.copy()
    bad[1] = np.nan                                      # row 1 is inactive
    assert act[1] == 0
    lins = [eg.exact_lins("benign")[o] for o in sel]
    for delta in (0.0, c.delta):
        a = slamhip.PoseOnlyProblem(gpu_ctx, pts, bad, c.cam)
        b = slamhip.PoseOnlyProblem(gpu_ctx, pts, meas, c.cam)
        try:
            a.set_active(act)
            b.set_active(act)
            Ha, ba, ca = a.normal_equations(c.poses12[0], delta)
            Hb, bb, cb = b.normal_equations(c.poses12[0], delta)
        finally:
            a.free()
            b.free()
        assert np.isfinite(Ha).all() and np.isfinite(ba).all()
        assert np.array_equal(Ha, Hb) and np.array_equal(ba, bb)
        keep = np.arange(n) != 1
        assert np.isnan(ca[1]) and np.array_equal(ca[keep], cb[keep])
        rH, rb, _ = eg.pose_normal_eq([q for q, k in zip(lins, keep) if k], act[keep], delta)
        eg.assert_exact(Ha, rH, "H with a NaN row inactive")
        eg.assert_exact(ba, rb, "b with a NaN row inactive")


def _check_schur(gpu_ctx, name, extreme):
    from slamhip.ba import SchurProblem

    c = eg.case(name)
    rng = np.random.default_rng(3)
    for ks, sel, delta, lam in eg.schur_configs(name, extreme):
        P, op, ol, meas = eg.window_problem(c, ks, sel)
        K = len(P)
        ref = eg.schur([eg.exact_lins(name)[o] for o in sel], op, ol, K, c.L, delta, lam)
        sp = SchurProblem(gpu_ctx, K, c.L, op, ol, meas, c.cam)
        try:
            S, rhs, bp, cost = sp.reduce(P, c.points, delta, lam)
            eg.assert_exact(S, ref["S"], f"{name} S")
            eg.assert_exact(rhs, ref["rhs"], f"{name} rhs")
            eg.assert_exact(bp, ref["bp"], f"{name} bp")
            eg.assert_exact(cost, eg.bsum(ref["cost"]), f"{name} cost (reduce)")
            for free in (None, [1, 2][:K - 1], [K - 1]):
                eg.assert_exact(sp.diag_max(free), eg.diag_max(ref, free), f"{name} diag_max free={free}")
            dp = rng.normal(0, 1e-3, (K, 6))
            dl, bl = sp.back_substitute(dp)
            dl_ref = eg.backsub(ref, op, ol, dp)
            eg.assert_exact(bl, ref["bl"], f"{name} bl")
            eg.assert_exact(dl, dl_ref, f"{name} dl")
            if not extreme:
                eg.assert_schur_is_tight(S, rhs, bp, dl, ref, dl_ref, name)
            for d in (0.0, c.delta):
                rc = eg.bsum(eg.huber(q.c2, d)[1] for q in (eg.exact_lins(name)[o] for o in sel))
                eg.assert_exact(sp.cost(P, c.points, d), rc, f"{name} cost delta={d}")
        finally:
            sp.free()


@pytest.mark.parametrize("name", SCHUR_CASES)
def test_schur_kernels_are_exact(gpu_ctx, name):
    """slam_ba_reduce_f64, slam_ba_backsub_f64, slam_ba_cost_f64 and SchurProblem.diag_max, with and without a free
    subset, on well-conditioned windows of at most four poses (a point seen by every pose, a pose with no observation,
    points nobody observes; exact_geometry.schur_configs): every output within the bound, and the bound tight enough that
    a wrong reduction fails it."""
    _check_schur(gpu_ctx, name, extreme=False)


@pytest.mark.parametrize("name", SCHUR_CASES)
def test_schur_kernels_at_extreme_damping(gpu_ctx, name):
    """The same with the point seen once kept and lambda = 1e-8 or 1e3: every output within the bound, which for S, rhs
    and dl is as wide as the ill-conditioned E makes it; bp, bl, the costs and diag_max do not go through E and stay
    tight."""
    _check_schur(gpu_ctx, name, extreme=True)


# ---- the iterative solvers on the hard geometries, against the oracle drivers -------------------------------------------
def _pose_frame(name, seed=5):
    """Pose 0 of a case with its points, measurements = projection + 0.4 px noise, every 7th row 40-120 px off, and a
    start pose perturbed by exp(xi) (translation scaled to the depth of the scene)."""
    from oracle import oracle

    c = eg.case(name)
    rng = np.random.default_rng(seed)
    T = np.eye(4)
    T[:3, :4] = c.poses12[0].reshape(3, 4)
    X = c.points[c.obs_point[c.obs_pose == 0]]
    pc = X @ T[:3, :3].T + T[:3, 3]
    fx, fy, cx, cy = c.cam
    meas = np.c_[fx * pc[:, 0] / pc[:, 2] + cx, fy * pc[:, 1] / pc[:, 2] + cy] + rng.normal(0, 0.4, (len(X), 2))
    meas[::7] += rng.uniform(40, 120, (len(meas[::7]), 2))
    xi = rng.normal(0, 0.02, 6)
    xi[3:] *= float(np.median(np.abs(pc[:, 2]))) / 10
    return oracle.se3_exp_np(xi) @ T, X, meas, c.cam


# cancel is left out of the pose-only comparison: its camera sits ~1.7e4 from the origin, so test_optimize_gpu's absolute
# pose tolerance of 1e-8 is 6e-13 relative, below what two correct f64 statements of the same LM reach there
# (oracle.pose_lm_c and oracle.pose_lm_np end 1.2e-4 apart after different numbers of accepted steps)
@pytest.mark.parametrize("name", [n for n in eg.LM_CASES if n != "cancel"])
def test_pose_lm_on_hard_geometry_matches_oracle(gpu_ctx, name):
    """slam_pose_optimize_f64 (one frame and the batch form) against oracle.pose_lm_np, with test_optimize_gpu's
    tolerances: pose 1e-8 (batch 1e-7), the same inliers, chi2 1e-6, accepted steps within 8."""
    from backend import Backend
    from oracle import oracle

    T0, X, meas, cam = _pose_frame(name)
    Tr, inl, chi2, acc = oracle.pose_lm_np(T0, X, meas, *cam)
    assert inl.sum() >= len(X) // 2
    be = Backend()
    got = be.optimize_pose(T0, X, meas, *cam, on_device=True)
    assert np.allclose(got.pose, Tr, rtol=0, atol=1e-8), np.abs(got.pose - Tr).max()
    assert np.array_equal(got.inliers, inl) and got.n_inliers == int(inl.sum())
    assert np.allclose(got.chi2, chi2, rtol=1e-6, atol=1e-6)
    assert abs(got.iterations - acc) <= 8
    batch = be.optimize_poses(np.stack([T0, T0]), [X, X], [meas, meas], *cam)
    for b in batch:
        assert np.array_equal(b.pose, got.pose) and np.array_equal(b.inliers, got.inliers)
        assert np.allclose(b.pose, Tr, rtol=0, atol=1e-7)


@pytest.mark.parametrize("name", eg.LM_CASES)
def test_one_launch_ba_on_hard_geometry_matches_oracle(gpu_ctx, name):
    """slam_ba_optimize_f64 against oracle.ba_lm_np with test_optimize_gpu's tolerances: the same accepted steps, the
    final cost to 1e-9 relative, poses to 1e-8, points to 1e-7.  Pose 0 holds the gauge; point 1 (seen once, its depth
    free) is left out."""
    from oracle import oracle
    from slamhip.ba import bundle_adjust_one_launch

    c = eg.case(name)
    rng = np.random.default_rng(5)
    K = c.K
    s = float(np.median(np.abs(eg.values([q.p[2] for q in eg.exact_lins(name)])))) / 10
    T0 = np.tile(np.eye(4), (K, 1, 1))
    T0[:, :3, :4] = c.poses12.reshape(K, 3, 4)
    for k in range(1, K):
        xi = rng.normal(0, 0.01, 6)
        xi[3:] *= s
        T0[k] = oracle.se3_exp_np(xi) @ T0[k]
    keep = c.obs_point != 1
    op, ol = c.obs_pose[keep], c.obs_point[keep]
    P = c.poses12.reshape(K, 3, 4)
    pc = np.einsum("oij,oj->oi", P[op, :, :3], c.points[ol]) + P[op, :, 3]
    fx, fy, cx, cy = c.cam
    meas = np.c_[fx * pc[:, 0] / pc[:, 2] + cx, fy * pc[:, 1] / pc[:, 2] + cy] + rng.normal(0, 0.2, (len(op), 2))
    X0 = c.points + rng.normal(0, 0.05 * s, c.points.shape)
    iters = 6
    got = bundle_adjust_one_launch(T0, X0, op, ol, meas, c.cam, iterations=iters, fixed_poses=(0,), ctx=gpu_ctx)
    Tr, Xr, c0, c1, acc, _ = oracle.ba_lm_np(T0[:, :3, :4].reshape(K, 12), X0, op, ol, meas, *c.cam, iters, (0,), 0.0)
    assert abs(got.chi2_initial - c0) <= 1e-9 * c0
    assert got.iterations == acc, (got.iterations, acc)
    assert abs(got.chi2_final - c1) <= 1e-9 * max(c1, 1.0), (got.chi2_final, c1)
    assert np.abs(got.poses - Tr).max() <= 1e-8 and np.abs(got.points - Xr).max() <= 1e-7
    assert np.array_equal(got.poses[0], T0[0]) and acc >= 3
