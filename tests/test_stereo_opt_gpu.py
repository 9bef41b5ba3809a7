"""GPU: stereo and level-weighted edges under the pose optimisation and the sparse bundle adjustment (csrc/stereo_edge.h,
pose_stereo.hip, ba_stereo.hip; slamhip/stereo_opt.py) - the per-edge linearisation against the host twin bit for bit, the pose
optimisation against oracle.pose_lm_np (monocular, unit information) and against the statement of tests/stereo_opt_ref.py
(mixed edges, level weights) at the bars of tests/test_optimize_gpu.py::test_device_lm_matches_oracle, the linearisation of the
bundle adjustment against its parent bit for bit and against the statement within the derived rounding bound, the whole
adjustment, LocalBundleAdjustment's schedule, and the refusals."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_sparse_ref as R  # noqa: E402
import stereo_edge_twin as tw  # noqa: E402
import stereo_opt_cases as C  # noqa: E402
import stereo_opt_ref as S  # noqa: E402
from oracle import oracle  # noqa: E402
from test_ba_limits_gpu import _holds  # noqa: E402

pytestmark = pytest.mark.gpu
PCG_TOL = 1e-10
_cache = {}


def _once(key, make):
    """References and scenes are computed once and never modified."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _index_errors(ctx):
    n = ctypes.c_int64(0)
    assert ctx.lib.slam_index_errors(ctx.handle, ctypes.byref(n)) == 0
    return n.value


def _rt(T):
    return T[:, :3, :4].reshape(len(T), 12)


def _mask(w):
    m = np.zeros(len(w["T0"]), bool)
    m[list(w["fixed"])] = True
    return m


def _edges(f):
    from slamhip import StereoEdges

    return StereoEdges(f["meas3"], f["info"], C.BF)


# ---- per-edge linearisation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("O", [1, 63, 257])
def test_edge_linearisation_equals_the_twin_bit_for_bit(gpu_ctx, O):
    """slam_reproj_rj_stereo_f64 against the host build of stereo_edge.h: e, Jpose, Jpoint, chi2 and w of mixed edges (both kinds,
    levels 0..7, s = 0), one index outside its range (NaN outputs, one count)."""
    from slamhip import StereoEdges, stereo_edge_linearization
    from test_stereo_opt_cpu import _table

    T12, X, op, ol, meas3, info = _table(O=max(O, 8))
    op, ol, meas3, info = op[:O].copy(), ol[:O].copy(), meas3[:O], info[:O]
    bad = O // 2 if O > 1 else None                          # (the lone edge of O = 1 stays a good one)
    if bad is not None:
        op[bad] = len(T12) + 3
    _index_errors(gpu_ctx)
    got = stereo_edge_linearization(T12, X, op, ol, StereoEdges(meas3, info, C.BF), R.INTR, S.DELTAS, ctx=gpu_ctx)
    assert _index_errors(gpu_ctx) == (bad is not None)
    ref = tw.edges(T12, X, op, ol, meas3, info, C.CAM, S.DELTAS)
    for k in ("e", "Jpose", "Jpoint", "chi2", "w"):
        assert np.array_equal(got[k], ref[k], equal_nan=True), k
    assert bad is None or (np.isnan(got["e"][bad]).all() and np.isnan(got["w"][bad]))
    assert np.isfinite(got["Jpose"][0]).all()


# ---- pose optimisation --------------------------------------------------------------------------------------------------------
def _pose_bars(got, ref, what):
    """The bars of test_device_lm_matches_oracle: pose 1e-8, the same inlier set, chi2 1e-6 relative, accepted steps within 8."""
    Tr, inl, chi2, acc = ref[:4]
    d = np.abs(got.pose - Tr).max()
    print(f"\n{what}: pose {d:.3g}, chi2 {np.abs(got.chi2 - chi2).max(initial=0.0):.3g}, steps {got.iterations} / {acc}, inliers {int(inl.sum())} of {len(inl)}")
    assert d <= 1e-8, d
    assert np.array_equal(got.inliers, inl) and got.n_inliers == int(inl.sum())
    assert np.allclose(got.chi2, chi2, rtol=1e-6, atol=1e-6)
    assert abs(got.iterations - acc) <= 8


@pytest.mark.parametrize("O,seed", [(12, 4), (200, 228), (C.STAGE + 1, 3)])
def test_monocular_unit_information_matches_the_oracle(gpu_ctx, O, seed):
    """All mr NaN, s = 1, both gates 5.991^2, both widths 1.0: the problem of slam_pose_optimize_f64, against oracle.pose_lm_np
    (C normal equations, numpy solve, scipy matrix exponential - nothing of this pull request) at that test's bars."""
    from slamhip import StereoEdges, optimize_poses_stereo

    f = C.mono_frame(seed, O)
    ref = _once(("oracle", O, seed), lambda: oracle.pose_lm_np(f["T_init"], f["X"], f["meas"], *R.INTR))
    got = optimize_poses_stereo(f["T_init"][None], [f["X"]], [StereoEdges(f["meas3"], f["info"], C.BF)], R.INTR, C.BF,
                                gates=(5.991 ** 2, 5.991 ** 2), deltas=(1.0, 1.0), ctx=gpu_ctx)[0]
    _pose_bars(got, ref, f"oracle O={O}")
    is_bad = np.zeros(O, bool)
    is_bad[f["bad"]] = True
    assert not ref[1][is_bad].any() and ref[1][~is_bad].mean() > 0.9


def _statement(name):
    f = C.pose_scene(name)
    return _once(("statement", name), lambda: S.pose_lm(f["T_init"], f["X"], f["meas3"], f["info"], C.CAM))


@pytest.mark.parametrize("name", list(C.POSE_SCENES))
def test_mixed_weighted_edges_match_the_statement(gpu_ctx, name):
    """Monocular and stereo edges mixed, levels 0..7, planted outliers of both kinds and switched-off edges, ORB-SLAM's gates
    and widths: against the statement at the oracle's bars; the stats row counts inliers, stereo inliers and edges with s > 0."""
    from slamhip import optimize_poses_stereo

    f = C.pose_scene(name)
    ref = _statement(name)
    st = []
    got = optimize_poses_stereo(f["T_init"][None], [f["X"]], [_edges(f)], R.INTR, C.BF, ctx=gpu_ctx, stats_out=st)[0]
    _pose_bars(got, ref, f"statement {name}")
    assert st[0][0].tolist() == [int(ref[1].sum()), got.iterations, ref[4], int((f["info"] > 0).sum())]


def _batch():
    """Frames of 0, 1, 6, STAGE and STAGE + 1 edges (the small ones without planted outliers: they could not lose one)."""
    frames = [C.pose_frame(50, 0, planted=False), C.pose_frame(51, 1, planted=False), C.pose_frame(52, 6, planted=False),
              C.pose_scene("stage"), C.pose_scene("stage+1")]
    refs = _once("batch", lambda: [S.pose_lm(f["T_init"], f["X"], f["meas3"], f["info"], C.CAM) for f in frames])
    return frames, refs


def _run(ctx, frames, **kw):
    from slamhip import optimize_poses_stereo

    st = []
    res = optimize_poses_stereo(np.stack([f["T_init"] for f in frames]), [f["X"] for f in frames], [_edges(f) for f in frames], R.INTR, C.BF,
                                ctx=ctx, stats_out=st, **kw)
    return res, st[0]


def _equal_bits(a, b):
    return np.array_equal(a.pose, b.pose) and np.array_equal(a.inliers, b.inliers) and np.array_equal(a.chi2, b.chi2) and \
        (a.n_inliers, a.iterations) == (b.n_inliers, b.iterations)


def test_batch_of_five_frame_sizes(gpu_ctx):
    """Frames of 0, 1, 6, STAGE and STAGE + 1 edges in one launch: each against the statement at the oracle's bars, the batch
    equal to the frames run one by one bit for bit, and two runs of the batch equal bit for bit."""
    frames, refs = _batch()
    res, st = _run(gpu_ctx, frames)
    assert [len(f["X"]) for f in frames] == [0, 1, 6, C.STAGE, C.STAGE + 1]
    for b, (got, ref) in enumerate(zip(res, refs)):
        _pose_bars(got, ref, f"batch frame {b}")
        assert st[b, 2] == ref[4] and st[b, 3] == int((frames[b]["info"] > 0).sum())
    assert np.array_equal(res[0].pose, frames[0]["T_init"]) and res[0].n_inliers == 0 and res[0].iterations == 0
    again, st2 = _run(gpu_ctx, frames)
    assert all(_equal_bits(a, b) for a, b in zip(res, again)) and np.array_equal(st, st2)
    for b, f in enumerate(frames):
        alone, _ = _run(gpu_ctx, [f])
        assert _equal_bits(alone[0], res[b]), b


def test_a_frame_of_switched_off_edges_returns_its_pose(gpu_ctx):
    f = dict(C.pose_scene("o200"))
    f["info"] = np.zeros_like(f["info"])
    res, st = _run(gpu_ctx, [f, C.pose_scene("o12")])
    assert np.array_equal(res[0].pose, f["T_init"]) and res[0].n_inliers == 0 and not res[0].inliers.any() and res[0].iterations == 0
    assert st[0].tolist() == [0, 0, 0, 0] and (res[0].chi2 == 0).all()
    assert res[1].n_inliers == int(_statement("o12")[1].sum())


def test_a_bad_offsets_table_and_a_bad_information_are_counted_and_clamped(gpu_ctx):
    """The offsets contract of slam_pose_optimize_batch_f64: a table that descends or leaves [0, O_total] shrinks its frames to
    what lies inside and counts them; the sane frame next to them is refined as usual.  A negative and a NaN information count
    once each and act as 0."""
    ctx, lib = gpu_ctx, gpu_ctx.lib
    f = C.pose_scene("o200")
    O = len(f["X"])
    pose = np.tile(f["T_init"][:3, :4].reshape(12), (4, 1))
    info = f["info"].copy()
    bufs = [ctx.upload(pose), ctx.upload(f["X"]), ctx.upload(f["meas3"]), ctx.upload(info), ctx.malloc(4 * 96), ctx.malloc(O), ctx.malloc(O * 8),
            ctx.malloc(64)]
    d_pose, d_pts, d_mes, d_inf, d_out, d_inl, d_chi, d_st = bufs
    _index_errors(ctx)

    def run(table):
        d_off = ctx.upload(np.array(table, np.int32))
        try:
            assert lib.slam_pose_optimize_stereo_batch_f64(ctx.handle, 4, d_pose.ptr, d_pts.ptr, d_mes.ptr, d_inf.ptr, d_off.ptr, O, *R.INTR, C.BF,
                                                           4, 10, *S.GATES, *S.DELTAS, d_out.ptr, d_inl.ptr, d_chi.ptr, d_st.ptr) == 0
            ctx.sync()
            return d_st.download(np.int32, (4, 4)), d_out.download(np.float64, (4, 12))
        finally:
            d_off.free()

    try:
        for table, bad_frames in (([0, 60, 120, 160, 200], 0), ([0, 60, 30, 400, 200], 3), ([-7, 60, 120, 1 << 30, 200], 3)):
            st, out = run(table)
            assert _index_errors(ctx) == bad_frames, table
            if table[0] == 0:
                sane = S.pose_lm(f["T_init"], f["X"][:60], f["meas3"][:60], f["info"][:60], C.CAM)
                assert st[0, 0] == int(sane[1].sum()) and np.abs(out[0].reshape(3, 4) - sane[0][:3]).max() <= 1e-8
        info[10], info[20] = -1.0, np.nan
        d_inf.upload(info)
        st, _ = run([0, 60, 120, 160, 200])
        assert _index_errors(ctx) == 2 and st[0, 3] == int((f["info"][:60] > 0).sum()) - 2
        assert not d_inl.download(np.uint8, (O,))[[10, 20]].any()
    finally:
        for b in bufs:
            b.free()


# ---- bundle adjustment: the linearisation -------------------------------------------------------------------------------------
WINDOWS = {"edges": R.case_edges, "hub": R.case_hub}


def _window(name):
    return _once(("window", name), WINDOWS[name])


def _blocks(ctx, w, delta, stereo):
    """(Hpl, Hll, bl, Hpp, bp, per-pose cost, scal, cost of the cost-only phase and its per-pose costs) at the start state."""
    from slamhip import SparseBAProblem

    K, L = len(w["T0"]), len(w["X0"])
    prob = SparseBAProblem(ctx, K, L, w["op"], w["ol"], w["meas"], R.INTR, _mask(w), stereo=stereo)
    try:
        prob.set_state(_rt(w["T0"]), w["X0"])
        prob.d_T[1].upload(_rt(w["T0"]))
        prob.d_X[1].upload(np.ascontiguousarray(w["X0"]))
        cost, dmax = prob.linearize(delta)
        O = prob.O
        out = dict(Hpl=prob.d_Hpl.download(np.float64, (O, 18)), Hll=prob.d_Hll.download(np.float64, (L, 6)), bl=prob.d_bl.download(np.float64, (L, 3)),
                   Hpp=prob.d_Hpp.download(np.float64, (K, 21)), bp=prob.d_bp.download(np.float64, (K, 6)),
                   cost_pose=prob.d_cost.download(np.float64, (K,)), cost=cost, dmax=dmax)
        c = prob.ctx
        if stereo is None:
            assert c.lib.slam_bas_cost_f64(c.handle, K, L, O, prob.d_T[1].ptr, prob.d_X[1].ptr, prob.d_op.ptr, prob.d_ol.ptr, prob.d_meas.ptr,
                                           prob.d_ps_ptr.ptr, prob.d_ps_obs.ptr, *R.INTR, float(delta), prob.d_cost2.ptr, prob.d_scal.view(24, 8).ptr) == 0
        else:
            assert c.lib.slam_bas_cost_stereo_f64(c.handle, K, L, O, prob.d_T[1].ptr, prob.d_X[1].ptr, prob.d_op.ptr, prob.d_ol.ptr, prob.d_meas3.ptr,
                                                  prob.d_info.ptr, prob.d_ps_ptr.ptr, prob.d_ps_obs.ptr, *R.INTR, C.BF, float(delta), float(delta),
                                                  prob.d_cost2.ptr, prob.d_scal.view(24, 8).ptr) == 0
        out["cost2_pose"] = prob.d_cost2.download(np.float64, (K,))
        out["cost2"] = float(prob.d_scal.download(np.float64, (4,))[3])
        return out
    finally:
        prob.free()


@pytest.mark.parametrize("delta", [0.0, 1.0])
@pytest.mark.parametrize("name", ["edges", "hub"])
def test_monocular_form_equals_the_parent_bit_for_bit(gpu_ctx, name, delta):
    """The parent rule: every mr NaN, every s = 1, delta_mono = huber_delta - Hpl, Hll, bl, Hpp, bp, the per-pose cost and d_scal
    of slam_bas_linearize_stereo_f64 / slam_bas_cost_stereo_f64 equal those of slam_bas_linearize_f64 / slam_bas_cost_f64 in value
    (numpy's ==: +0 and -0 are one value)."""
    from slamhip import StereoEdges

    w = _window(name)
    O = len(w["op"])
    parent = _blocks(gpu_ctx, w, delta, None)
    mono = _blocks(gpu_ctx, w, delta, StereoEdges(np.c_[w["meas"], np.full(O, np.nan)], np.ones(O), C.BF))
    for k in parent:
        assert np.array_equal(parent[k], mono[k]), k
    assert parent["cost"] > 0 and np.isfinite(parent["Hpl"]).all()


@pytest.mark.parametrize("delta", [(0.0, 0.0), S.DELTAS])
@pytest.mark.parametrize("name", ["edges", "hub"])
def test_stereo_blocks_against_the_statement(gpu_ctx, name, delta):
    """u_right on about half of the observations, levels 0..7: the reduced system (Hdiag, every W_e, b) built from the stereo
    blocks against the statement, entry by entry within twice the derived rounding bound - ba_sparse_ref.reduce's bound times
    stereo_opt_ref.BOUND_FACTOR, which carries the third row and the factor s - and the cost to 1e-12 relative."""
    from slamhip import SparseBAProblem, StereoEdges

    w, lam = _window(name), 2.5
    K, L = len(w["T0"]), len(w["X0"])
    meas3, info = _once(("stereo", name), lambda: C.stereo_window(w, 5))
    fixed = _mask(w)
    lin = S.linearize(_rt(w["T0"]), w["X0"], w["op"], w["ol"], meas3, info, C.CAM, delta)
    red = R.reduce(lin, w["op"], w["ol"], fixed, lam)
    prob = SparseBAProblem(gpu_ctx, K, L, w["op"], w["ol"], None, R.INTR, fixed, stereo=StereoEdges(meas3, info, C.BF))
    try:
        prob.set_state(_rt(w["T0"]), w["X0"])
        cost, dmax = prob.linearize(delta)
        prob.reduce(lam)
        Hd, W, b = prob.reduced_system()
        chi2, inl = prob.classify(*S.GATES)
    finally:
        prob.free()
    free = np.flatnonzero(~fixed)
    from test_ba_sparse_gpu import _worst

    B = {k: S.BOUND_FACTOR * v for k, v in red["bound"].items()}
    ratios = dict(W=_worst(W - red["W"], B["W"]), Hdiag=_worst(Hd[free] - red["Hdiag"][free], B["Hdiag"][free]),
                  b=_worst(b[free] - red["b"][free], B["b"][free]))
    print(f"\nstereo blocks [{name}, delta={delta}]: |difference| / bound (allowed 2): " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items())
          + f"; cost {abs(cost - lin['cost']) / lin['cost']:.3g} relative")
    assert max(ratios.values()) <= 2.0, ratios
    assert abs(cost - lin["cost"]) <= 1e-12 * lin["cost"]
    d = max(lin["Hpp"][~fixed].reshape(-1, 36)[:, ::7].max(), lin["Hll"].reshape(-1, 9)[:, ::4].max())
    assert abs(dmax - d) <= 1e-12 * d
    rchi2, rinl = S.classify(_rt(w["T0"]), w["X0"], w["op"], w["ol"], meas3, info, C.CAM)
    assert np.array_equal(chi2, rchi2) and np.array_equal(inl, rinl) and 0 < inl.sum() < len(inl)
    assert (~np.isnan(meas3[:, 2])).mean() > 0.4 and len(set(info.tolist())) == 8


@pytest.mark.parametrize("delta", [(0.0, 0.0), S.DELTAS])
@pytest.mark.parametrize("name", ["edges", "hub"])
def test_whole_stereo_adjustment_follows_the_statement(gpu_ctx, name, delta):
    """Six iterations of bundle_adjust_sparse(..., stereo=...) against the statement's lm (ba_sparse_ref.lm on the stereo
    linearisation) at _holds' bars: the same accepted steps, cost 1e-9 relative, poses 1e-8, points 1e-7, fixed poses bit for
    bit; every solve converged."""
    from slamhip import StereoEdges, bundle_adjust_sparse

    w = _window(name)
    meas3, info = _once(("stereo", name), lambda: C.stereo_window(w, 5))
    ref = _once(("lm", name, delta), lambda: S.lm(w["T0"], w["X0"], w["op"], w["ol"], meas3, info, C.CAM, 6, w["fixed"], delta, PCG_TOL))
    got, st = bundle_adjust_sparse(w["T0"], w["X0"], w["op"], w["ol"], None, R.INTR, iterations=6, fixed_poses=w["fixed"], huber_delta=delta,
                                   pcg_tol=PCG_TOL, ctx=gpu_ctx, stereo=StereoEdges(meas3, info, C.BF))
    print(f"\nstereo adjustment [{name}, delta={delta}]: poses {np.abs(got.poses - ref[0]).max():.3g}, points {np.abs(got.points - ref[1]).max():.3g}, "
          f"cost {abs(got.chi2_final - ref[3]) / max(ref[3], 1.0):.3g} relative, stats {st}")
    _holds(got, (ref[0], ref[1], ref[2], ref[3], ref[4], ref[5]["trials"]), w)
    assert st["unconverged"] == 0 and st["status"] == 0 and st["trials"] == ref[5]["trials"]


# ---- LocalBundleAdjustment ----------------------------------------------------------------------------------------------------
def test_local_bundle_adjust_schedule(gpu_ctx):
    """A window of 12 poses (2 fixed, one camera centre) and 300 points with planted outliers of both kinds and a point that
    starts behind a camera: the outlier list equals the statement's, no planted outlier is inside its gate afterwards, and the
    stereo window comes back at metric scale where the monocular one (the same data, every mr NaN) keeps the perturbed scale.
    Bar of the scale: the relative depth noise of ONE stereo observation, sigma_d Z / bf = 0.3 * 9 / 50.45 = 0.054 (the start is
    0.1 off; the window averages several hundred such observations but runs 5 + 10 iterations only)."""
    from backend import Backend
    from slamhip import StereoEdges, local_bundle_adjust

    w = C.local_window()
    O = len(w["op"])
    ref = _once("local", lambda: S.local_ba(w["T0"], w["X0"], w["op"], w["ol"], w["meas3"], w["info"], C.CAM, w["fixed"]))
    got, outliers, st = local_bundle_adjust(w["T0"], w["X0"], w["op"], w["ol"], StereoEdges(w["meas3"], w["info"], C.BF), R.INTR,
                                            fixed_poses=w["fixed"], ctx=gpu_ctx)
    print(f"\nlocal window: {O} observations, {len(outliers)} outliers ({st['outliers_first']} after the first stage), "
          f"{int(w['planted'].sum())} planted, stats {st}")
    assert len(w["T0"]) == 12 and len(w["X0"]) == 300 and w["fixed"] == (0, 1)
    assert np.array_equal(outliers, ref[2]) and st["outliers_first"] == len(ref[3])
    kinds = np.isnan(w["meas3"][w["planted"], 2])
    assert kinds.any() and (~kinds).any()
    assert np.isin(np.flatnonzero(w["planted"]), outliers).all()
    chi2, inl = S.classify(_rt(got.poses), got.points, w["op"], w["ol"], w["meas3"], w["info"], C.CAM)
    assert not inl[w["planted"]].any()
    behind = np.flatnonzero(w["ol"] == 7)
    assert np.isin(behind[w["op"][behind] == 2], ref[3]).all()                 # the observation of the point behind pose 2's camera
    for k in w["fixed"]:
        assert np.array_equal(got.poses[k], w["T0"][k])
    assert np.abs(got.poses - ref[0]).max() <= 1e-6 and np.abs(got.points - ref[1]).max() <= 1e-5
    bar = 0.3 * 9.0 / C.BF
    mono3 = w["meas3"].copy()
    mono3[:, 2] = np.nan
    mono, _, _ = Backend().local_bundle_adjust(w["T0"], w["X0"], w["op"], w["ol"], StereoEdges(mono3, w["info"], C.BF), *R.INTR,
                                               fixed_poses=w["fixed"])
    s_stereo, s_mono = C.window_scale(got.poses, w["centre"]), C.window_scale(mono.poses, w["centre"])
    print(f"scale against the truth: start {w['scale']}, stereo {s_stereo:.4f}, monocular {s_mono:.4f}, bar {bar:.3f}")
    assert abs(s_stereo - 1) <= bar < abs(s_mono - 1)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_raw_entry_points_refuse_with_a_context(gpu_ctx):
    """SLAM_ERR_INVALID before any launch: bf <= 0, negative gates and widths, sizes out of range, a null pointer.  (d_meas3 needs
    no alignment beyond a double's.)"""
    ctx, lib = gpu_ctx, gpu_ctx.lib
    f = C.pose_scene("o12")
    O = len(f["X"])
    bufs = [ctx.upload(f["T_init"][:3, :4].reshape(1, 12)), ctx.upload(f["X"]), ctx.upload(f["meas3"]), ctx.upload(f["info"]),
            ctx.upload(np.array([0, O], np.int32)), ctx.malloc(96), ctx.malloc(O), ctx.malloc(O * 8), ctx.malloc(16)]
    p = [b.ptr for b in bufs]

    def pose(bf=C.BF, gates=S.GATES, deltas=S.DELTAS, B=1, rounds=4, null=None):
        a = list(p)
        if null is not None:
            a[null] = None
        return lib.slam_pose_optimize_stereo_batch_f64(ctx.handle, B, a[0], a[1], a[2], a[3], a[4], O, *R.INTR, bf, rounds, 10, *gates, *deltas,
                                                       a[5], a[6], a[7], a[8])

    try:
        _index_errors(ctx)
        for kw in (dict(bf=0.0), dict(bf=-3.0), dict(bf=float("nan")), dict(gates=(-1.0, 7.8)), dict(gates=(5.9, float("nan"))),
                   dict(deltas=(1.0, -2.0)), dict(B=-1), dict(rounds=65), *[dict(null=i) for i in range(9)]):
            assert pose(**kw) == -1, kw
        assert pose(B=0) == 0 and pose() == 0
        ctx.sync()
        K = L = 1
        op = ctx.upload(np.zeros(O, np.int32))
        rj = [ctx.malloc(O * 24), ctx.malloc(O * 144), ctx.malloc(O * 72), ctx.malloc(O * 8), ctx.malloc(O * 8)]
        bufs += [op, *rj]
        args = lambda bf, dm, n=None: [ctx.handle, p[0], K, p[1], O, op.ptr, op.ptr, p[2], p[3], O, *R.INTR, bf, dm, 0.0,  # noqa: E731
                                       *[None if n == i else b.ptr for i, b in enumerate(rj)]]
        assert lib.slam_reproj_rj_stereo_f64(*args(0.0, 0.0)) == -1 and lib.slam_reproj_rj_stereo_f64(*args(C.BF, -1.0)) == -1
        assert all(lib.slam_reproj_rj_stereo_f64(*args(C.BF, 0.0, n)) == -1 for n in range(5))
        cl = lambda bf, g: lib.slam_bas_classify_stereo_f64(ctx.handle, K, O, O, p[0], p[1], op.ptr, op.ptr, p[2], p[3], *R.INTR, bf, g, 7.8,  # noqa: E731
                                                            rj[3].ptr, p[6])
        assert cl(0.0, 5.9) == -1 and cl(C.BF, -5.9) == -1 and cl(C.BF, 5.9) == 0
        ctx.sync()
        assert _index_errors(ctx) == 0
    finally:
        for b in bufs:
            b.free()
