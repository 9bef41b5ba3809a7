"""GPU: the one-launch window bundle adjustment (slam_ba_optimize_f64, csrc/ba_schur.hip) at the limits of its launch shape,
the size routing of Backend.optimize between it and the per-phase form, and the pose-only refinement at its LDS staging
switch.

The one-launch form cuts every pose task and every pair task (a pair of free poses) into `slices` parts, one workgroup
each, and the consumers add the parts back in slice order; with more tasks than workgroups, workgroups take several tasks.
A wrong slice count, a dropped or double-counted slice or a lost task changes the answer by a little, which only an oracle
sees.  So every case here is held to oracle.ba_lm_c (the C statement of the same Schur-complement LM) with the bar of
tests/test_optimize_gpu.py: the same number of accepted steps, initial and final cost to 1e-9 relative, poses to 1e-8,
points to 1e-7, fixed poses returned bit for bit.  Each case names its regime and asserts it, as literal (workgroups,
slices), through slamhip.ba.one_launch_shape, the rule the launch itself uses: a retune of that rule fails here until the
cases are moved back onto their edges.

The windows follow tests/test_optimize_gpu.py: its intrinsics, int32 indices, observations in arbitrary order, pixel
noise, small pose and point perturbations.  Seeds and step counts were chosen so that every trial's gain ratio stays well
away from 0, where rounding could legitimately split the two sides (tools/fuzz_ba.py)."""
import numpy as np
import pytest

from ba_sparse_ref import scene as _scene, smallest as _smallest, uneven as _uneven, window as _window
from oracle import oracle

pytestmark = pytest.mark.gpu
FX, FY, CX, CY = 458.654, 457.296, 367.215, 248.375
INTR = (FX, FY, CX, CY)
MAX_OBS = 131072
# 16 moving poses of 64, scattered: not a prefix, pose 0 holds the gauge, the last pose moves
FREE64 = (3, 7, 11, 12, 18, 22, 29, 30, 37, 41, 44, 50, 53, 57, 60, 63)


def _all_pairs(rng, K, L, fixed):
    """Every point seen by every pose."""
    T, X = _scene(rng, K, L)
    op = np.repeat(np.arange(K), L)
    ol = np.tile(np.arange(L), K)
    return _window(rng, T, X, op, ol, fixed)


def _dense(rng, K, L, O, fixed):
    """L points, each pose sees a random subset; exactly O observations."""
    T, X = _scene(rng, K, L)
    pick = np.sort(rng.choice(K * L, O, replace=False))
    return _window(rng, T, X, pick // L, pick % L, fixed)


def _sliding(rng, K, O, dense_points=0):
    """A keyframe window: every point seen by 2 to 6 consecutive poses, `dense_points` more seen by all K poses; exactly O
    observations (the last sliding point takes what is left); the moving poses are FREE64."""
    spans = []
    left = O - dense_points * K
    while left > 0:
        n = min(int(rng.integers(2, 7)), left)
        spans.append((int(rng.integers(0, K - n + 1)), n))
        left -= n
    L = dense_points + len(spans)
    T, X = _scene(rng, K, L)
    op = [np.repeat(np.arange(K), dense_points)]
    ol = [np.tile(np.arange(dense_points), K)]
    for i, (s, n) in enumerate(spans):
        op.append(np.arange(s, s + n))
        ol.append(np.full(n, dense_points + i))
    op, ol = np.concatenate(op), np.concatenate(ol)
    fixed = [k for k in range(K) if k not in FREE64]
    return _window(rng, T, X, op, ol, fixed)


def _shape(w):
    from slamhip.ba import one_launch_shape

    K = w["T0"].shape[0]
    return one_launch_shape(K, len(w["op"]), K - len(set(w["fixed"])))


def _oracle(w, iters, delta):
    K = w["T0"].shape[0]
    return oracle.ba_lm_c(w["T0"][:, :3, :4].reshape(K, 12), w["X0"], w["op"], w["ol"], w["meas"], FX, FY, CX, CY, iters,
                          w["fixed"], delta)


def _holds(got, ref, w, min_steps=3):
    """got (a BAResult) against oracle.ba_lm_c's (T, X, cost0, cost, accepted, trials) with the suite's bar."""
    Tr, Xr, c0, c1, acc, _ = ref
    assert got.iterations == acc, (got.iterations, acc)
    assert abs(got.chi2_initial - c0) <= 1e-9 * c0, (got.chi2_initial, c0)
    assert abs(got.chi2_final - c1) <= 1e-9 * max(c1, 1.0), (got.chi2_final, c1)
    assert np.abs(got.poses - Tr).max() <= 1e-8, np.abs(got.poses - Tr).max()
    assert np.abs(got.points - Xr).max() <= 1e-7, np.abs(got.points - Xr).max()
    for k in w["fixed"]:
        assert np.array_equal(got.poses[k], w["T0"][k]), k
    assert acc >= min_steps and c1 < 0.05 * c0, (acc, c0, c1)


def _one_launch(ctx, w, iters, delta):
    from slamhip.ba import bundle_adjust_one_launch

    return bundle_adjust_one_launch(w["T0"], w["X0"], w["op"], w["ol"], w["meas"], INTR, iterations=iters, fixed_poses=w["fixed"],
                                    huber_delta=delta, ctx=ctx)


def _per_phase(ctx, w, iters, delta):
    from slamhip.ba import bundle_adjust_device

    return bundle_adjust_device(w["T0"], w["X0"], w["op"], w["ol"], w["meas"], INTR, iterations=iters, fixed_poses=w["fixed"],
                                huber_delta=delta, ctx=ctx)


def _same(a, b):
    return (np.array_equal(a.poses, b.poses) and np.array_equal(a.points, b.points) and a.chi2_initial == b.chi2_initial
            and a.chi2_final == b.chi2_final and a.iterations == b.iterations)


def _per_phase_agrees(ctx, w, iters, delta, got):
    """The per-phase form (slam_ba_reduce_f64 + host solve) follows the one-launch result, as in the trajectory test."""
    dev = _per_phase(ctx, w, iters, delta)
    assert dev.iterations == got.iterations and abs(dev.chi2_final - got.chi2_final) <= 1e-9 * max(got.chi2_final, 1.0)
    assert np.abs(dev.poses - got.poses).max() <= 1e-8


# ---- the one-launch form at the edges of its shape -----------------------------------------------------------------------
@pytest.mark.parametrize("delta", [0.0, 1.0])
def test_eight_slices_on_128_workgroups_at_the_observation_limit(gpu_ctx, delta):
    """K = 2 with pose 1 moving, 65 536 points seen by both: O = 131 072 = SLAM_BA_LM_MAX_OBS exactly.  Three tasks (two
    poses, one pair) on the 128-workgroup cap, each cut into the 8-slice cap: every slice of a pose list is 8 192 entries,
    eight 1024-entry strides of bg_pose.  Two launches are bit-identical; the per-phase form follows."""
    w = _all_pairs(np.random.default_rng(131072), 2, 65536, (0,))
    assert len(w["op"]) == MAX_OBS and _shape(w) == (128, 8)
    got = _one_launch(gpu_ctx, w, 6, delta)
    assert _same(got, _one_launch(gpu_ctx, w, 6, delta))
    _holds(got, _oracle(w, 6, delta), w)
    _per_phase_agrees(gpu_ctx, w, 6, delta, got)


def test_first_window_of_three_poses_with_eight_slices(gpu_ctx):
    """K = 3 with poses 1 and 2 moving (six tasks) and 24 065 observations: the first size at which that window reaches 8
    slices (48 workgroups); one observation fewer gives 7."""
    from slamhip.ba import one_launch_shape

    w = _dense(np.random.default_rng(24065), 3, 9000, 24065, (0,))
    assert _shape(w) == (48, 8) and one_launch_shape(3, 24064, 2) == (47, 7)
    _holds(_one_launch(gpu_ctx, w, 6, 0.0), _oracle(w, 6, 0.0), w)


def test_seven_slices_over_lists_that_do_not_divide(gpu_ctx):
    """K = 4 with three moving poses (ten tasks), 40 000 observations: 79 workgroups, 7 slices - not a power of two - over
    pose lists whose lengths are not multiples of 7, so the last slice of every list is short."""
    w = _dense(np.random.default_rng(40001), 4, 12000, 40000, (0,))
    assert _shape(w) == (79, 7)
    counts = np.bincount(w["op"], minlength=4)
    assert (counts % 7 != 0).all(), counts
    _holds(_one_launch(gpu_ctx, w, 6, 1.5), _oracle(w, 6, 1.5), w)


@pytest.mark.parametrize("delta", [0.0, 2.0])
def test_uneven_pose_lists_under_slicing(gpu_ctx, delta):
    """4 slices on 73 workgroups (K = 7, four moving poses: 17 tasks), over lists of every awkward length: a moving pose and
    a fixed pose with no observation (every slice of them, and every pair task that starts at the moving one, is empty), a
    moving pose with 2 observations (fewer than the slices: two empty slices), one pose with more than half of all
    observations; points seen once, by every pose that sees anything, and by nobody.  slam_ba_optimize_host_f64 takes such
    a window: poses without observations only get the damping on their diagonal, points without observations keep their
    position."""
    w = _uneven(np.random.default_rng(37002))
    assert _shape(w) == (73, 4)
    counts = np.bincount(w["op"], minlength=7)
    assert counts[2] == 0 and counts[6] == 0 and counts[3] == 2 and counts[4] > len(w["op"]) / 2
    got = _one_launch(gpu_ctx, w, 6, delta)
    _holds(got, _oracle(w, 6, delta), w)
    unseen = np.setdiff1d(np.arange(len(w["X0"])), w["ol"])
    assert len(unseen) == 500 and np.array_equal(got.points[unseen], w["X0"][unseen])


@pytest.mark.parametrize("delta", [0.0, 1.0])
def test_sixty_four_poses_two_hundred_tasks(gpu_ctx, delta):
    """K = 64 (the most sT / s_ps_ptr in LDS hold) with 16 scattered moving poses (the most, pose 63 among them): 64 pose
    and 136 pair tasks on 128 workgroups, one slice, so workgroups take a second task; a keyframe window of 10 000
    observations, every point seen by 2 to 6 consecutive poses."""
    w = _sliding(np.random.default_rng(64), 64, 10000)
    assert _shape(w) == (128, 1) and len(w["op"]) == 10000
    _holds(_one_launch(gpu_ctx, w, 6, delta), _oracle(w, 6, delta), w)


@pytest.mark.parametrize("delta", [0.0, 1.0])
def test_sixty_four_poses_at_the_observation_limit(gpu_ctx, delta):
    """K = 64, 16 scattered moving poses and 131 072 observations: 1 800 points seen by all 64 poses (the four-lanes-per-point
    path) and a keyframe window of 2 to 6 consecutive poses; 200 tasks on 128 workgroups.  Two launches are bit-identical;
    the per-phase form follows."""
    w = _sliding(np.random.default_rng(6464), 64, MAX_OBS, dense_points=1800)
    assert _shape(w) == (128, 1) and len(w["op"]) == MAX_OBS
    got = _one_launch(gpu_ctx, w, 5, delta)
    assert _same(got, _one_launch(gpu_ctx, w, 5, delta))
    _holds(got, _oracle(w, 5, delta), w)
    _per_phase_agrees(gpu_ctx, w, 5, delta, got)


def test_smallest_launch_with_lists_shorter_than_the_slices(gpu_ctx):
    """The 8-workgroup floor: K = 3, one moving pose (four tasks, 2 slices), 25 observations; pose 0's list has a single
    entry, so its second slice is empty."""
    w = _smallest(np.random.default_rng(8))
    assert _shape(w) == (8, 2) and np.bincount(w["op"]).tolist() == [1, 12, 12]
    _holds(_one_launch(gpu_ctx, w, 6, 0.0), _oracle(w, 6, 0.0), w)


# ---- Backend.optimize: which form a window goes to ----------------------------------------------------------------------
def _spy(monkeypatch):
    """Record the calls of bundle_adjust_auto and bundle_adjust_device that Backend.optimize makes (both still run)."""
    import slamhip.ba as ba

    calls = []
    for name in ("bundle_adjust_auto", "bundle_adjust_device"):
        real = getattr(ba, name)

        def spy(*args, _real=real, _name=name, **kwargs):
            calls.append(_name)
            return _real(*args, **kwargs)

        monkeypatch.setattr(ba, name, spy)
    return calls


def _route(monkeypatch, w, iters=5, delta=0.0):
    from backend import Backend

    calls = _spy(monkeypatch)
    got = Backend().optimize(w["T0"], w["X0"], w["op"], w["ol"], w["meas"], FX, FY, CX, CY, iterations=iters, fixed_poses=w["fixed"],
                             huber_delta=delta)
    _holds(got, _oracle(w, iters, delta), w)
    return calls


def _route_windows():
    """(name, window, form) at and one past each limit of the one-launch form."""
    out = []
    w = _sliding(np.random.default_rng(640), 64, 6000)
    out.append(("64 poses", w, "one launch"))
    out.append(("65 poses", _sliding(np.random.default_rng(650), 65, 6000), "per phase"))     # still 16 moving
    rng = np.random.default_rng(16)
    out.append(("16 free", _dense(rng, 18, 400, 5000, (0, 1)), "one launch"))
    out.append(("17 free", _dense(rng, 19, 400, 5000, (0, 1)), "per phase"))
    rng = np.random.default_rng(17)
    out.append(("131072 observations", _dense(rng, 3, 43700, MAX_OBS, (0,)), "one launch"))
    out.append(("131073 observations", _dense(rng, 3, 43700, MAX_OBS + 1, (0,)), "per phase"))
    return out


@pytest.mark.parametrize("case", range(6), ids=["64-poses", "65-poses", "16-free", "17-free", "131072-obs", "131073-obs"])
def test_backend_routes_windows_at_and_past_each_limit(gpu_ctx, monkeypatch, case):
    """Backend.optimize sends a window exactly at a limit of the one-launch form (64 poses, 16 moving poses, 131 072
    observations) to bundle_adjust_auto and one past it (65, 17, 131 073) to the per-phase form, whose first test beyond
    16 poses this is; both match the oracle."""
    from slamhip.ba import one_launch_shape

    name, w, form = _route_windows()[case]
    K, O, nf = w["T0"].shape[0], len(w["op"]), w["T0"].shape[0] - len(set(w["fixed"]))
    if form == "one launch":
        one_launch_shape(K, O, nf)
        assert _route(monkeypatch, w) == ["bundle_adjust_auto"], name
    else:
        with pytest.raises(ValueError):
            one_launch_shape(K, O, nf)
        assert _route(monkeypatch, w) == ["bundle_adjust_device"], name


def test_backend_per_phase_window_of_a_hundred_poses(gpu_ctx, monkeypatch):
    """100 poses, 30 of them moving (a 180 x 180 reduced system solved on the host) and 20 000 observations: per-phase
    form, against the oracle."""
    rng = np.random.default_rng(100)
    moving = set(rng.choice(np.arange(1, 100), 30, replace=False).tolist())
    w = _dense(rng, 100, 2000, 20000, [k for k in range(100) if k not in moving])
    assert _route(monkeypatch, w) == ["bundle_adjust_device"]


# ---- the pose-only refinement at its staging switch ----------------------------------------------------------------------
def _pose_frame(O, seed):
    rng = np.random.default_rng(seed)
    T, X = _scene(rng, 1, O)
    pc = X @ T[0, :3, :3].T + T[0, :3, 3]
    meas = np.c_[FX * pc[:, 0] / pc[:, 2] + CX, FY * pc[:, 1] / pc[:, 2] + CY] + rng.normal(0, 0.4, (O, 2))
    bad = np.arange(0, O, 7)
    meas[bad] += rng.uniform(40, 120, (len(bad), 2)) * rng.choice([-1, 1], (len(bad), 2))
    meas = meas.astype(np.int32).astype(np.float64)
    return oracle.se3_exp_np(rng.normal(0, 0.02, 6)) @ T[0], X, meas


@pytest.mark.parametrize("O", [511, 512, 513])
def test_pose_refinement_at_the_staging_switch(gpu_ctx, O):
    """SLAM_POSE_STAGE = 512: up to 512 edges pose_opt_kernel keeps them in LDS (two chi2 buffers, zero-copy polled host
    call), from 513 on it works from global memory.  Each side of the switch against oracle.pose_lm_np with the bar of
    test_device_lm_matches_oracle."""
    from backend import Backend

    T0, X, meas = _pose_frame(O, 5000 + O)
    Tr, inl, chi2, acc = oracle.pose_lm_np(T0, X, meas, FX, FY, CX, CY)
    got = Backend().optimize_pose(T0, X, meas, FX, FY, CX, CY, on_device=True)
    assert np.allclose(got.pose, Tr, rtol=0, atol=1e-8), np.abs(got.pose - Tr).max()
    assert np.array_equal(got.inliers, inl) and got.n_inliers == int(inl.sum())
    assert np.allclose(got.chi2, chi2, rtol=1e-6, atol=1e-6)
    assert abs(got.iterations - acc) <= 8
    assert not inl[::7].any() and inl.mean() > 0.8


def test_pose_refinement_batch_across_the_staging_switch(gpu_ctx):
    """511, 512 and 513 edges in one slam_pose_optimize_batch_f64 launch == the single-frame calls, bit for bit."""
    from backend import Backend

    frames = [_pose_frame(O, 5000 + O) for O in (511, 512, 513)]
    be = Backend()
    batch = be.optimize_poses(np.stack([f[0] for f in frames]), [f[1] for f in frames], [f[2] for f in frames], FX, FY, CX, CY)
    for (T0, X, meas), b in zip(frames, batch):
        one = be.optimize_pose(T0, X, meas, FX, FY, CX, CY, on_device=True)
        assert np.array_equal(b.pose, one.pose) and np.array_equal(b.inliers, one.inliers) and np.array_equal(b.chi2, one.chi2)
        assert b.n_inliers == one.n_inliers and b.iterations == one.iterations
