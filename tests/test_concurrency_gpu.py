"""GPU: one context under concurrent threads, as the reference runs it (slam.py:26-35: a tracking thread and a backend
thread; the overlay gives both the same context).  Tracking threads cycle through the host-buffer (*_host) entry points while
a backend thread cycles through the device-pointer ones, all on ONE context, and every result is held to a value computed
before the threads start: index and distance tables, flags and counts exactly (oracle.bf_knn_c / bf_match_c /
bf_cross_check_c, numpy restatements of the ratio and min-distance filters, of the radius and the window searches), pose
refinement and bundle adjustment to the bars of tests/test_optimize_gpu.py and tests/test_ba_limits_gpu.py.

A call that takes a context block (workspace, merge state, chunk tables, the pinned completion / count block, the filter
scratch, the staging arena) while another thread's kernel still uses it, or reads a count that another call's kernel wrote,
shows up here as a wrong table or count.  Each case makes its own context, so every block starts empty and grows during the
run."""
import ctypes
import threading

import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

FX, FY, CX, CY = 458.654, 457.296, 367.215, 248.375
INTR = (FX, FY, CX, CY)
RATIO, MIN_DIST = 0.75, 40.0
RADIUS = 64.5
JOIN_S = 120.0
NONE_IDX, NONE_DIST = -1, np.iinfo(np.int32).max


def rand_desc(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def _pair(rng, n, m):
    """Random rows with planted near-duplicates and exact duplicates (ties that must go to the lowest index)."""
    q, t = rand_desc(rng, n), rand_desc(rng, m)
    k = min(n, m) // 3
    t[:k] = q[:k]
    flip = rng.integers(0, 256, (k, 32), dtype=np.uint8) & rng.integers(0, 256, (k, 32), dtype=np.uint8) & 0x11
    t[:k] ^= flip
    if m > 8:
        t[m - 1] = t[1]
    return q, t


# ---- restatements of what the kernels compute (numpy, f64) -------------------------------------------------------------
def ratio_keep(idx, dist):
    """Lowe's test as the library states it: a neighbour exists and d0 < ratio * d1 (in f64; a missing d1 is INT32_MAX)."""
    return (idx[:, 0] >= 0) & (dist[:, 0].astype(np.float64) < RATIO * dist[:, 1].astype(np.float64))


def min_dist_keep(idx, dist):
    """feature_matchers.py:41-43: keep d0 < max(2 * min_dist, threshold), min_dist over the queries with a neighbour."""
    has = idx[:, 0] >= 0
    if not has.any():
        return has, NONE_DIST
    mn = int(dist[has, 0].min())
    return has & (dist[:, 0].astype(np.float64) < max(2.0 * mn, MIN_DIST)), mn


def ref_radius(q, t, r):
    from slamhip import radius_threshold

    d = oracle.hamming_matrix_np(q, t)
    qi, ti = np.nonzero(d < radius_threshold(r))
    di = d[qi, ti].astype(np.int32)
    order = np.lexsort((ti, di, qi))
    off = np.zeros(q.shape[0] + 1, np.int64)
    np.cumsum(np.bincount(qi, minlength=q.shape[0]), out=off[1:])
    return off, ti[order].astype(np.int32), di[order]


def ref_window(q, t, qxy, txy, radius, k):
    n, m = q.shape[0], t.shape[0]
    r = np.broadcast_to(np.asarray(radius, np.float32), (m,))
    w = (np.abs(qxy[:, 0][:, None] - txy[None, :, 0]) <= r[None, :]) & (np.abs(qxy[:, 1][:, None] - txy[None, :, 1]) <= r[None, :])
    d = oracle.hamming_matrix_np(q, t).astype(np.int64)
    key = np.where(w, (d << 23) | np.arange(m)[None, :], np.int64(1) << 40)
    top = np.sort(key, axis=1, kind="stable")[:, :k]
    ok = top < (np.int64(1) << 40)
    idx = np.where(ok, top & ((1 << 23) - 1), NONE_IDX).astype(np.int32)
    dist = np.where(ok, top >> 23, NONE_DIST).astype(np.int32)
    return idx, dist


def _scene(rng, K, L):
    from scipy.spatial.transform import Rotation

    T = np.tile(np.eye(4), (K, 1, 1))
    T[:, :3, :3] = Rotation.from_rotvec(rng.uniform(-0.15, 0.15, (K, 3))).as_matrix()
    T[:, :3, 3] = rng.uniform(-0.5, 0.5, (K, 3))
    X = np.c_[rng.uniform(-4, 4, (L, 2)), rng.uniform(6, 15, L)]
    return T, X


def _pose_frame(rng, O):
    T, X = _scene(rng, 1, O)
    pc = X @ T[0, :3, :3].T + T[0, :3, 3]
    meas = np.c_[FX * pc[:, 0] / pc[:, 2] + CX, FY * pc[:, 1] / pc[:, 2] + CY] + rng.normal(0, 0.4, (O, 2))
    meas[::7] += rng.uniform(40, 120, (len(meas[::7]), 2))
    meas = meas.astype(np.int32).astype(np.float64)
    T_init = oracle.se3_exp_np(rng.normal(0, 0.02, 6)) @ T[0]
    return T_init, X, meas, oracle.pose_lm_np(T_init, X, meas, FX, FY, CX, CY)


def _ba_window(rng, K, L, O, fixed):
    """L points, each pose sees a random subset, exactly O observations in arbitrary order (tests/test_ba_limits_gpu.py)."""
    T, X = _scene(rng, K, L)
    pick = rng.permutation(np.sort(rng.choice(K * L, O, replace=False)))
    op, ol = (pick // L).astype(np.int32), (pick % L).astype(np.int32)
    pc = np.einsum("oij,oj->oi", T[op, :3, :3], X[ol]) + T[op, :3, 3]
    meas = np.c_[FX * pc[:, 0] / pc[:, 2] + CX, FY * pc[:, 1] / pc[:, 2] + CY] + rng.normal(0, 0.3, (O, 2))
    T0 = T.copy()
    for k in range(K):
        if k not in fixed:
            T0[k] = oracle.se3_exp_np(rng.normal(0, 0.01, 6)) @ T[k]
    X0 = X + rng.normal(0, 0.05, X.shape)
    w = dict(T0=T0, X0=X0, op=op, ol=ol, meas=meas, fixed=tuple(fixed), iters=5)
    w["ref"] = oracle.ba_lm_c(T0[:, :3, :4].reshape(K, 12), X0, op, ol, meas, FX, FY, CX, CY, w["iters"], w["fixed"], 0.0)
    return w


def _ba_holds(got, w):
    """tests/test_ba_limits_gpu.py's bar against oracle.ba_lm_c; returns a reason or None."""
    Tr, Xr, c0, c1, acc, _ = w["ref"]
    if got.iterations != acc:
        return f"accepted {got.iterations} vs {acc}"
    if abs(got.chi2_initial - c0) > 1e-9 * c0 or abs(got.chi2_final - c1) > 1e-9 * max(c1, 1.0):
        return f"cost {got.chi2_initial}/{got.chi2_final} vs {c0}/{c1}"
    if np.abs(got.poses - Tr).max() > 1e-8 or np.abs(got.points - Xr).max() > 1e-7:
        return f"state off by {np.abs(got.poses - Tr).max()} / {np.abs(got.points - Xr).max()}"
    if any(not np.array_equal(got.poses[k], w["T0"][k]) for k in w["fixed"]):
        return "a fixed pose moved"
    return None


def _pose_holds(got, frame, atol=1e-8):
    Tr, inl, chi2, _ = frame[3]
    if not np.allclose(got.pose, Tr, rtol=0, atol=atol):
        return f"pose off by {np.abs(got.pose - Tr).max()}"
    if not np.array_equal(got.inliers, inl) or not np.allclose(got.chi2, chi2, rtol=1e-6, atol=1e-6):
        return "inliers / chi2 differ"
    return None


# ---- the matching problems and their expected values ---------------------------------------------------------------------
class MatchCase:
    """One (query, train) pair with everything the host and device calls must return for it."""

    def __init__(self, rng, n, m, topk=True, radius=True, window=True):
        self.q, self.t = _pair(rng, n, m)
        self.n, self.m = n, m
        self.idx2, self.dist2 = oracle.bf_knn_c(self.q, self.t, 2, threads=4)
        self.match0 = oracle.bf_match_c(self.t, self.q, None, threads=4)
        self.match1 = oracle.bf_match_c(self.t, self.q, MIN_DIST, threads=4)
        self.keep_ratio = ratio_keep(self.idx2, self.dist2)
        assert np.array_equal(self.keep_ratio, oracle.bf_ratio_c(self.idx2, self.dist2, RATIO))
        self.keep_min, self.min_dist = min_dist_keep(self.idx2, self.dist2)
        assert np.array_equal(np.flatnonzero(self.keep_min), self.match1[0])
        assert np.array_equal(np.flatnonzero(self.idx2[:, 0] >= 0), self.match0[0])
        self.cross = oracle.bf_cross_check_c(self.q, self.t, threads=4)
        self.rev_idx2, self.rev_dist2 = oracle.bf_knn_c(self.t, self.q, 2, threads=4)
        self.topk = oracle.bf_knn_c(self.q, self.t, 5, threads=4) if topk else None
        self.radius = ref_radius(self.q, self.t, RADIUS) if radius else None
        if window:
            self.qxy = rng.uniform(0, 640, (n, 2)).astype(np.float32)
            self.txy = np.clip(self.qxy[rng.integers(0, n, m)] + rng.normal(0, 20, (m, 2)), 0, 640).astype(np.float32)
            self.win = ref_window(self.q, self.t, self.qxy, self.txy, 30.0, 2)
        else:
            self.win = None


def _cmp(errors, tag, got, want):
    if len(got) != len(want) or not all(np.array_equal(a, b) for a, b in zip(got, want)):
        errors.append(tag)


def tracking_step(ctx, c, errors, tag):
    """Every host-buffer call on one MatchCase (and the per-frame pose refinement / the K = 7 window adjustment)."""
    import slamhip

    _cmp(errors, f"{tag} match mode 0", slamhip.match_arrays(c.t, c.q, None, ctx=ctx), c.match0)
    _cmp(errors, f"{tag} match mode 1", slamhip.match_arrays(c.t, c.q, MIN_DIST, ctx=ctx), c.match1)
    qi, ti, di = slamhip.ratio_test_arrays(c.q, c.t, RATIO, ctx=ctx)
    kept = np.flatnonzero(c.keep_ratio)
    _cmp(errors, f"{tag} match mode 2", (qi, ti, di), (kept, c.idx2[kept, 0], c.dist2[kept, 0].astype(np.float32)))
    qi, ti, di = slamhip.cross_check_arrays(c.q, c.t, ctx=ctx)
    oi, od = c.cross
    kept = np.flatnonzero(oi >= 0)
    _cmp(errors, f"{tag} crossCheck", (qi, ti, di), (kept, oi[kept], od[kept].astype(np.float32)))
    _cmp(errors, f"{tag} knn2", slamhip.knn_match_arrays(c.q, c.t, 2, ctx=ctx), (c.idx2, c.dist2))
    if c.topk is not None:
        _cmp(errors, f"{tag} top-5", slamhip.topk_match_arrays(c.q, c.t, 5, ctx=ctx), c.topk)
    if c.radius is not None:
        _cmp(errors, f"{tag} radius", slamhip.radius_match_arrays(c.q, c.t, RADIUS, ctx=ctx), c.radius)
    if c.win is not None:
        _cmp(errors, f"{tag} window", slamhip.window_match_arrays(c.q, c.t, c.qxy, c.txy, 30.0, k=2, ctx=ctx), c.win)


class DeviceRows:
    """One thread's own device copies of a MatchCase (caller-owned buffers: never shared between threads)."""

    def __init__(self, ctx, c):
        self.dq, self.dt = ctx.upload(c.q), ctx.upload(c.t)
        self.idx, self.dist = ctx.malloc(c.n * 8), ctx.malloc(c.n * 8)
        self.keep = ctx.malloc(c.n)
        self.fwd_idx, self.fwd_dist = ctx.upload(c.idx2), ctx.upload(c.dist2)
        self.rev_idx = ctx.upload(c.rev_idx2)
        self.out_idx, self.out_dist = ctx.malloc(c.n * 4), ctx.malloc(c.n * 4)

    def free(self):
        for b in (self.dq, self.dt, self.idx, self.dist, self.keep, self.fwd_idx, self.fwd_dist, self.rev_idx, self.out_idx,
                  self.out_dist):
            b.free()


def backend_search_step(ctx, c, d, errors, tag):
    """The device-pointer searches and filters with a count on one MatchCase."""
    import slamhip

    lib = ctx.lib
    for mode, want in ((0, c.idx2[:, 0] >= 0), (2, c.keep_ratio)):
        cnt = slamhip.knn2_select_device(ctx, d.dq, c.n, d.dt, c.m, d.idx, d.dist, d.keep, mode=mode, param=RATIO)
        if cnt != int(want.sum()):
            errors.append(f"{tag} select mode {mode}: count {cnt} vs {int(want.sum())}")
        keep = d.keep.download(np.uint8, (c.n,))
        if not np.array_equal(keep.astype(bool), want):
            errors.append(f"{tag} select mode {mode}: flags")
        if not (np.array_equal(d.idx.download(np.int32, (c.n, 2)), c.idx2) and np.array_equal(d.dist.download(np.int32, (c.n, 2)), c.dist2)):
            errors.append(f"{tag} select mode {mode}: tables")
    cnt, mind = ctypes.c_int64(-1), ctypes.c_int32(-1)
    assert lib.slam_bf_match_filter(ctx.handle, d.fwd_idx.ptr, d.fwd_dist.ptr, c.n, 1, MIN_DIST, d.keep.ptr, ctypes.byref(cnt),
                                    ctypes.byref(mind)) == 0
    if cnt.value != int(c.keep_min.sum()) or mind.value != c.min_dist:
        errors.append(f"{tag} filter mode 1: count {cnt.value} / min {mind.value} vs {int(c.keep_min.sum())} / {c.min_dist}")
    if not np.array_equal(d.keep.download(np.uint8, (c.n,)).astype(bool), c.keep_min):
        errors.append(f"{tag} filter mode 1: flags")
    cnt = ctypes.c_int64(-1)
    assert lib.slam_bf_cross_check(ctx.handle, d.fwd_idx.ptr, d.fwd_dist.ptr, c.n, d.rev_idx.ptr, c.m, d.out_idx.ptr,
                                   d.out_dist.ptr, ctypes.byref(cnt)) == 0
    oi, od = c.cross
    if cnt.value != int((oi >= 0).sum()):
        errors.append(f"{tag} cross check: count {cnt.value} vs {int((oi >= 0).sum())}")
    if not (np.array_equal(d.out_idx.download(np.int32, (c.n,)), oi) and np.array_equal(d.out_dist.download(np.int32, (c.n,)), od)):
        errors.append(f"{tag} cross check: tables")


class Storm:
    """The problems of one run, built (with every expected value) before any thread starts."""

    def __init__(self, seed, grow):
        rng = np.random.default_rng(seed)
        self.grow = grow
        # tracking: frame-sized (zero-copy, polled) and beyond 4096 rows; growing, the shapes climb step by step
        shapes = [(300, 250), (1500, 1200), (2600, 3100), (5000, 4500)] if grow else [(300, 250), (5000, 4500)]
        self.track = [MatchCase(rng, n, m, radius=n <= 2600, window=n <= 2600) for n, m in shapes]
        # backend: fused select / filter / cross check on device rows; growing, N passes the sizes at which the pinned
        # block's per-wave counts (64 queries a word) and the merge state must grow
        dshapes = [(700, 600), (5000, 300), (140000, 96), (300000, 96)] if grow else [(700, 600), (9000, 300)]
        self.dev = [MatchCase(rng, n, m, topk=False, radius=False, window=False) for n, m in dshapes]
        self.frames = [_pose_frame(rng, O) for O in (200, 120, 650)]
        self.batch = [_pose_frame(rng, int(O)) for O in rng.integers(20, 300, 16)]
        self.ba7 = _ba_window(rng, 7, 300, 1200, (0, 1))                 # the reference's window (backend.py:11)
        self.ba20 = _ba_window(rng, 20, 240, 2400, (0, 1))                # 18 moving poses: the per-phase form


def _run(ctx, storm, tracking_threads=3, rounds=2):
    """Start the threads on one context, join them with a time limit, return the list of mismatches and exceptions."""
    from backend import Backend

    errors = []
    lock = threading.Lock()

    def guarded(fn, name):
        def body():
            errs = []
            try:
                fn(errs, name)
            except Exception as exc:   # noqa: BLE001
                errs.append(f"{name}: {type(exc).__name__}: {exc}")
            with lock:
                errors.extend(errs)
        return body

    def tracking(errs, name):
        import slamhip.ba as ba

        be = Backend()
        be._ctx = ctx
        k = int(name[-1])
        cases = storm.track
        for r in range(rounds):
            for j, c in enumerate(cases):
                c = cases[j] if storm.grow else cases[(j + k + r) % len(cases)]
                tracking_step(ctx, c, errs, f"{name} round {r} {c.n}x{c.m}")
                f = storm.frames[(j + k) % len(storm.frames)]
                why = _pose_holds(be.optimize_pose(f[0], f[1], f[2], FX, FY, CX, CY, on_device=True), f)
                if why:
                    errs.append(f"{name} host pose refinement: {why}")
            w = storm.ba7
            why = _ba_holds(ba.bundle_adjust_auto(w["T0"], w["X0"], w["op"], w["ol"], w["meas"], INTR, iterations=w["iters"],
                                                  fixed_poses=w["fixed"], ctx=ctx), w)
            if why:
                errs.append(f"{name} bundle_adjust_auto K=7: {why}")

    def backend(errs, name):
        be = Backend()
        be._ctx = ctx
        rows = [DeviceRows(ctx, c) for c in storm.dev]
        try:
            for r in range(rounds):
                for c, d in zip(storm.dev, rows):
                    backend_search_step(ctx, c, d, errs, f"{name} round {r} {c.n}x{c.m}")
                f = storm.frames[r % len(storm.frames)]
                why = _pose_holds(be.optimize_pose(f[0], f[1], f[2], FX, FY, CX, CY, on_device=False), f)
                if why:
                    errs.append(f"{name} optimize_pose(on_device=False): {why}")
                got = be.optimize_poses(np.stack([b[0] for b in storm.batch]), [b[1] for b in storm.batch],
                                        [b[2] for b in storm.batch], FX, FY, CX, CY)
                for i, (g, b) in enumerate(zip(got, storm.batch)):
                    why = _pose_holds(g, b, atol=1e-7)
                    if why:
                        errs.append(f"{name} optimize_poses[{i}]: {why}")
                w = storm.ba20
                why = _ba_holds(be.optimize(w["T0"], w["X0"], w["op"], w["ol"], w["meas"], FX, FY, CX, CY,
                                            iterations=w["iters"], fixed_poses=w["fixed"]), w)
                if why:
                    errs.append(f"{name} Backend.optimize K=20: {why}")
        finally:
            for d in rows:
                d.free()

    threads = [threading.Thread(target=guarded(tracking, f"tracking{k}")) for k in range(tracking_threads)]
    threads.append(threading.Thread(target=guarded(backend, "backend")))
    for th in threads:
        th.start()
    for th in threads:
        th.join(JOIN_S)
    assert not any(th.is_alive() for th in threads), "a thread did not finish within the time limit"
    return errors


def _assert_clean(errors):
    assert not errors, f"{len(errors)} mismatches; first: {errors[:6]}"


def _storm(seed, grow):
    return Storm(seed, grow)


def test_tracking_threads_beside_one_device_thread(built):
    """Three tracking threads on the *_host entry points beside one backend thread on the device-pointer entry points,
    all on one fresh context: every table, flag vector and count exact, poses and windows to the oracle bars."""
    import slamhip

    storm = _storm(2601, grow=False)
    ctx = slamhip.Context(0)
    try:
        _assert_clean(_run(ctx, storm, rounds=6))
    finally:
        ctx.close()


def test_every_shared_block_grows_while_others_use_it(built):
    """The same mix, each thread raising its sizes step by step, so that the workspace, the merge state, the pinned
    completion / count block, the staging arena and the radius tables all grow while other threads' calls are in flight."""
    import slamhip

    storm = _storm(2602, grow=True)
    ctx = slamhip.Context(0)
    try:
        # the smallest problem of each kind once, alone: the blocks' first sizes
        be_errors = []
        tracking_step(ctx, storm.track[0], be_errors, "warm-up")
        d = DeviceRows(ctx, storm.dev[0])
        try:
            backend_search_step(ctx, storm.dev[0], d, be_errors, "warm-up")
        finally:
            d.free()
        _assert_clean(be_errors)
        first = ctx.block_bytes()
        assert all(v > 0 for v in first.values()), first
        _assert_clean(_run(ctx, storm, tracking_threads=2, rounds=1))
        last = ctx.block_bytes()
        grew = {k: (first[k], last[k]) for k in first}
        assert all(last[k] > first[k] for k in first), f"a block did not grow: {grew}"
    finally:
        ctx.close()


def test_state_is_clean_after_the_storm(built):
    """After the threads join, the merge state is idle, no kernel met an index out of range, and one more search run alone
    matches the oracle."""
    import slamhip

    storm = _storm(2603, grow=False)
    ctx = slamhip.Context(0)
    try:
        _assert_clean(_run(ctx, storm, tracking_threads=2, rounds=3))
        assert ctx.state_dirty() == 0
        n = ctypes.c_int64(-1)
        assert ctx.lib.slam_index_errors(ctx.handle, ctypes.byref(n)) == 0 and n.value == 0
        c = storm.track[-1]
        idx, dist = slamhip.knn_match_arrays(c.q, c.t, 2, ctx=ctx)
        assert np.array_equal(idx, c.idx2) and np.array_equal(dist, c.dist2)
        d = DeviceRows(ctx, c)
        try:
            slamhip.knn2_device(ctx, d.dq, c.n, d.dt, c.m, d.idx, d.dist)
            assert np.array_equal(d.idx.download(np.int32, (c.n, 2)), c.idx2)
            assert np.array_equal(d.dist.download(np.int32, (c.n, 2)), c.dist2)
        finally:
            d.free()
        assert ctx.state_dirty() == 0
    finally:
        ctx.close()
