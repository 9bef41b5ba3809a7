"""Time of the fusion search and of the map-point refresh (slam_fuse_*).  Device calls are bracketed by HIP events
(slam_timer_start/stop) around one warm call on device-resident arrays - the bracket holds the call's host side too: the pair
table, the check of the observation offsets, the job table - and the median of the rounds with the spread (min - max) is
reported.  Host-side lines are wall clock and say so.

    python tools/fuse_time.py [--rounds R]

  * scene    that of tools/proj_match_time.py: a 752 x 480 frame of 2000 features over 8 levels at 1.2 and 256 point sets of 2000
             map points, 1500 of each seen by the frame, every pair under its own first pose.  Every point is a map point with
             three observations in other frames (the skip's binary search runs and finds nothing); half of the frame's rows hold
             a map point.  The observation table of the 1-pair case holds that set's 2000 points, that of the 256-pair case all
             512000.
  * search   slam_fuse_search of 1 and of 256 pairs alternating in one process with slam_proj_match_search on the same pairs,
             points, poses and radius factor (th = 3), and the scan kernels alone by the library's own event bracket;
  * refresh  slam_fuse_refresh of 10^5 points with 8 observations and of 10^3 points with 256, over 256 frames of 2000 rows,
             beside the numpy statement of tests/fuse_ref.py on one host core (wall clock, on the first points of each case).
The values are a record, not a gate."""
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "slam-experiments_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import slamhip  # noqa: E402
from slamhip import fuse as fz  # noqa: E402
from slamhip import proj_match as pm  # noqa: E402
from slamhip._lib import FuseParams, ProjParams, addr  # noqa: E402

import fuse_ref  # noqa: E402
import proj_match_time as PT  # noqa: E402
from bow_time import opt, spread  # noqa: E402

W, H, L, SCALE, CAMERA, B, N, SEEN = PT.W, PT.H, PT.L, PT.SCALE, PT.CAMERA, PT.B, PT.N, PT.SEEN
TH = 3.0


def main():
    rounds = max(15, opt("--rounds", 15))
    ctx = slamhip.default_context()
    lib, h = ctx.lib, ctx.handle
    rng = np.random.default_rng(2203)
    s, s2 = pm.scale_tables(L, SCALE)

    def timed(fn):
        ctx.timer_start()
        fn()
        return ctx.timer_stop()

    print(slamhip.load().slam_version().decode())
    print(f"limits: {fz.limits()}")
    frame = PT.make_frame(rng, N)
    sets = [PT.make_points(rng, frame, N, SEEN, s) for _ in range(B)]
    cat = lambda k: np.concatenate([p[k] for p in sets])  # noqa: E731
    ps = pm.PointSets(cat("xyz"), cat("desc"), np.arange(B + 1) * N, cat("dmin2"), cat("dmax2"), cat("normal"), None, cat("bins"), ctx=ctx)
    fg = pm.FrameGrids.from_arrays(frame["desc"], frame["xy"], frame["level"], (W, H), bins=frame["bins"], ctx=ctx)
    poses = np.ascontiguousarray(np.stack([PT.first_pose(rng) for _ in range(B)]))
    centres = pm.camera_centres(poses)
    th = np.full(B, TH)
    pairs = np.stack([np.arange(B), np.zeros(B, np.int64)], 1).astype(np.int32)
    prm = ProjParams(*CAMERA, 0.0, float(W), 0.0, float(H), pm.COS2_LIMIT, pm.RATIO, addr(s), addr(s2), L, pm.TH_HIGH, 1, -1, 0, 0)
    fp = FuseParams(fz.MARGINS[0], fz.MARGINS[1], fz.CHI2, fz.TH_LOW, 0)
    d_id = ctx.upload(np.arange(B * N, dtype=np.int32))
    out = [ctx.malloc(4 * B * N) for _ in range(4)]
    d_c, d_m, d_c2 = ctx.malloc(12 * B), ctx.malloc(4 * B * N), ctx.malloc(4 * B)
    sp, sf = ps._struct(ctx), fg._struct(ctx)
    for P in (1, B):
        M = P * N
        ob = fz.MapObservations.from_arrays(np.arange(M + 1, dtype=np.int64) * 3, np.stack([np.tile([1, 2, 3], M), rng.integers(0, N, 3 * M)], 1), ctx)
        dev = ob._resident(ctx)
        d_pt = ctx.upload(np.where(rng.uniform(size=N) < 0.5, rng.integers(0, M, N), -1).astype(np.int32))

        def fuse():
            assert lib.slam_fuse_search(h, ctypes.byref(sp), d_id.ptr, ctypes.byref(sf), d_pt.ptr, addr(ob.offsets), dev["offsets"].ptr,
                                        dev["obs"].ptr, M, addr(pairs), addr(poses), addr(centres), addr(th), P, ctypes.byref(prm),
                                        ctypes.byref(fp), *(o.ptr for o in out), d_c.ptr, None, None, None) == 0

        def proj():
            assert lib.slam_proj_match_search(h, ctypes.byref(sp), ctypes.byref(sf), addr(pairs), addr(poses), addr(centres), addr(th), P,
                                              ctypes.byref(prm), d_m.ptr, d_c2.ptr, *[None] * 6) == 0

        timed(fuse)
        timed(proj)
        t_f, t_p = [], []
        for _ in range(rounds):                             # alternating in one process
            t_f.append(timed(fuse))
            t_p.append(timed(proj))
        cnt = d_c.download(np.int32, (P, 3)).sum(0)
        found = int(d_c2.download(np.int32, (P,)).sum())
        ctx.prof_enable(True)
        k_f, k_p = [], []
        for _ in range(rounds):
            fuse()
            ctx.sync()
            k_f.append(ctx.prof_read()[1])
            proj()
            ctx.sync()
            k_p.append(ctx.prof_read()[1])
        ctx.prof_enable(False)
        name = f"{P} x {N}"
        print(f"fuse       {name:>10} points, th {TH:g}, table of {M} points: {spread(t_f)}  {np.median(t_f) * 1e3 / P:8.2f} us / pair; per pair "
              f"{cnt[0] / P:.0f} added, {cnt[1] / P:.0f} same landmark, {cnt[2] / P:.0f} lost the row")
        print(f"projection {name:>10} points, th {TH:g}: {spread(t_p)}  {np.median(t_p) * 1e3 / P:8.2f} us / pair, {found / P:.0f} matches / pair")
        print(f"scans      {name:>10} fz_scan_kernel alone: {spread(k_f)}   pm_scan_kernel alone: {spread(k_p)}")
        ratio = np.median(t_f) / np.median(t_p)
        print(f"ratio      {name:>10}: the fusion search takes {ratio:6.3f} of search_by_projection's time - it "
              f"{'is faster than' if ratio < 1 else 'loses to'} search_by_projection on the same pairs")
        ob.free()
        d_pt.free()
    for o in (ps, fg, d_id, d_c, d_m, d_c2, *out):
        o.free()

    # ---- the refresh: 256 frames of 2000 rows, descriptors in clusters of 64 so that the medians are not all alike
    FB = 256
    seeds = rng.integers(0, 256, (64, 32), dtype=np.uint8)
    desc = seeds[rng.integers(0, 64, FB * N)] ^ (rng.integers(0, 256, (FB * N, 32), dtype=np.uint8) & rng.integers(0, 256, (FB * N, 32), dtype=np.uint8)
                                                  & rng.integers(0, 256, (FB * N, 32), dtype=np.uint8))
    level = rng.integers(0, L, FB * N).astype(np.int32)
    xy = np.stack([rng.uniform(0, W, FB * N), rng.uniform(0, H, FB * N)], 1).astype(np.float32)
    foff = np.arange(FB + 1, dtype=np.int64) * N
    frames = pm.FrameGrids.from_arrays(desc, xy, level, (W, H), foff, ctx=ctx)
    cen = rng.normal(0, 1, (FB, 3))
    d_cen = ctx.upload(cen)
    sf = frames._struct(ctx)
    for M, n_obs, n_host in ((100000, 8, 2000), (1000, 256, 50)):
        fr = np.stack([np.sort(rng.choice(FB, n_obs, replace=False)) for _ in range(M)])
        obs = np.stack([fr.reshape(-1), rng.integers(0, N, M * n_obs)], 1)
        ob = fz.MapObservations.from_arrays(np.arange(M + 1, dtype=np.int64) * n_obs, obs, ctx)
        dev = ob._resident(ctx)
        xyz = rng.normal(0, 1, (M, 3)) + np.array([0.0, 0.0, 8.0])
        d_x = ctx.upload(xyz)
        res = [ctx.malloc(sz * M) for sz in (4, 32, 24, 16)]

        def refresh():
            assert lib.slam_fuse_refresh(h, d_x.ptr, addr(ob.offsets), dev["obs"].ptr, M, None, M, sf.d_desc, frames.device["inverse"].ptr, sf.d_level,
                                         addr(foff), FB, d_cen.ptr, None, addr(s), L, *(o.ptr for o in res)) == 0

        timed(refresh)
        t_r = [timed(refresh) for _ in range(rounds)]
        ctx.prof_enable(True)
        k_r = []
        for _ in range(rounds):
            refresh()
            ctx.sync()
            k_r.append(ctx.prof_read()[1])
        ctx.prof_enable(False)
        best = res[0].download(np.int32, (M,))
        lists = [[(int(f), int(r)) for f, r in ob.list(m)] for m in range(n_host)]
        t0 = time.perf_counter()
        want = fuse_ref.refresh(xyz[:n_host], lists, desc.reshape(FB, N, 32), level.reshape(FB, N), cen, s)
        wall = (time.perf_counter() - t0) * 1e3
        assert np.array_equal(best[:n_host], want["best"])
        ratio = np.median(t_r) / (wall * M / n_host)
        print(f"refresh    {M:6d} points x {n_obs:3d} observations: {spread(t_r)}  {np.median(t_r) * 1e3 / M:8.3f} us / point; the kernel(s) alone: "
              f"{spread(k_r)}")
        print(f"numpy      {n_host:6d} of them on one host core: {wall:10.1f} ms wall clock, {wall * 1e3 / n_host:8.1f} us / point -> "
              f"{wall * M / n_host:10.1f} ms for all {M}; the device call takes {ratio:8.5f} of that - it "
              f"{'is faster than' if ratio < 1 else 'loses to'} the numpy statement")
        for o in (ob, d_x, *res):
            o.free()
    frames.free()
    d_cen.free()


if __name__ == "__main__":
    main()
