"""Time of the projection search (slam_proj_match_*).  Device calls are bracketed by HIP events
(slam_timer_start/stop) around one warm call on device-resident arrays; the median and the spread (min - max) over the rounds
are reported.  Host-side lines are wall clock and say so.

    python tools/proj_match_time.py [--rounds R]

  * scene    a 752 x 480 frame of 2000 features over 8 levels at 1.2 (level l holds a share ~ 1.2^-l of them) and 256 point
             sets of 2000 map points: 1500 of each are seen by the frame (their feature within a pixel of the projection, on the
             level their distance predicts, 12 descriptor bits flipped), 500 are not; every pair has its own first pose a few
             pixels off.  And one pair of 8192 points against a frame of 8192 features.
  * grid     slam_proj_match_grid of 1 and of 256 frames (cell ids, LDS sort by (cell, row), gathers);
  * search   slam_proj_match_search of 1 pair x 2000, 1 x 8192 and 256 x 2000 points (pair table, claims, scan, finish), with
             ranges, normals and bins, th = 15;
  * window   what the library offered before for one pair: the projection in numpy on the host and window_match_arrays (one
             host call: it uploads, runs its 8 - 12 launches and reads back), wall clock.  It applies no level rule, no ratio
             between neighbours of one level and no one-to-one step, so its matches differ;
  * dense    the dense top-2 (knn2_device; knn2_device_batch in 8 launches of 32 pairs) on the same descriptors by device
             events: every point against every feature, no gate, no window.
The searches alternate with the dense top-2 in one process.  The values are a record, not a gate."""
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "slam-experiments_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import slamhip  # noqa: E402
from slamhip import proj_match as pm  # noqa: E402
from slamhip._lib import ProjParams, addr  # noqa: E402

from bow_time import opt, spread  # noqa: E402

W, H, L, SCALE = 752, 480, 8, 1.2
CAMERA = (458.654, 457.296, 367.215, 248.375)
B, N, SEEN, BIG, TH = 256, 2000, 1500, 8192, 15.0


def make_frame(rng, n):
    share = SCALE ** -np.arange(L)
    level = rng.choice(L, n, p=share / share.sum()).astype(np.int32)
    return dict(desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), level=level, bins=rng.integers(0, 32, n),
                xy=np.stack([rng.uniform(16, W - 16, n), rng.uniform(16, H - 16, n)], 1).astype(np.float32))


def make_points(rng, frame, n, seen, s):
    """n map points, the first ``seen`` (shuffled afterwards) on features of the frame under the identity pose."""
    fx, fy, cx, cy = CAMERA
    rows = rng.permutation(len(frame["level"]))[:seen]
    uv = np.concatenate([frame["xy"][rows].astype(np.float64) + rng.normal(0, 0.4, (seen, 2)),
                         np.stack([rng.uniform(0, W, n - seen), rng.uniform(0, H, n - seen)], 1)])
    level = np.concatenate([frame["level"][rows], rng.integers(0, L, n - seen)])
    z = rng.uniform(1.5, 15.0, n)
    xyz = np.stack([(uv[:, 0] - cx) / fx * z, (uv[:, 1] - cy) / fy * z, z], 1)
    d = np.linalg.norm(xyz, axis=1)
    dmax = np.where(level == 0, d * 1.01, d * s[level] * (1.0 - rng.uniform(0.05, 0.8, n) * (1.0 - 1.0 / SCALE)))
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    desc[:seen] = frame["desc"][rows]
    bit = np.stack([rng.permutation(256)[:12] for _ in range(seen)])
    for k in range(12):
        desc[np.arange(seen), bit[:, k] >> 3] ^= (1 << (bit[:, k] & 7)).astype(np.uint8)
    bins = np.concatenate([(frame["bins"][rows] + 2) % 32, rng.integers(0, 32, n - seen)])
    o = rng.permutation(n)
    return dict(xyz=xyz[o], desc=desc[o], dmin2=(0.5 * dmax[o] / s[-1]) ** 2, dmax2=dmax[o] ** 2, normal=(xyz / d[:, None])[o], bins=bins[o])


def first_pose(rng):
    w = rng.normal(0, 0.002, 3)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.c_[np.eye(3) + K + 0.5 * K @ K, rng.normal(0, 0.01, 3)]


def main():
    rounds = max(9, opt("--rounds", 9))
    ctx = slamhip.default_context()
    lib, h = ctx.lib, ctx.handle
    rng = np.random.default_rng(2107)
    s, s2 = pm.scale_tables(L, SCALE)

    def timed(fn):
        ctx.timer_start()
        fn()
        return ctx.timer_stop()

    print(slamhip.load().slam_version().decode())
    print(f"plan for {B} frames, {B} pairs of {N}: {pm.plan_describe(B, B, N)}")
    print(f"plan for 1 frame, 1 pair of {BIG}: {pm.plan_describe(1, 1, BIG)}")
    frame, big_frame = make_frame(rng, N), make_frame(rng, BIG)
    sets = [make_points(rng, frame, N, SEEN, s) for _ in range(B)]
    big = make_points(rng, big_frame, BIG, 6000, s)
    cat = lambda k: np.concatenate([p[k] for p in sets])  # noqa: E731
    ps = pm.PointSets(cat("xyz"), cat("desc"), np.arange(B + 1) * N, cat("dmin2"), cat("dmax2"), cat("normal"), None, cat("bins"), ctx=ctx)
    ps_big = pm.PointSets(big["xyz"], big["desc"], None, big["dmin2"], big["dmax2"], big["normal"], None, big["bins"], ctx=ctx)

    # ---- the grid step: 1 and 256 frames (256 copies of the frame's arrays, resident)
    many = {k: np.concatenate([frame[k]] * B) for k in frame}
    d_in = [ctx.upload(many["desc"]), ctx.upload(many["xy"]), ctx.upload(many["level"])]
    d_out = [ctx.malloc(sz * B * N) for sz in (4, 32, 4, 4, 4, 8, 4)]
    off = np.arange(B + 1, dtype=np.int64) * N
    for images in (1, B):
        def grid():
            assert lib.slam_proj_match_grid(h, d_in[0].ptr, d_in[1].ptr, d_in[2].ptr, None, addr(off), images, W, H, pm.CELL, *(o.ptr for o in d_out)) == 0

        timed(grid)
        v = [timed(grid) for _ in range(rounds)]
        print(f"grid       {images:3d} frame(s) of {N} rows, cell {pm.CELL}: {spread(v)}  {np.median(v) * 1e3 / images:8.2f} us / frame")
    for o in d_in + d_out:
        o.free()

    fg = pm.FrameGrids.from_arrays(frame["desc"], frame["xy"], frame["level"], (W, H), bins=frame["bins"], ctx=ctx)
    fg_big = pm.FrameGrids.from_arrays(big_frame["desc"], big_frame["xy"], big_frame["level"], (W, H), bins=big_frame["bins"], ctx=ctx)
    d_frame, d_big_frame = ctx.upload(frame["desc"]), ctx.upload(big_frame["desc"])
    d_m, d_c = ctx.malloc(4 * B * N), ctx.malloc(4 * B)
    tab_i, tab_d = ctx.malloc(8 * B * N), ctx.malloc(8 * B * N)
    poses = np.ascontiguousarray(np.stack([first_pose(rng) for _ in range(B)]))
    centres = pm.camera_centres(poses)
    th = np.full(B, TH)
    prm = ProjParams(*CAMERA, 0.0, float(W), 0.0, float(H), pm.COS2_LIMIT, pm.RATIO, addr(s), addr(s2), L, pm.TH_HIGH, 1, -1, 0, 0)
    pairs = np.stack([np.arange(B), np.zeros(B, np.int64)], 1).astype(np.int32)

    def dense_device(P, d_q, n, d_t, m):
        if P == 1:
            slamhip.knn2_device(ctx, d_q.view(0, 32 * n), n, d_t, m, tab_i.view(0, 8 * n), tab_d.view(0, 8 * n))
            return
        for g in range(0, P, 32):
            slamhip.knn2_device_batch(ctx, [(d_q.view(32 * n * p, 32 * n), n, d_t, m, tab_i.view(8 * n * p, 8 * n), tab_d.view(8 * n * p, 8 * n))
                                            for p in range(g, min(P, g + 32))])

    for name, P, n, points, frames, d_t in (("1 x 2000", 1, N, ps, fg, d_frame), ("1 x 8192", 1, BIG, ps_big, fg_big, d_big_frame),
                                           ("256 x 2000", B, N, ps, fg, d_frame)):
        sp, sf = points._struct(ctx), frames._struct(ctx)

        def search():
            assert lib.slam_proj_match_search(h, ctypes.byref(sp), ctypes.byref(sf), addr(pairs), addr(poses), addr(centres), addr(th), P,
                                              ctypes.byref(prm), d_m.ptr, d_c.ptr, *[None] * 6) == 0

        d_q = points.device["desc"]
        timed(search)
        timed(lambda: dense_device(P, d_q, n, d_t, n))
        t_s, t_d = [], []
        for _ in range(rounds):                             # alternating in one process
            t_s.append(timed(search))
            t_d.append(timed(lambda: dense_device(P, d_q, n, d_t, n)))
        found = int(d_c.download(np.int32, (P,)).sum())
        ctx.prof_enable(True)                               # the scan kernel alone, by the library's own event bracket
        t_k = []
        for _ in range(rounds):
            search()
            ctx.sync()
            t_k.append(ctx.prof_read()[1])
        ctx.prof_enable(False)
        print(f"search     {name:>10} points, th {TH:g}: {spread(t_s)}  {np.median(t_s) * 1e3 / P:8.2f} us / pair, {found / P:.0f} matches / pair")
        print(f"scan       {name:>10} pm_scan_kernel alone: {spread(t_k)}  (the rest of the call: copy of the pair table, memset, finish)")
        print(f"dense      {name:>10} top-2 alone:    {spread(t_d)}  {np.median(t_d) * 1e3 / P:8.2f} us / pair  ({(P + 31) // 32} launch(es))")
        ratio = np.median(t_s) / np.median(t_d)
        print(f"ratio      {name:>10}: the projection search takes {ratio:6.3f} of the dense top-2's device time - it "
              f"{'is faster than' if ratio < 1 else 'loses to'} the dense search's device part")

    # ---- the lone pair through the window search of 3e: projection on the host, one host call
    p0, fx, fy, cx, cy = sets[0], *CAMERA
    A = poses[0]

    def window():
        c = p0["xyz"] @ A[:, :3].T + A[:, 3]
        uv = np.stack([fx * c[:, 0] / c[:, 2] + cx, fy * c[:, 1] / c[:, 2] + cy], 1).astype(np.float32)
        return slamhip.window_match_arrays(frame["desc"], p0["desc"], frame["xy"], uv, TH * s[3], k=2, ctx=ctx)

    window()
    wall = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        idx, _ = window()
        wall.append((time.perf_counter() - t0) * 1e3)
    print(f"window     {'1 x 2000':>10} host projection + window_match_arrays (radius {TH * s[3]:.1f}, features as queries): "
          f"{spread(wall)}  wall clock, one host call with its copies; {int((idx[:, 0] >= 0).sum())} features with a neighbour "
          f"(no level, ratio-by-level or one-to-one rule: not the same matches)")
    for o in (ps, ps_big, fg, fg_big, d_frame, d_big_frame, d_m, d_c, tab_i, tab_d):
        o.free()


if __name__ == "__main__":
    main()
