#!/usr/bin/env python3
"""Times the ORB extraction (slam_orb_*) and writes profiles/orb_time.log.

Device entry: events around warm launches on resident buffers, 752x480 and 640x480, B in {1, 2, 16, 64}, n_features in {200, 2000}
(the frames are the desk fixture tiled to size, each one shifted so the images of a batch differ).  Host entry: wall clock of one
frame, upload and download included.  The numpy restatement the tests compare with is timed on one frame as context, not as a
baseline.  No earlier implementation exists, so nothing is compared and nothing is gated.

    python tools/orb_time.py                      # timings -> profiles/orb_time.log
    rocprofv3 --kernel-trace --stats -d trace_orb -o orb -- python tools/orb_time.py --trace-run
    python tools/orb_time.py --split trace_orb    # appends the per-stage split of that trace to the log

With --dist the same three commands time the quadtree distribution (slam_orb_extract_dist_u8) beside the Harris
selection in one session, 752x480, B in {1, 16, 64}, n_features in {200, 2000}, and write profiles/orb_dist_time.log.
"""
import argparse
import glob
import os
import sqlite3
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "slam-experiments_amd"), os.path.join(ROOT, "tests")]
LOG = os.path.join(ROOT, "profiles", "orb_time.log")
DIST_LOG = os.path.join(ROOT, "profiles", "orb_dist_time.log")


def frames(B, H, W):
    desk = np.load(os.path.join(ROOT, "tests", "golden", "orb_desk_320x240.npz"))["image"]
    big = np.tile(desk, (H // 240 + 2, W // 320 + 2))
    return np.stack([big[7 * b % 240:7 * b % 240 + H, 11 * b % 320:11 * b % 320 + W] for b in range(B)]).copy()


def time_device(ctx, orb, B, H, W, n_features, reps, **mode):
    P = orb.OrbParams(H, W, n_features=n_features, **mode)
    ex = orb.OrbExtractor(ctx, B, P)
    try:
        ex.upload(frames(B, H, W))
        for _ in range(3):
            ex.run()
        ctx.sync()
        best = []
        for _ in range(5):
            ctx.timer_start()
            for _ in range(reps):
                ex.run()
            best.append(ctx.timer_stop() / reps)
        count = ex.download()[0]
        return min(best), float(np.median(best)), float(count.mean())
    finally:
        ex.free()


def split(where, log=LOG, what="orb_time.py --trace-run"):
    dbs = sorted(glob.glob(os.path.join(where, "**", "*_results.db"), recursive=True))
    if not dbs:
        raise SystemExit(f"no *_results.db under {where}")
    rows = sqlite3.connect(dbs[-1]).execute("select name, count(*), avg(duration), sum(duration) from kernels where name like '%orb\\_%' "
                                            "escape '\\' group by name order by sum(duration) desc").fetchall()
    total = sum(r[3] for r in rows)
    with open(log, "a") as f:
        f.write(f"\n# per-stage split: rocprofv3 --kernel-trace --stats of `{what}` (752x480, B = 16, n_features = 2000)\n")
        f.write("#   calls   avg us   share  kernel\n")
        for name, calls, avg, tot in rows:
            f.write(f"{calls:9d} {avg / 1e3:8.2f} {100 * tot / total:6.1f}%  {name.split('(')[0].replace('void ', '')}\n")
    print(open(log).read())


QUADTREE = dict(distribution="quadtree")
ADAPTIVE = dict(distribution="quadtree", fast_threshold_min=7)


def dist(ctx, orb):
    """The Harris selection, the quadtree at one threshold and the quadtree with the lower threshold 7, timed in one session."""
    lines = ["# ORB extraction at 752x480, events around warm launches on resident buffers: best / median of 5 groups, ms per call",
             "# harris = slam_orb_extract_u8; quadtree = slam_orb_extract_dist_u8 at thresholds 20 / 20; adaptive = the same at 20 / 7",
             "# mode, B, n_features: ms per call (best, median), us per frame (best), mean keypoints per frame"]
    for n_features in (200, 2000):
        for B in (1, 16, 64):
            for name, mode in (("harris", {}), ("quadtree", QUADTREE), ("adaptive", ADAPTIVE)):
                lo, med, kps = time_device(ctx, orb, B, 480, 752, n_features, 50 if B == 1 else 10, **mode)
                lines.append(f"{name:<9s} B={B:<3d} n_features={n_features:<5d} {lo:9.4f} {med:9.4f} ms   {1e3 * lo / B:9.1f} us/frame   {kps:7.1f} keypoints")
                print(lines[-1], flush=True)
    P = orb.OrbParams(480, 752, n_features=2000, **ADAPTIVE)
    ex = orb.OrbExtractor(ctx, 1, P)
    try:
        ex.upload(frames(1, 480, 752))
        ex.run()
        n = [len(ex.stage(0, l)[3][0]) for l in range(P.L)]
    finally:
        ex.free()
    lines.append(f"# candidates per level of the first frame at threshold 7: {n}; quotas {P.quota.tolist()}")
    with open(DIST_LOG, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace-run", action="store_true", help="a few launches of one shape only (to run under rocprofv3)")
    ap.add_argument("--split", metavar="DIR", help="append the per-kernel split of a rocprofv3 trace directory to the log")
    ap.add_argument("--dist", action="store_true", help="the quadtree distribution beside the Harris selection -> profiles/orb_dist_time.log")
    args = ap.parse_args()
    if args.split:
        return split(args.split, DIST_LOG, "orb_time.py --dist --trace-run") if args.dist else split(args.split)
    import slamhip
    from slamhip import orb

    ctx = slamhip.default_context()
    if args.trace_run:
        time_device(ctx, orb, 16, 480, 752, 2000, 4, **(ADAPTIVE if args.dist else {}))
        return
    if args.dist:
        return dist(ctx, orb)
    lines = ["# ORB extraction (slam_orb_extract_u8), events around warm launches on resident buffers: best / median of 5 groups, ms per call",
             "# H x W, B, n_features: ms per call (best, median), us per frame (best), mean keypoints per frame"]
    for H, W in ((480, 752), (480, 640)):
        for n_features in (200, 2000):
            for B in (1, 2, 16, 64):
                lo, med, kps = time_device(ctx, orb, B, H, W, n_features, 50 if B <= 2 else 10)
                lines.append(f"{H}x{W} B={B:<3d} n_features={n_features:<5d} {lo:9.4f} {med:9.4f} ms   {1e3 * lo / B:9.1f} us/frame   {kps:7.1f} keypoints")
                print(lines[-1], flush=True)
    lines.append("# host entry (slam_orb_extract_u8_host through orb_extract_arrays): one frame, wall clock, upload and download included")
    for H, W in ((480, 752), (480, 640)):
        img = frames(1, H, W)[0]
        for n_features in (200, 2000):
            for _ in range(3):
                orb.orb_extract_arrays(img, n_features=n_features, ctx=ctx)
            t = []
            for _ in range(20):
                t0 = time.perf_counter()
                orb.orb_extract_arrays(img, n_features=n_features, ctx=ctx)
                t.append(time.perf_counter() - t0)
            lines.append(f"{H}x{W} host call n_features={n_features:<5d} {1e3 * min(t):9.4f} {1e3 * float(np.median(t)):9.4f} ms (best, median of 20)")
            print(lines[-1], flush=True)
    import orb_ref

    lines.append("# context only, not a baseline: the numpy restatement the tests compare with (tests/orb_ref.py), one frame, one CPU thread")
    for H, W in ((480, 752), (480, 640)):
        img = frames(1, H, W)[0]
        P = orb.OrbParams(H, W, n_features=2000)
        t0 = time.perf_counter()
        want = orb_ref.extract(img, P.lh, P.lw, P.quota, P.t, P.table)
        dt = time.perf_counter() - t0
        res = orb.orb_extract_arrays(img, n_features=2000, ctx=ctx)
        same = np.array_equal(res.descriptors[0], want["descriptors"]) and np.array_equal(res.response[0], want["response"])
        lines.append(f"{H}x{W} numpy restatement n_features=2000 {1e3 * dt:9.1f} ms   device result identical: {same}")
        print(lines[-1], flush=True)
    with open(LOG, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
