#!/usr/bin/env python3
"""Times stereo matching (slam_stereo_match) and writes profiles/stereo_time.log.

752 x 480, 2000 features a side, 8 levels; the frames are the desk fixture tiled to size, the right frame of pair b cut 9 + b
columns further right, so a pair has a true disparity.  One extractor holds the left and the right frames; its buffers stay
resident.  Events (slam_timer_start / stop) around one warm call, the median and the spread of 7; for 1 pair and for 64 pairs:

  * the whole call (two small copies and three launches);
  * the dense top-2 Hamming search of the same rows alone (knn2_device per pair), for scale;
  * the numpy statement (tests/stereo_ref.py) of one pair on one host core, by the host clock, once.

    python tools/stereo_time.py                                   # -> profiles/stereo_time.log
    rocprofv3 --kernel-trace --stats -d trace_st1 -o st -- python tools/stereo_time.py --trace-run 1
    python tools/stereo_time.py --split trace_st1 1               # appends each launch apart (also for 64)

The values are a record, not a gate."""
import argparse
import ctypes
import glob
import os
import sqlite3
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "slam-experiments_amd"), os.path.join(ROOT, "tests")]
LOG = os.path.join(ROOT, "profiles", "stereo_time.log")
H, W, FEATURES, LEVELS = 480, 752, 2000, 8
FX, BF = 458.654, 458.654 * 0.11


def frames(B):
    desk = np.load(os.path.join(ROOT, "tests", "golden", "orb_desk_320x240.npz"))["image"]
    big = np.tile(desk, (H // 240 + 2, W // 320 + 3))
    left = [big[7 * b % 240:7 * b % 240 + H, 11 * b % 320:11 * b % 320 + W] for b in range(B)]
    right = [big[7 * b % 240:7 * b % 240 + H, 11 * b % 320 + 9 + b:11 * b % 320 + 9 + b + W] for b in range(B)]
    return np.stack(left + right).copy()


class Scene:
    """An extractor of 2 B frames after run(), and the buffers of one stereo call on its B pairs."""

    def __init__(self, ctx, B):
        from slamhip import orb, stereo

        self.ctx, self.B = ctx, B
        self.P = orb.OrbParams(H, W, n_features=FEATURES, n_levels=LEVELS)
        self.ex = orb.OrbExtractor(ctx, 2 * B, self.P)
        self.ex.upload(frames(B))
        self.ex.run()
        ctx.sync()
        self.pairs = np.ascontiguousarray(np.stack([np.arange(B), B + np.arange(B)], 1), np.int32)
        self.scale = stereo.scale_table(self.P.scale, self.P.L)
        need = ctypes.c_uint64(0)
        assert ctx.lib.slam_stereo_workspace(B, self.P.n_max, ctypes.byref(need)) == 0
        slots = B * self.P.n_max
        self.need = need.value
        self.bufs = [ctx.malloc(self.need)] + [ctx.malloc(n * slots) for n in (4, 8, 8, 4, 4, 1)] + [ctx.malloc(8 * B)]
        lay = self.ex.layout
        self.off = np.ascontiguousarray(lay["image"], np.uint64)
        self.pitch = np.ascontiguousarray(lay["pitch"], np.int32)

    def call(self):
        ex, P, b = self.ex, self.P, self.bufs
        blk = (2 * self.B, ex.bufs["count"].ptr, ex.bufs["kp"].ptr, ex.bufs["desc"].ptr, ex.bufs["ws"].ptr)
        rc = self.ctx.lib.slam_stereo_match(self.ctx.handle, self.B, self.pairs.ctypes.data, *blk, *blk, P.n_max, P.L, ex.layout["image_base"],
                                            ex.layout["image_stride"], self.off.ctypes.data, self.pitch.ctypes.data, P.lw.ctypes.data,
                                            P.lh.ctypes.data, self.scale.ctypes.data, BF, 0.0, FX, 75, 5, 5, 1, b[0].ptr, self.need,
                                            *[x.ptr for x in b[1:]])
        assert rc == 0, self.ctx.lib.slam_last_error()

    def counts(self):
        return self.bufs[7].download(np.int32, (self.B, 2))

    def status(self):
        return self.bufs[6].download(np.uint8, (self.B, self.P.n_max))

    def free(self):
        for x in self.bufs:
            x.free()
        self.ex.free()


def spread(v):
    return f"{np.median(v) * 1e3:10.1f} us  [{min(v) * 1e3:9.1f} - {max(v) * 1e3:9.1f}]"


def split(where, pairs):
    dbs = sorted(glob.glob(os.path.join(where, "**", "*_results.db"), recursive=True))
    if not dbs:
        raise SystemExit(f"no *_results.db under {where}")
    rows = sqlite3.connect(dbs[-1]).execute("select name, count(*), avg(duration), min(duration), max(duration) from kernels where name like '%stereo\\_%' "
                                            "escape '\\' group by name order by avg(duration) desc").fetchall()
    with open(LOG, "a") as f:
        f.write(f"\n# each launch apart, {pairs} pair(s): rocprofv3 --kernel-trace --stats of `stereo_time.py --trace-run {pairs}`\n")
        f.write("#   calls   avg us   min us   max us  kernel\n")
        for name, calls, avg, lo, hi in rows:
            f.write(f"{calls:9d} {avg / 1e3:8.2f} {lo / 1e3:8.2f} {hi / 1e3:8.2f}  {name.split('(')[0].replace('void ', '')}\n")
    print(open(LOG).read())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--trace-run", type=int, metavar="PAIRS", help="a few calls of one shape only (to run under rocprofv3)")
    ap.add_argument("--split", nargs=2, metavar=("DIR", "PAIRS"), help="append the per-kernel times of a rocprofv3 trace directory to the log")
    args = ap.parse_args()
    if args.split:
        return split(args.split[0], int(args.split[1]))
    import slamhip
    import stereo_ref as ref

    ctx = slamhip.default_context()
    if args.trace_run:
        s = Scene(ctx, args.trace_run)
        for _ in range(10):
            s.call()
        ctx.sync()
        return s.free()

    def timed(fn):
        ctx.timer_start()
        fn()
        return ctx.timer_stop()

    lines = [slamhip.load().slam_version().decode(),
             f"# slam_stereo_match, {W} x {H}, {FEATURES} features a side, {LEVELS} levels, resident buffers; events around one warm call: median [min - max] of "
             f"{args.rounds}"]
    for B in (1, 64):
        s = Scene(ctx, B)
        try:
            timed(s.call)
            v = [timed(s.call) for _ in range(args.rounds)]
            counts, status = s.counts(), s.status()
            n = s.ex.download()[0]
            lines.append(f"whole call  P = {B:2d}: {spread(v)}  {np.median(v) * 1e3 / B:8.1f} us / pair | rows per image {n.mean():.0f}, status 0 per pair "
                         f"{counts[:, 0].mean():.0f}, accepted before the median {counts[:, 1].mean():.0f}, statuses of pair 0 "
                         f"{np.bincount(status[0, :n[0]], minlength=7).tolist()}")
            tab = slamhip.Top2Table(ctx, s.P.n_max)
            desc = s.ex.bufs["desc"]

            def dense():
                for b in range(B):
                    slamhip.knn2_device(ctx, desc.view(b * s.P.n_max * 32, int(n[b]) * 32), int(n[b]), desc.view((B + b) * s.P.n_max * 32, int(n[B + b]) * 32),
                                        int(n[B + b]), tab.idx, tab.dist)

            timed(dense)
            v2 = [timed(dense) for _ in range(args.rounds)]
            tab.free()
            lines.append(f"dense top-2 P = {B:2d}: {spread(v2)}  {np.median(v2) * 1e3 / B:8.1f} us / pair  (knn2_device of the same rows, one call per pair: no gates, no SAD)")
            if B == 1:
                count, kp, _, dsc = s.ex.download()
                blk = dict(count=count, kp=kp, desc=dsc, planes=[[s.ex.stage(b, l)[0] for l in range(LEVELS)] for b in range(2)])
                t = time.perf_counter()
                want = ref.match(s.pairs, blk, blk, s.scale, bf=BF, max_d=FX)
                t = time.perf_counter() - t
                assert np.array_equal(want["status"], status) and np.array_equal(want["counts"], counts)
                lines.append(f"numpy statement, one pair, one host core, host clock, once: {t * 1e3:10.1f} ms  (the device's statuses and counts equal it)")
            print("\n".join(lines[-3:]), flush=True)
        finally:
            s.free()
    lines.append("# not measured: other image sizes and feature counts, L other than 8, w and Ls other than 5, the Python layer with its downloads")
    with open(LOG, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
