"""Local-map selection and keyframe culling on the device (slamhip.local_map, csrc/local_map.hip) beside their numpy
statements, on three maps: 2 000 keyframes x 200 000 points x 10^6 observations (the map of DESIGN.md §4i) and 200 keyframes x
20 000 points x 10^5 observations; and 400 keyframes x 8 000 points whose lists hold 2 .. 256 observations (10^6 in all), where
the culling kernel runs all three of its lane-group classes.

Per map, in ONE session: the vote for B = 1 and B = 256 queries of 2 000 tracked points; the local points of the same queries
(80 local keyframes each); keyframe_redundancy for 30 candidates and for all F; cull_keyframes over 30 candidates, sequential,
with its launch count.  Each beside its ``*_host`` function on one core.  Every device time is a host clock around a whole
Python call - uploads of the query lists, allocations, launches, the downloads that end it, the frees; one warm-up run, then the
median of REPS with every run listed.  Needs the GPU; writes to stdout (kept as profiles/local_map_time.log)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "slam-experiments_amd"))
from slamhip import MapObservations, MapTables, local_map as L  # noqa: E402
from slamhip.device import default_context  # noqa: E402

REPS = 7
clock = time.perf_counter


def med(xs):
    return sorted(xs)[len(xs) // 2]


def listed(xs):
    return ", ".join(f"{x * 1e3:.3f}" for x in sorted(xs))


def make_map(F, M, seed, max_obs=8):
    """Point m is seen by 2 .. max_obs consecutive keyframes starting near m F / M (five on average at 8); the rows of a frame are its
    observations in a random order plus a fifth of rows without a point; levels 0 .. 7."""
    rng = np.random.default_rng(seed)
    n = np.minimum(rng.integers(2, max_obs + 1, M), F)
    base = np.minimum(np.arange(M, dtype=np.int64) * F // M, F - n)
    point = np.repeat(np.arange(M, dtype=np.int64), n)
    first = np.cumsum(n) - n
    frame = np.repeat(base - first, n) + np.arange(int(n.sum()))
    per_frame = np.bincount(frame, minlength=F)
    sizes = per_frame + per_frame // 5 + 1
    fo = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    row = np.zeros(len(frame), np.int64)
    order = np.argsort(frame, kind="stable")
    start = np.cumsum(per_frame) - per_frame
    for f in range(F):                                               # a random injection of the frame's observations into its rows
        row[order[start[f]:start[f] + per_frame[f]]] = rng.permutation(sizes[f])[:per_frame[f]]
    offsets = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    obs = np.stack([frame, row], 1).astype(np.int32)
    level = rng.integers(0, 8, int(fo[-1])).astype(np.int32)
    return offsets, obs, fo, level, point


def queries(F, M, B, rng):
    """B query frames spread over the map: 2 000 tracked points around the frame's place, and the 80 keyframes around it."""
    q, kf = [], []
    for b in range(B):
        f = int(rng.integers(0, F))
        lo = max(0, min(M - 4000, f * M // F - 2000))
        q.append(rng.choice(np.arange(lo, min(M, lo + 4000)), min(2000, M), replace=False))
        k0 = max(0, min(F - 80, f - 40))
        kf.append(np.arange(k0, min(F, k0 + 80)))
    return q, kf


def race(name, device, host, same):
    got, want = device(), host()                                     # warm-up: code objects, and the comparison
    equal = same(got, want)
    td, th = [], []
    for _ in range(REPS):
        t = clock()
        device()
        td.append(clock() - t)
        t = clock()
        host()
        th.append(clock() - t)
    verdict = "WINS over" if med(td) < med(th) else "LOSES to"
    print(f"{name}: device {med(td) * 1e3:.3f} ms (median of {REPS}; all: {listed(td)}) {verdict} numpy {med(th) * 1e3:.3f} ms (all: {listed(th)}), "
          f"{med(th) / med(td):.2f} x; equal in every bit: {equal}")
    sys.stdout.flush()


def same_votes(a, b):
    return all(np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in ("votes", "best", "nvoted"))


def same_lists(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))


def report(name, ctx, F, M, seed, max_obs=8):
    offsets, o, fo, level, _ = make_map(F, M, seed, max_obs)
    obs = MapObservations.from_arrays(offsets, o, ctx)
    t = clock()
    tab = MapTables.from_observations(obs, fo, level, ctx=ctx)
    built = clock() - t
    fp = tab.frame_points()
    print(f"== {name}: F={F} M={M} nnz={obs.nnz} rows={tab.n_rows}, longest list {tab.max_list} ==")
    print(f"MapTables.from_observations (uploads, the inverse table, its read-back): {built * 1e3:.2f} ms, one run; "
          f"frame_points equal to numpy's: {np.array_equal(fp, L.frame_points_host(obs, fo)[0])}")
    rng = np.random.default_rng(seed + 1)
    for B in (1, 256):
        q, kf = queries(F, M, B, rng)
        race(f"vote, B={B} queries of 2 000 points", lambda: L.local_keyframe_votes(tab, q), lambda: L.votes_host(obs, F, q), same_votes)
        race(f"local points, B={B}, 80 local keyframes each", lambda: L.local_points(tab, kf, q),
             lambda: L.local_points_host(fp, fo, M, kf, q), same_lists)
    cand = np.sort(rng.choice(F, 30, replace=False))
    pair = lambda a, b: all(np.array_equal(x, y) for x, y in zip(a, b))  # noqa: E731
    race("keyframe_redundancy, 30 candidates", lambda: L.keyframe_redundancy(tab, cand, return_flags=True),
         lambda: L.keyframe_redundancy_host(obs, fp, level, fo, cand), pair)
    race(f"keyframe_redundancy, all {F} frames", lambda: L.keyframe_redundancy(tab, None, return_flags=True),
         lambda: L.keyframe_redundancy_host(obs, fp, level, fo, None), pair)

    launches = []

    def cull_device():
        tab.set_frame_removed(np.zeros(F, np.uint8))
        tab.cull_launches = 0
        out = L.cull_keyframes(tab, cand, ratio=(1, 2), protect=())
        launches.append(tab.cull_launches)
        return out

    def cull_host():
        removed, rem, c = [], np.zeros(F, np.uint8), cand
        while len(c):
            hit = np.flatnonzero(L.redundant_verdict(L.keyframe_redundancy_host(obs, fp, level, fo, c, frame_removed=rem)[0], (1, 2)))
            if not len(hit):
                break
            rem[c[hit[0]]] = 1
            removed.append(c[hit[0]])
            c = c[hit[0] + 1:]
        return np.array(removed, np.int32)

    race("cull_keyframes, 30 candidates, sequential, more than half of the points redundant", cull_device, cull_host, np.array_equal)
    print(f"  {launches[-1]} launches of keyframe_redundancy for {launches[-1] - 1} removals")
    tab.free()
    obs.free()


if __name__ == "__main__":
    ctx = default_context()
    which = sys.argv[1:] or ["large", "small", "long"]
    if "large" in which:
        report("the map of §4i", ctx, 2000, 200000, 41)
    if "small" in which:
        report("200 keyframes", ctx, 200, 20000, 42)
    if "long" in which:                                              # lists of up to 256: all three lane-group classes of the culling kernel
        report("400 keyframes, lists of 2 .. 256", ctx, 400, 8000, 43, max_obs=256)
