"""Local-map selection and keyframe culling by brute force: Python sets per point and dicts per frame, no numpy bincount and no
sort.  The rules are exact integers, so this is the truth the ``*_host`` functions of slamhip.local_map and the device must
equal with ``np.array_equal``.  ``lists[m]`` is the observation list of point m as (frame, row) pairs; ``removed`` and ``bad``
are sets of frames and of points."""
import numpy as np


def frame_points_ref(lists, frame_offsets):
    """(frame_points int32 [n], slots out of range, claims of a row that already had a point)"""
    fo = [int(v) for v in frame_offsets]
    F = len(fo) - 1
    claims = {}
    out_of_range = 0
    for m, lst in enumerate(lists):
        for f, r in lst:
            if not (0 <= f < F and 0 <= r < fo[f + 1] - fo[f]):
                out_of_range += 1
                continue
            claims.setdefault(fo[f] + r, []).append(m)
    fp = np.full(fo[-1], -1, np.int32)
    twice = 0
    for at, ms in claims.items():
        fp[at] = max(ms)
        twice += len(ms) - 1
    return fp, out_of_range, twice


def votes_ref(lists, F, queries, removed=(), bad=()):
    """dict(votes int32 [B,F], best int32 [B,2], nvoted int32 [B], skipped)"""
    removed, bad, M = set(removed), set(bad), len(lists)
    votes = np.zeros((len(queries), F), np.int32)
    best = np.zeros((len(queries), 2), np.int32)
    nvoted = np.zeros(len(queries), np.int32)
    skipped = 0
    for b, query in enumerate(queries):
        tally = {}
        for m in query:
            m = int(m)
            if m == -1:
                continue
            if not 0 <= m < M:
                skipped += 1
                continue
            if m in bad:
                continue
            for f, _ in lists[m]:
                if not 0 <= f < F:
                    skipped += 1
                elif f not in removed:
                    tally[f] = tally.get(f, 0) + 1
        top = (-1, 0)
        for f, v in tally.items():
            votes[b, f] = v
            if v > top[1] or (v == top[1] and f < top[0]):
                top = (f, v)
        best[b] = top
        nvoted[b] = len(tally)
    return dict(votes=votes, best=best, nvoted=nvoted, skipped=skipped)


def local_points_ref(frame_points, frame_offsets, M, keyframes, queries, removed=(), bad=()):
    """per query the int32 array of its local points, ascending"""
    removed, bad = set(removed), set(bad)
    fo = [int(v) for v in frame_offsets]
    F = len(fo) - 1
    out = []
    for kfs, query in zip(keyframes, queries):
        local = set()
        for f in kfs:
            f = int(f)
            if 0 <= f < F and f not in removed:
                for r in range(fo[f], fo[f + 1]):
                    m = int(frame_points[r])
                    if 0 <= m < M and m not in bad:
                        local.add(m)
        local -= {int(m) for m in query}
        out.append(np.array([m for m in range(M) if m in local], np.int32))
    return out


def redundancy_ref(lists, frame_points, level, frame_offsets, candidates=None, th_obs=3, removed=(), bad=()):
    """(counts int32 [C,2], flags u8 per candidate row in candidate order)"""
    removed, bad = set(removed), set(bad)
    fo = [int(v) for v in frame_offsets]
    F = len(fo) - 1
    cand = range(F) if candidates is None else [int(c) for c in candidates]
    counts, flags = [], []
    for c in cand:
        n_points = n_redundant = 0
        for r in range(fo[c], fo[c + 1]):
            m = int(frame_points[r])
            if c in removed or m < 0 or m in bad:
                flags.append(0)
                continue
            observers = [(f, rr) for f, rr in lists[m] if f not in removed]
            near = [1 for f, rr in observers if f != c and int(level[fo[f] + rr]) <= int(level[r]) + 1]
            n_points += 1
            if len(observers) > th_obs and len(near) >= th_obs:
                n_redundant += 1
                flags.append(2)
            else:
                flags.append(1)
        counts.append((n_points, n_redundant))
    return np.array(counts, np.int32).reshape(-1, 2), np.array(flags, np.uint8)
