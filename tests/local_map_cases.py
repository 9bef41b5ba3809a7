"""Shared cases of the local-map tests: maps as plain Python lists (a ``Scene``), sized from ``slam_lmap_limits`` where a size
decides which form of a kernel runs.  Built once per process and never changed."""
import functools

import numpy as np

TH = 3                                        # KeyFrameCulling's th_obs in every designed case


class Scene:
    """``lists[m]`` the (frame, row) pairs of point m (frames ascending), ``frame_offsets`` int64 [F+1], ``level`` int32 [n] in
    row order; ``removed`` / ``bad``: sorted lists of frames / points the masks set."""

    def __init__(self, F, lists, frame_offsets, level, removed=(), bad=(), notes=None):
        self.F, self.M, self.lists = F, len(lists), lists
        self.frame_offsets, self.level = np.asarray(frame_offsets, np.int64), np.asarray(level, np.int32)
        self.removed, self.bad = sorted(removed), sorted(bad)
        self.notes = notes or {}

    @property
    def n_rows(self):
        return int(self.frame_offsets[-1])

    def mask(self, which):
        m = np.zeros(self.F if which == "removed" else self.M, np.uint8)
        m[getattr(self, which)] = 1
        return m

    def observations(self, ctx=None):
        from slamhip import MapObservations

        return MapObservations.from_lists(self.lists, ctx)

    def tables(self, ctx):
        """(MapTables, MapObservations) on ``ctx``; the caller frees both."""
        from slamhip import MapTables

        obs = self.observations(ctx)
        try:
            return MapTables.from_observations(obs, self.frame_offsets, self.level, self.mask("removed"), self.mask("bad"), ctx=ctx), obs
        except BaseException:
            obs.free()
            raise


def from_tracks(F, tracks, seed, spare=1, levels=None, n_levels=8, removed=(), bad=(), empty_frames=(), notes=None):
    """``tracks[m]``: the frames that see point m (any order, no frame twice).  Every frame gets one row per point it sees
    and ``spare`` rows without a point, shuffled; ``levels[(m, f)]`` fixes the level of an observation, the rest are random."""
    rng = np.random.default_rng(seed)
    per_frame = [[] for _ in range(F)]
    for m, fs in enumerate(tracks):
        for f in fs:
            per_frame[f].append(m)
    row_of, sizes = {}, []
    for f in range(F):
        n = 0 if f in empty_frames else len(per_frame[f]) + spare
        perm = rng.permutation(n)
        for k, m in enumerate(per_frame[f]):
            row_of[(m, f)] = int(perm[k])
        sizes.append(n)
    fo = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    level = rng.integers(0, n_levels, int(fo[-1])).astype(np.int32)
    for (m, f), l in (levels or {}).items():
        level[fo[f] + row_of[(m, f)]] = l
    lists = [[(f, row_of[(m, f)]) for f in sorted(fs)] for m, fs in enumerate(tracks)]
    return Scene(F, lists, fo, level, removed, bad, notes)


def random_tracks(rng, F, M, max_obs, hot=()):
    """M tracks of 1 .. max_obs frames out of F; the frames ``hot`` are in every fourth track."""
    tracks = []
    for m in range(M):
        n = int(rng.integers(1, min(max_obs, F) + 1))
        fs = set(int(f) for f in rng.choice(F, n, replace=False))
        if hot and m % 4 == 0:
            fs |= set(hot)
        tracks.append(sorted(fs))
    return tracks


def limits():
    from slamhip import local_map

    return local_map.limits()


# ---- culling ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def cull_lengths():
    """Frame 0 sees one point of every list length around the lane-group sizes (and 1, 2 and 256); point i of length n is seen
    by frames 0 .. n - 1.  Frames 300 .. 302: no rows at all, only rows without a point, only bad points."""
    lim = limits()
    lengths = sorted({1, 2, TH, TH + 1, 256} | {g + d for g in (lim["group16"], lim["group64"]) for d in (-1, 0, 1)} | {lim["group256"] - 1})
    tracks = [list(range(n)) for n in lengths] * 2
    tracks += [[302], [302, 5], [7]]                                   # two bad points of frame 302 and a filler
    bad = [len(tracks) - 3, len(tracks) - 2]
    return from_tracks(303, tracks, 11, spare=2, n_levels=3, bad=bad, empty_frames=(300,), notes=dict(lengths=lengths))


@functools.lru_cache(None)
def cull_designed():
    """Every boundary of the rule with th_obs = 3, one candidate frame each (the notes name them):

    exact      c = 0: a point with N = 3 observers (never redundant) and one with N = 4, all at the candidate's level (redundant)
    short      c = 1: N = 5 but only 2 observers within a level of the candidate's (level 0 against 0, 1, 2, 2) - not redundant
    levels     c = 2: candidate at level 14; observers at 15, 15, 15 (redundant) / at 15, 15 and one of a point whose candidate
               row is at level 13 (15 = l + 2: does not count) - one redundant, one not
    own        c = 3: N = 4 with the candidate's own observation the only one besides 2 qualifying ones - not redundant
    nine       c = 4: ten points, nine redundant (kept at 9/10: 90 > 90 is false; culled at ratio (0, 1))
    ten        c = 5: ten points, ten redundant (culled)
    removed    c = 6: N = 4 of which frame 20 is removed: N = 3, not redundant; c = 20 itself is a removed candidate
    twins      c = 7 and 8: thirty points seen by 7, 8, 9 and 10 only; 9 and 10 see sixty more alone
    """
    t, lv = [], {}

    def point(frames, levels):
        t.append(sorted(frames))
        for f, l in zip(frames, levels):
            lv[(len(t) - 1, f)] = l

    point([0, 11, 12], [2, 2, 2])
    point([0, 11, 12, 13], [2, 2, 2, 2])
    point([1, 11, 12, 13, 14], [0, 0, 1, 2, 2])
    point([2, 11, 12, 13], [14, 15, 15, 15])
    point([2, 11, 12, 13], [13, 15, 14, 14])
    point([3, 11, 12, 13], [5, 6, 6, 8])
    for k in range(10):
        point([4, 11, 12, 13], [3, 3, 3, 3] if k else [3, 3, 3, 5])
    for k in range(10):
        point([5, 11, 12, 13], [3, 4, 0, 2])
    point([6, 11, 12, 20], [1, 1, 1, 1])
    point([20, 11, 12, 13, 14], [1, 1, 1, 1, 1])
    for k in range(30):
        point([7, 8, 9, 10], [2, 2, 2, 2])
    for k in range(60):
        point([9, 10], [2, 2])
    return from_tracks(21, t, 12, spare=1, levels=lv, n_levels=16, removed=[20],
                       notes=dict(exact=0, short=1, levels=2, own=3, nine=4, ten=5, removed=6, removed_candidate=20, twins=(7, 8)))


@functools.lru_cache(None)
def cull_random():
    rng = np.random.default_rng(13)
    return from_tracks(40, random_tracks(rng, 40, 900, 9, hot=(3, 4, 5, 6)), 14, spare=3, n_levels=4, removed=[4, 17], bad=[0, 5, 77, 899])


def cull_scenes():
    return {"lengths": cull_lengths(), "designed": cull_designed(), "random": cull_random()}


def candidate_sets(scene):
    """C = 0, 1, some in an order of their own (one twice), and all F (None)."""
    F = scene.F
    return {"none": [], "one": [min(7, F - 1)], "some": [F - 1, 0, 2, 2, min(20, F - 1), 1], "all": None}


# ---- the vote ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def vote_scene(F):
    """300 points over F frames; the last frame and frames 0 .. 2 are in every fourth track, frame 1 is removed where it exists
    beside others, point 8 is bad."""
    rng = np.random.default_rng(100 + F % 97)
    hot = sorted({0, min(2, F - 1), F - 1})
    return from_tracks(F, random_tracks(rng, F, 300, 6, hot=hot), 15, spare=0, removed=[1] if F > 3 else [], bad=[8])


def vote_sizes():
    """F = 1, a few, and one below, at and one above both LDS sizes."""
    lim = limits()
    return [1, 2, 37] + [c + d for c in (lim["vote_lds_small"], lim["vote_lds_frames"]) for d in (-1, 0, 1)]


def vote_queries(scene, B):
    """B query lists: one without points, one of -1 only, one with a point repeated, one with entries out of range, one that
    ties two frames at the maximum, the rest random."""
    rng = np.random.default_rng(200 + B)
    M = scene.M
    special = [[], [-1, -1, -1], [4, 4, 4, 12, 4], [0, M, -7, 8, 3, 1 << 30], [0, 4, 8, 12, 16, 20, 24]]
    out = []
    for b in range(B):
        if B > 1 and b < len(special):
            out.append(np.array(special[b], np.int64))
        else:
            q = rng.integers(0, M, int(rng.integers(1, 120)))
            q[rng.uniform(size=len(q)) < 0.1] = -1
            out.append(q.astype(np.int64))
    return out


@functools.lru_cache(None)
def tie_scene():
    """Frames 5 and 2 both get three votes from the query [0, 1, 2]; frame 7 gets one: the lowest index wins."""
    return from_tracks(9, [[5, 2], [2, 5], [5, 2, 7], [8]], 16, spare=1)


# ---- local points -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def points_scene(M):
    """M points over 6 frames: point m is seen by frame m % 5 and, every third, by frame (m + 1) % 5 too - overlapping
    keyframes; frame 5 sees none.  The last point is seen, a few are bad."""
    tracks = [sorted({m % 5, (m + 1) % 5} if m % 3 == 0 else {m % 5}) for m in range(M)]
    bad = sorted({1, M // 2, M - 2} & set(range(M)))
    return from_tracks(6, tracks, 17, spare=1, bad=bad, removed=[3])


def points_sizes():
    """M around a bitmap word and around a scan tile of bitmap words, and two tiles and a word."""
    bits = 32 * limits()["scan_tile_words"]
    return [31, 32, 33, bits - 1, bits, bits + 1, 2 * bits + 33]


def points_queries(scene):
    """(local keyframes, tracked points) of three queries: all frames with a few tracked; nothing (the empty middle query);
    frames 0, 1, 0 and 3 (removed) with every point of the map tracked already."""
    M = scene.M
    return [[0, 1, 2, 3, 4, 5], [], [0, 1, 0, 3]], [np.array([0, -1, 2, 2]), np.array([5]), np.arange(M)]
