"""Cases for the forms of csrc/covis.hip that the size of the problem selects and tests/covis_cases.py never reaches: 64-bit
observation keys, 64-bit pair keys over several sort tiles and six passes, scans three levels deep, one list of thousands, and
``cv_rows`` on a large map.  Shared by tests/test_covis_edges_cpu.py (the cases' own properties, the closed forms against the
brute force) and tests/test_covis_edges_gpu.py (the device against both).

A case is ``(K, L, obs_pose, obs_point, fixed)`` as in covis_cases.  Every case is built when a test asks for it, never at
import or collection; the small ones and their expected tables are kept, the ones of millions of pairs are not.  Sizes at which
the kernels change their path come from ``slam_covis_limits``."""
import numpy as np

import covis_cases as C
from covis_ref import covisibility_ref

_cache = {}
limits = C.limits


def bitlen(v):
    return int(v).bit_length()


def scan_levels(n):
    """Levels ``cv_scan`` takes over n entries: one more for every time the block totals do not fit one scan tile."""
    tile, levels = limits()["scan_tile"], 1
    m = -(-max(int(n), 1) // tile)
    while m > 1:
        m, levels = -(-m // tile), levels + 1
    return levels


def masked(case, on):
    """The case with its mask, or in graph mode (nothing fixed)."""
    return case if on else case[:4] + (None,)


def expected(name, case, on):
    """The five tables of the case by brute force (tests/covis_ref.py), computed once."""
    key = ("expected", name, bool(on))
    if key not in _cache:
        K, L, op, ol, fixed = masked(case, on)
        _cache[key] = covisibility_ref(op, ol, K, fixed)
    return _cache[key]


def _distinct_rows(rng, K, n, width):
    """int64 [n, width]: in every row ``width`` different poses of [0, K), each drawn over all of [0, K)."""
    rows = rng.integers(0, K, (n, width))
    while True:
        s = np.sort(rows, 1)
        bad = (s[:, 1:] == s[:, :-1]).any(1)
        if not bad.any():
            return rows
        rows[bad] = rng.integers(0, K, (int(bad.sum()), width))


def _shuffled(rng, op, ol):
    perm = rng.permutation(len(op))
    return np.ascontiguousarray(op[perm], np.int32), np.ascontiguousarray(ol[perm], np.int32), perm


# ---- 1. the width of the observation key ---------------------------------------------------------------------------------------
def width_sizes():
    """{name: (K, L, obs key bits, obs key bytes, obs passes, pair key bits, pair key bytes, pair passes)}: the bits of the
    observation key at 31, 32 and 33 beside 32-bit and 64-bit pair keys, and the largest K."""
    from slamhip.pose_graph import MAX_VERTICES

    K32 = limits()["key32_max_K"]
    out = {}
    for K, obits in ((K32, 31), (K32, 32), (K32, 33), (K32 + 1, 32), (K32 + 1, 33), (MAX_VERTICES, 46)):
        pb = bitlen(K - 1)
        # the largest L of that many bits, and the smallest where the key outgrows 32
        L = 1 << 20 if K == MAX_VERTICES else (1 << (obits - pb - 1)) - 1 if obits <= 32 else 1 << (32 - pb - 1)
        pbits = bitlen(K * K - 1)
        out[f"K{K}-L{L}"] = (K, L, obits, 4 if obits <= 32 else 8, -(-obits // 8), pbits, 4 if pbits <= 32 else 8, -(-pbits // 8))
    return out


WIDTH_POINTS, WIDTH_LONG_TRACKS = 12000, 4000


def width_case(name):
    """12 000 observed points drawn over all of [0, L) except two at either end, 4 000 of them seen by two to four poses and
    the rest by one to four, poses drawn over all of [0, K); every pose that is 5 mod 8 is fixed.  Point order: the edges
    (0, K-1), (K-2, K-1) and (0, 1), then a point seen by two fixed poses only."""
    if ("width", name) not in _cache:
        K, L = width_sizes()[name][:2]
        rng = np.random.default_rng(1000 + K % 1000 + L % 1000)
        points = 2 + rng.choice(L - 4, WIDTH_POINTS, replace=False)
        lengths = rng.integers(1, 5, WIDTH_POINTS)
        lengths[:WIDTH_LONG_TRACKS] = rng.integers(2, 5, WIDTH_LONG_TRACKS)
        rows = _distinct_rows(rng, K, WIDTH_POINTS, 4)
        fixed = np.arange(K) % 8 == 5
        top_fixed = (K - 6) // 8 * 8 + 5
        for t, pair in enumerate(((0, K - 1), (K - 2, K - 1), (0, 1), (5, top_fixed))):
            rows[t, :2], lengths[t] = pair, 2
        assert not fixed[[0, 1, K - 2, K - 1]].any() and fixed[[5, top_fixed]].all()
        take = np.arange(4)[None, :] < lengths[:, None]
        op, ol, _ = _shuffled(rng, rows[take], np.repeat(points, lengths))
        _cache["width", name] = (K, L, op, ol, fixed)
    return _cache["width", name]


def with_bad_entries(case, seed):
    """The case with 24 observations out of range spread through its list: poses -1, K and 2^30, points -1, L and 2^30, on
    either side valid or not.  -> (case, how many)."""
    K, L, op, ol, fixed = case
    bad = np.array([(-1, 0), (K, 7), (0, L), (1 << 30, L - 1), (3, -1), (5, 1 << 30), (K, L), (-1, -1)] * 3, np.int64)
    at = np.sort(np.random.default_rng(seed).choice(len(op) + 1, len(bad), replace=False))
    return (K, L, np.insert(op, at, bad[:, 0]).astype(np.int32), np.insert(ol, at, bad[:, 1]).astype(np.int32), fixed), len(bad)


# ---- 2. 64-bit pair keys over more than one sort tile ------------------------------------------------------------------------------
LONG_RUN = 3000


def pair_key_sizes():
    from slamhip.pose_graph import MAX_VERTICES

    T = limits()["sort_tile"]
    return {f"K{K}-P{P}": (K, P) for K in (70000, MAX_VERTICES) for P in (T - 1, T, T + 1, 2 * T + 1)}


def pair_key_case(name):
    """P points of two poses each, so exactly P pairs, with a mask too (the fixed pose sees nothing): the edges (0, 1),
    (0, K-1) and (K-2, K-1), one edge on 3 000 points, the rest with both poses drawn over all of [0, K).  The long edge is
    put where 1 500 pairs of a smaller key and a sort tile's worth in all lie in front of its last pair, if there are that
    many others: its run then crosses the first tile boundary of the sorted order.  -> (case, facts)."""
    if ("pairkeys", name) not in _cache:
        K, P = pair_key_sizes()[name]
        T = limits()["sort_tile"]
        rng = np.random.default_rng(2000 + K % 1000 + P)
        other = np.sort(_distinct_rows(rng, K, P - LONG_RUN, 2), 1)
        other[:3] = (0, 1), (0, K - 1), (K - 2, K - 1)
        key = np.sort(other[:, 0] * K + other[:, 1])
        r = min(T - LONG_RUN // 2, len(key) // 2)                      # pairs in front of the long edge's run
        while key[r] // K - key[r - 1] // K < 2:                        # a first pose between two neighbours: no edge twice
            r += 1
        a = int(key[r - 1] // K) + 1
        rows = np.concatenate([other, np.tile((a, a + 1), (LONG_RUN, 1))])
        rows = rows[rng.permutation(P)]                                 # the long edge's points lie anywhere in [0, P)
        fixed = np.zeros(K, bool)
        fixed[np.setdiff1d(np.arange(min(K, 4 * P)), rows)[-1]] = True  # a pose that no track names
        op, ol, _ = _shuffled(rng, rows.reshape(-1), np.repeat(np.arange(P), 2))
        _cache["pairkeys", name] = (K, P, op, ol, fixed), dict(long_edge=(a, a + 1), first=r, crosses=r < T < r + LONG_RUN)
    return _cache["pairkeys", name]


# ---- 3. a hub of n poses: a list of thousands, and as many pairs as the head scan needs for a third level -------------------------
def hub_size():
    """The largest n with n (n - 1) / 2 < scan_tile^2 - 1."""
    S = limits()["scan_tile"] ** 2
    n = int(np.sqrt(2.0 * S))
    while n * (n - 1) // 2 < S - 1:
        n += 1
    while n * (n - 1) // 2 >= S - 1:
        n -= 1
    return n


def hub_case(n, extra, seed, hub_point=None):
    """K = n + 1 poses; pose 0 is fixed and sees nothing; poses 1 .. n all see one point (the hub), and ``extra`` more points are
    seen by two of those poses each (the first two by the same pair; none by (n-1, n)), so P = n (n - 1) / 2 + extra, every
    pair of poses is an edge and E < P.  The hub is point ``hub_point`` (the middle one if None).

    -> (case, expected): the five tables stated from the construction.  The edges are all (i, j), 1 <= i < j <= n, in
    lexicographic order: edge (i, j) is slot (j - i - 1) of row i - 1 of the strict upper triangle.  Its weight is 1 plus the
    extra points on it; its pairs ascend in the point, the hub's among them, and name where the shuffle put the observations."""
    rng = np.random.default_rng(seed)
    h = extra // 2 if hub_point is None else int(hub_point)
    K, L = n + 1, extra + 1
    ex = 1 + np.sort(_distinct_rows(rng, n, extra, 2), 1)
    if extra > 1:
        ex[1] = ex[0]
    while True:
        last = (ex[:, 0] == n - 1) & (ex[:, 1] == n)
        if not last.any():
            break
        ex[last] = 1 + np.sort(_distinct_rows(rng, n, int(last.sum()), 2), 1)
    ex_point = np.delete(np.arange(L), h)[rng.permutation(extra)]
    op, ol, perm = _shuffled(rng, np.r_[np.arange(1, n + 1), ex.reshape(-1)], np.r_[np.full(n, h), np.repeat(ex_point, 2)])
    at = np.empty(len(perm), np.int64)
    at[perm] = np.arange(len(perm))                                     # where the shuffle put each observation
    at_hub, at_a, at_b = at[:n], at[n::2], at[n + 1::2]
    fixed = np.zeros(K, bool)
    fixed[0] = True

    i, j = np.triu_indices(n, 1)                                        # rows in order: (i + 1, j + 1) ascends lexicographically
    E, P = len(i), len(i) + extra
    xi, xj = ex[:, 0] - 1, ex[:, 1] - 1
    ex_edge = xi * (2 * n - xi - 1) // 2 + xj - xi - 1
    weights = 1 + np.bincount(ex_edge, minlength=E)
    ptr = np.r_[0, np.cumsum(weights)]
    order = np.lexsort((ex_point, ex_edge))                             # the extra pairs by (edge, point)
    es, ps = ex_edge[order], ex_point[order]
    slot_ex = ptr[es] + np.arange(extra) - np.searchsorted(es, es) + (ps > h)      # behind the hub's pair if the point is
    slot_hub = ptr[:-1] + np.bincount(ex_edge[ex_point < h], minlength=E)
    pa, pb = np.empty(P, np.int32), np.empty(P, np.int32)
    pa[slot_hub], pb[slot_hub] = at_hub[i], at_hub[j]
    pa[slot_ex], pb[slot_ex] = at_a[order], at_b[order]
    tables = (np.stack([i + 1, j + 1], 1).astype(np.int32), weights.astype(np.int32), ptr.astype(np.int32), pa, pb)
    return (K, L, op, ol, fixed), tables


def hub_pairs_sizes():
    """Pair counts around scan_tile^2 (the head scan takes a third level just past it), and one a tile further, where the
    third level's sums reach more than one entry."""
    S, tile = limits()["scan_tile"] ** 2, limits()["scan_tile"]
    return (S - 1, S, S + 1, S + tile + 1)


# ---- 3. L + 1 scan entries around scan_tile^2 --------------------------------------------------------------------------------------
POINT_TRACKS = 3000


def points_sizes():
    """L with L + 1 = scan_tile^2 and one more (the pair scan takes a third level), and L a tile and a bit further, where the
    entries of more than one tile hang on the third level."""
    S, tile = limits()["scan_tile"] ** 2, limits()["scan_tile"]
    return (S - 1, S, S + tile + 2)


def points_case(L):
    """K = 5, pose 2 fixed; 3 000 observed points over [0, L), every other point unobserved: point 0, point L - 1, the points
    around every scan tile boundary past scan_tile^2 that L leaves room for, the rest anywhere."""
    if ("points", L) not in _cache:
        S, tile = limits()["scan_tile"] ** 2, limits()["scan_tile"]
        rng = np.random.default_rng(3000 + L % 1000)
        named = sorted({p for p in (0, L - 1, S - 1, S, S + 1, S + tile - 1, S + tile) if 0 <= p < L})
        points = np.union1d(named, rng.choice(L, POINT_TRACKS, replace=False))
        tracks = C.random_tracks(rng, 5, len(points), 1, 3)
        where = {int(p): t for t, p in enumerate(points)}
        for p in named:
            tracks[where[p]] = (0, 1, 3) if p % 2 == 0 else (1, 3, 4)    # two free observers at least: pairs at both ends
        op, ol, _ = _shuffled(rng, np.array([k for t in tracks for k in t]), np.repeat(points, [len(t) for t in tracks]))
        fixed = np.zeros(5, bool)
        fixed[2] = True
        _cache["points", L] = (5, int(L), op, ol, fixed)
    return _cache["points", L]


# ---- 4. a large map for CovisibilityTables.from_observations -----------------------------------------------------------------------
MAP_POINTS, MAP_EMPTY_ENDS, MAP_FRAMES = 200000, 70000, 64


def large_map(seed=51):
    """(K, offsets, obs): 200 000 map points over 64 frames; the first and the last 70 000 have no observation, the 60 000
    between have 0 to 6 (the first and the last of them 3 and 2), frames strictly ascending, rows inside the frames arbitrary."""
    if "map" not in _cache:
        rng = np.random.default_rng(seed)
        n = MAP_POINTS - 2 * MAP_EMPTY_ENDS
        counts = rng.integers(0, 7, n)
        counts[0], counts[-1] = 3, 2
        frames = rng.permuted(np.tile(np.arange(MAP_FRAMES), (n, 1)), axis=1)[:, :6]
        frames[np.arange(6)[None, :] >= counts[:, None]] = MAP_FRAMES
        frames = np.sort(frames, 1)[np.arange(6)[None, :] < counts[:, None]]          # the first counts[m] of row m, ascending
        offsets = np.zeros(MAP_POINTS + 1, np.int64)
        offsets[MAP_EMPTY_ENDS + 1:MAP_EMPTY_ENDS + n + 1] = np.cumsum(counts)
        offsets[MAP_EMPTY_ENDS + n + 1:] = offsets[MAP_EMPTY_ENDS + n]
        obs = np.stack([frames, rng.integers(0, 2000, len(frames))], 1).astype(np.int32)
        _cache["map"] = (MAP_FRAMES, offsets, obs)
    return _cache["map"]
