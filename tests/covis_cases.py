"""Cases for the covisibility graph on the device (csrc/covis.hip), shared by tests/test_covis_cpu.py (the brute-force statement
against slamhip.covisibility) and tests/test_covis_gpu.py (the device against both).

A case is ``(K, L, obs_pose, obs_point, fixed)``: int32 observation lists in a seeded shuffled order unless its name ends in
"-sorted", and ``fixed`` a bool mask [K] or None (nothing fixed: the graph mode, which slamhip.covisibility refuses).  Sizes at
which the kernels change their path come from ``slam_covis_limits``, not from constants copied here."""
import numpy as np

_cache = {}


def limits():
    from slamhip import covis

    return covis.limits()


def from_tracks(K, tracks, fixed, seed, L=None, shuffle=True):
    """One point per track (the poses that see it; an empty track is a point nobody observes)."""
    op = np.array([k for t in tracks for k in t], np.int32)
    ol = np.array([l for l, t in enumerate(tracks) for _ in t], np.int32)
    if shuffle:
        perm = np.random.default_rng(seed).permutation(len(op))
        op, ol = op[perm], ol[perm]
    mask = None
    if fixed is not None:
        mask = np.zeros(K, bool)
        mask[list(fixed)] = True
    return int(K), int(L if L is not None else max(len(tracks), 1)), op, ol, mask


def random_tracks(rng, K, L, lo, hi, pool=None):
    pool = np.arange(K) if pool is None else np.asarray(pool)
    return [tuple(sorted(rng.choice(pool, int(rng.integers(lo, hi + 1)), replace=False).tolist())) for _ in range(L)]


def pair_tracks(rng, K, P, pool=None):
    """P points of track length 2 over K poses (or over ``pool``): exactly P pairs."""
    return random_tracks(rng, K, P, 2, 2, pool)


def _build():
    lim = limits()
    rng = np.random.default_rng(20240)
    c = {}

    def both(name, K, tracks, fixed, seed, **kw):
        """The layout with the mask and without it."""
        c[name] = from_tracks(K, tracks, fixed, seed, **kw)
        c[name + "-nomask"] = from_tracks(K, tracks, None, seed, **kw)

    # ---- empty and tiny
    both("empty", 3, [], (0,), 1)
    both("one-observation", 3, [(1,)], (0,), 2)
    both("one-pose", 1, [(0,), (0,), ()], (0,), 3)
    c["two-poses-nomask"] = from_tracks(2, [(0, 1)], None, 4)                       # E = 1, P = 1
    c["two-free-poses"] = from_tracks(3, [(1, 2)], (0,), 5)                         # the same with a mask: pose 0 holds the gauge
    both("seen-once", 9, [(int(k),) for k in rng.integers(0, 9, 40)], (0,), 6)     # E = 0, P = 0
    both("fixed-only-points", 8, [(0, 1)] * 5 + [(0,), (1,)] + [(2, 3), (3, 4, 5), (0, 2, 6), (1, 7)], (0, 1), 7)
    both("fixed-in-the-middle", 12, random_tracks(rng, 12, 60, 1, 5), (4, 5, 9), 8)
    both("all-but-one-fixed", 6, random_tracks(rng, 6, 30, 1, 4), (0, 1, 2, 4, 5), 9)
    both("gaps", 7, [t if i % 3 == 0 else () for i, t in enumerate(random_tracks(rng, 7, 90, 2, 4))], (0,), 10, L=120)
    c["gaps-sorted"] = from_tracks(7, [t if i % 3 == 0 else () for i, t in enumerate(random_tracks(rng, 7, 90, 2, 4))], (0,), 10, L=120, shuffle=False)

    # ---- long lists: longer than a wave, than a workgroup, than both with company
    both("hub300", 300, [tuple(range(300))], (0,), 11)
    both("hub300-among-2000", 300, pair_tracks(rng, 300, 1000) + [tuple(range(300))] + pair_tracks(rng, 300, 1000), (7,), 12)
    for n in sorted({lim["ballot_lanes"], lim["threads"]}):                          # list lengths around a wave and a workgroup
        K = n + 3
        tracks = [tuple(range(1, m + 1)) for m in (n - 1, n, n + 1)] + random_tracks(rng, K, 20, 1, 3)
        both(f"lists-around-{n}", K, tracks, (0,), 13 + n)
    for n in sorted({lim["sort_tile"], lim["scan_tile"]}):                           # pair counts around a sort tile and a scan tile
        for P in (n - 1, n, n + 1):
            both(f"pairs-{P}", 6, pair_tracks(rng, 6, P, pool=np.arange(1, 6)), (0,), 14 + P)     # pose 0 sees nothing: P pairs with the mask too
    for L in (lim["scan_tile"] - 2, lim["scan_tile"] - 1, lim["scan_tile"]):         # L + 1 scan entries around a scan tile
        both(f"points-{L}", 5, random_tracks(rng, 5, L, 1, 3), (2,), 15 + L)
    O = lim["sort_tile"]
    for extra in (-1, 0, 1):                                                          # observations around a sort tile
        tracks = pair_tracks(rng, 9, O // 2 - 1) + [(3,), (4,) if extra >= 0 else (), (5,) if extra > 0 else ()]
        both(f"observations-{O + extra}", 9, tracks, (8,), 16 + extra)

    # ---- key widths: the bits of K^2 - 1 at, under and over a digit boundary; 64-bit keys
    for K in (16, 17, 255, 256, 257):
        tracks = random_tracks(rng, K, 150, 1, 4) + [(K - 2, K - 1), (0, K - 1), (1, 2)]
        both(f"K{K}", K, tracks, (0,), 17 + K)
    for K in (65536, 70000):
        both(f"K{K}", K, random_tracks(rng, K, 40, 3, 3, pool=np.arange(K - 1000, K)), (0,), 18 + K)

    # ---- long edges
    both("long-edge", 52, [(50, 51)] * 5000 + random_tracks(rng, 50, 300, 1, 4), (0,), 19)
    both("configs4-scaled", 40, random_tracks(rng, 40, 1500, 12, 12), (0,), 20)
    return c


def cases():
    """{name: (K, L, obs_pose, obs_point, fixed)}, built once."""
    if "cases" not in _cache:
        _cache["cases"] = _build()
    return _cache["cases"]


def names(masked):
    return sorted(n for n, c in cases().items() if (c[4] is not None) == masked)


def permuted(case, seed):
    """The same problem with its observation list in another order -> (case, perm): new[i] = old[perm[i]]."""
    K, L, op, ol, fixed = case
    perm = np.random.default_rng(seed).permutation(len(op))
    return (K, L, op[perm], ol[perm], fixed), perm


def with_duplicate(case, at, gap):
    """The case with the observation at index ``at`` repeated ``gap`` entries later."""
    K, L, op, ol, fixed = case
    j = at + gap
    return K, L, np.insert(op, j, op[at]), np.insert(ol, j, ol[at]), fixed


def refusal_base(seed=31):
    """K = 20, pose 0 fixed, 4 000 points of 2 to 4 observers: more than 10^4 observations."""
    rng = np.random.default_rng(seed)
    return from_tracks(20, random_tracks(rng, 20, 4000, 2, 4), (0,), seed)


def map_observations(seed=41):
    """(K, lists) for MapObservations.from_lists: 300 points over 60 frames, tracks of 0 to 9 ascending frames and one of all 60,
    rows inside the frames arbitrary."""
    rng = np.random.default_rng(seed)
    K = 60
    tracks = random_tracks(rng, K, 300, 0, 9) + [tuple(range(K))]
    return K, [[(k, int(rng.integers(0, 2000))) for k in t] for t in tracks]
