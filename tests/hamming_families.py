"""Descriptor families whose Hamming distances are known by construction, and the expected results of the top-k, radius and
window searches on them from integer arithmetic alone (a helper module of the search-edge suites, like two_view_ref.py).

Row i of ``prefix_rows(a)`` has its first ``a[i]`` bits set, so queries ``prefix_rows(b)`` against trains ``prefix_rows(a)``
sit at distance exactly ``|a[i] - b[j]|``: every expectation below is a sort of those integers by (distance, train index),
independent of the C oracle, of numpy popcounts and of the code under test.  Random 256-bit rows are 128 +- 8 bits apart;
these families reach distance 0 and 256, mass ties at every level of a list, lists of a chosen length and train sets that
make every row (or no row) enter a list.

The two brute-force references of the radius and window suites (``ref_radius``, ``ref_window``) live here too, so that the
CPU suite can tie them to the integer expectations."""
import numpy as np

from oracle import oracle

NONE_IDX, NONE_DIST = -1, np.iinfo(np.int32).max
BITS = 256


# ---- descriptors ---------------------------------------------------------------------------------------------------------

def prefix_rows(a):
    """uint8 [len(a), 32]: row i has its first a[i] bits set (0 <= a[i] <= 256)."""
    a = np.asarray(a, np.int64).reshape(-1)
    assert a.size == 0 or (0 <= a.min() and a.max() <= BITS), "a prefix length lies in [0, 256]"
    bits = (np.arange(BITS)[None, :] < a[:, None]).astype(np.uint8)
    return np.ascontiguousarray(np.packbits(bits, axis=1).reshape(a.size, 32))


def distances(a, b):
    """int64 [len(b), len(a)]: |a[i] - b[j]|, the distance of query j to train row i."""
    return np.abs(np.asarray(a, np.int64)[None, :] - np.asarray(b, np.int64)[:, None])


# ---- expectations ----------------------------------------------------------------------------------------------------------

def _ordered(a, b, allowed=None):
    """Per DISTINCT query value: the train rows in (distance, index) order, the count of allowed rows, and the map back."""
    a, b = np.asarray(a, np.int64).reshape(-1), np.asarray(b, np.int64).reshape(-1)
    ub, inv = np.unique(b, return_inverse=True)
    d = distances(a, ub)
    if allowed is not None:
        d = np.where(np.asarray(allowed, bool)[None, :], d, BITS + 1)          # behind every real distance
    order = np.argsort(d, axis=1, kind="stable")                              # stable: ties keep ascending index
    return d, order, inv


def expected_topk(a, b, k):
    """(idx, dist) int32 [len(b), k] of the k nearest train rows, (distance, index) order, fillers (-1, INT_MAX)."""
    return expected_window(a, b, None, k)


def expected_window(a, b, in_window, k):
    """``expected_topk`` over the train rows with ``in_window[i]`` true (bool [len(a)], the same for every query; None: all)."""
    d, order, inv = _ordered(a, b, in_window)
    m = d.shape[1]
    idx = np.full((d.shape[0], k), NONE_IDX, np.int32)
    dist = np.full((d.shape[0], k), NONE_DIST, np.int32)
    kk = min(k, m)
    top = order[:, :kk]
    dd = np.take_along_axis(d, top, axis=1)
    ok = dd <= BITS
    idx[:, :kk] = np.where(ok, top, NONE_IDX)
    dist[:, :kk] = np.where(ok, dd, NONE_DIST)
    return np.ascontiguousarray(idx[inv]), np.ascontiguousarray(dist[inv])


def expected_radius(a, b, th):
    """(offsets int64 [len(b) + 1], idx int32 [T], dist int32 [T]): every train row with distance < th per query, each list
    in (distance, index) order."""
    d, order, inv = _ordered(a, b)
    ds = np.take_along_axis(d, order, axis=1)
    cnt = (ds < th).sum(1)
    off = np.zeros(inv.size + 1, np.int64)
    np.cumsum(cnt[inv], out=off[1:])
    idx = np.empty(off[-1], np.int32)
    dist = np.empty(off[-1], np.int32)
    for j, u in enumerate(inv):
        idx[off[j]:off[j + 1]] = order[u, :cnt[u]]
        dist[off[j]:off[j + 1]] = ds[u, :cnt[u]]
    return off, idx, dist


# ---- generators of the train multiset a ------------------------------------------------------------------------------------

def constant(m, v):
    return np.full(m, v, np.int64)


def ladder(m, kind):
    """a[i] = i mod 257 ("asc"), its reverse 256 - i mod 257 ("desc"), or a fixed permutation of each run of 257 ("perm")."""
    i = np.arange(m, dtype=np.int64)
    if kind == "asc":
        return i % 257
    if kind == "desc":
        return 256 - i % 257
    if kind == "perm":
        return (i * 100 + 31) % 257                                            # 257 is prime: a bijection on every run
    raise ValueError(kind)


def straddle(boundary, count):
    """``count`` consecutive rows with half of them on each side of row ``boundary`` (clipped at row 0)."""
    start = max(0, boundary - count // 2)
    return np.arange(start, start + count)


def plateau(m, k, D, count, positions, b0=0):
    """A train set for queries of value b0 in {0, 256}: ``count`` rows at distance D at ``positions[1]``, the rows at
    ``positions[0]`` (fewer than k of them; none when D = 0) closer than D, every other row farther - or, for D = 256 where
    nothing is farther, at D as well (the plateau then holds every other row)."""
    closer, at = np.asarray(positions[0], np.int64), np.asarray(positions[1], np.int64)
    assert at.size == count and closer.size < k and (D > 0 or closer.size == 0)
    assert np.intersect1d(closer, at).size == 0 and at.max() < m and (closer.size == 0 or closer.max() < m)
    i = np.arange(m, dtype=np.int64)
    dist = np.full(m, D, np.int64) if D == BITS else D + 1 + i % (BITS - D)    # farther rows: every value above D
    dist[at] = D
    if closer.size:
        dist[closer] = np.arange(closer.size) % D                              # 0 .. D-1: ties among the closer rows too
    return dist if b0 == 0 else BITS - dist


def alphabet(m, values, rng):
    """m rows drawn from a few values: every level of every list is a mass tie."""
    return rng.choice(np.asarray(values, np.int64), m)


def lengths(b, L):
    """A train set on which radius 0 gives query j exactly L[j] rows (a == b[j]); queries that share a value share a length.
    The rows of every value are spread evenly along the train index, so every chunk contributes to every longer list."""
    b, L = np.asarray(b, np.int64), np.asarray(L, np.int64)
    vals, pos = [], []
    for v in np.unique(b):
        c = np.unique(L[b == v])
        assert c.size == 1, "queries of one value share their list"
        vals.append(np.full(c[0], v, np.int64))
        pos.append((np.arange(c[0]) + 0.5) / max(c[0], 1))
    vals, pos = np.concatenate(vals), np.concatenate(pos)
    return vals[np.argsort(pos, kind="stable")]


# ---- query sets ------------------------------------------------------------------------------------------------------------

def queries_alternating(n):
    """0 and 256 by lane: on a descending ladder the even lanes insert every row while the odd lanes reject every row."""
    return np.where(np.arange(n) % 2 == 0, 0, BITS).astype(np.int64)


def queries_equal(n, v=0):
    return np.full(n, v, np.int64)


def queries_ramp(n):
    return np.arange(n, dtype=np.int64) % 257


# ---- the brute-force references of the radius and window suites --------------------------------------------------------

def ref_radius(q, t, radii, step=16384):
    """{radius: (offsets, idx, dist)} by brute force over the full distance matrix, in chunks of train rows."""
    from slamhip import radius_threshold

    ths = {r: radius_threshold(r) for r in radii}
    parts = {r: [] for r in radii}
    for a in range(0, t.shape[0], step):
        d = oracle.hamming_matrix_np(q, t[a:a + step])
        for r, th in ths.items():
            qi, ti = np.nonzero(d < th)
            parts[r].append((qi.astype(np.int64), (ti + a).astype(np.int32), d[qi, ti].astype(np.int32)))
    out = {}
    for r in radii:
        qi = np.concatenate([p[0] for p in parts[r]]) if parts[r] else np.zeros(0, np.int64)
        ti = np.concatenate([p[1] for p in parts[r]]) if parts[r] else np.zeros(0, np.int32)
        di = np.concatenate([p[2] for p in parts[r]]) if parts[r] else np.zeros(0, np.int32)
        order = np.lexsort((ti, di, qi))
        off = np.zeros(q.shape[0] + 1, np.int64)
        np.cumsum(np.bincount(qi, minlength=q.shape[0]), out=off[1:])
        out[r] = (off, ti[order], di[order])
    return out


def ref_window(q, t, qxy, txy, radius, k, rows=None):
    """(idx, dist) int32 [len(rows), k] of the k nearest in-window train rows of each query row, by definition."""
    n, m = q.shape[0], t.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    qxy, txy = np.asarray(qxy, np.float32).reshape(-1, 2), np.asarray(txy, np.float32).reshape(-1, 2)
    r = np.broadcast_to(np.asarray(radius, np.float32), (m,))
    idx = np.full((rows.size, k), NONE_IDX, np.int32)
    dist = np.full((rows.size, k), NONE_DIST, np.int32)
    if m == 0:
        return idx, dist
    step = max(1, (1 << 22) // m)
    for a in range(0, rows.size, step):
        rr = rows[a:a + step]
        with np.errstate(invalid="ignore"):
            w = ((np.abs(qxy[rr, 0][:, None] - txy[None, :, 0]) <= r[None, :])
                 & (np.abs(qxy[rr, 1][:, None] - txy[None, :, 1]) <= r[None, :]))
        cols = np.flatnonzero(w.any(0))
        if cols.size == 0:
            continue
        d = oracle.hamming_matrix_np(q[rr], t[cols]).astype(np.int64)
        key = np.where(w[:, cols], (d << 23) | cols[None, :], np.int64(1) << 40)
        top = np.sort(key, axis=1, kind="stable")[:, :k]
        ok = top < (np.int64(1) << 40)
        kk = top.shape[1]
        idx[a:a + rr.size, :kk] = np.where(ok, top & ((1 << 23) - 1), NONE_IDX)
        dist[a:a + rr.size, :kk] = np.where(ok, top >> 23, NONE_DIST)
    return idx, dist


# ---- the shapes and cases of tests/test_search_edges_gpu.py (test_search_edges_cpu.py checks the regime each one aims at) ----

TOPK_N = (1, 63, 64, 65, 255, 256, 257)
TOPK_M_SINGLE = (1, 15, 16, 17, 255, 256)        # one chunk: results written directly, nothing exchanged
TOPK_M_MULTI = (1029, 1039)                      # five chunks of 208 rows; the last one ends in 5 / in 15 single rows
TOPK_M = 1029                                    # the multi-chunk train set of the ladder, plateau and alphabet cases
TOPK_TILE_SHAPE = (131072, 2000)                 # so many query blocks that a chunk spans several 256-row tiles, for every k
PLATEAU_KS = (1, 2, 5, 8, 17, 32)
PLATEAU_DS = (0, 1, 128, 255, 256)
WIDE_KS = tuple(k for k in range(1, 33) if k not in (4, 8, 16, 32))      # k that runs on a wider instantiation: pad slots

RADIUS_N = 300
RADIUS_LENGTHS = {0: 0, 1: 4096, 2: 1, 3: 2, 4: 63, 254: 4095, 255: 8192, 256: 8193, 257: 64, 298: 65, 299: 4097}
RADIUS_TH = ((0.0, 1), (1.0, 2), (2.5, 3))       # (radius, the threshold d < th it stands for)
RADIUS_BIN_M = (257, 5 * 257 + 3, 17 * 257 + 3)  # each bin once (short path), five times (short), 17 times (long path)
RADIUS_BIN_TH = ((0.0, 1), (1.0, 2), (127.5, 128), (255.0, 256), (256.0, 257))
RADIUS_CONST_M = (1, 2, 64, 65, 4096, 4097)

WINDOW_M = (63, 64, 65, 1023, 1024, 1025, 2049)
WINDOW_N = (1, 63, 64, 65, 130)
WINDOW_KINDS = ("const0", "const256", "desc", "plateau3", "alphabet2", "alphabet3")


def plateau_case(m, k, D, boundary):
    """(a, (closer, at)): k + 3 rows at distance D from the value 0 with half of them on each side of row ``boundary``, and
    k - 1 closer rows (none for D = 0) - the first half of them in front of the plateau, the others at the end of the set."""
    at = straddle(boundary, k + 3)
    free = np.setdiff1d(np.arange(m), at)
    nc = k - 1 if D > 0 else 0
    closer = np.r_[free[:(nc + 1) // 2], free[free.size - nc // 2:]] if nc else np.zeros(0, np.int64)
    return plateau(m, k, D, k + 3, (closer, at)), (closer, at)


def radius_lengths_case():
    """(a, b, L): RADIUS_N queries; the lists of RADIUS_LENGTHS on their queries at radius 0, lists of 0 .. 4 rows on all
    others, every value of 0 .. 256 in use so that wider radii join neighbouring bins."""
    special = {q: 3 + 23 * s for s, q in enumerate(sorted(RADIUS_LENGTHS))}
    rest = [v for v in range(257) if v not in special.values()]
    b = np.zeros(RADIUS_N, np.int64)
    L = np.zeros(RADIUS_N, np.int64)
    j = 0
    for q in range(RADIUS_N):
        if q in special:
            b[q], L[q] = special[q], RADIUS_LENGTHS[q]
        else:
            b[q] = rest[j % len(rest)]
            L[q] = b[q] % 5
            j += 1
    return lengths(b, L), b, L


def window_case(kind, n, m):
    """(a, b) of one window case: the train values and the query values."""
    rng = np.random.default_rng(1000 * m + n)
    if kind == "const0":
        return constant(m, 0), queries_equal(n)
    if kind == "const256":
        return constant(m, 256), queries_equal(n)
    if kind == "desc":
        return ladder(m, "desc"), queries_alternating(n)
    if kind == "plateau3":                                          # best row in the middle, three second-best rows far apart
        a = 200 + np.arange(m, dtype=np.int64) % 57
        a[[1, m // 2 + 1, m - 1]] = 5
        a[m // 3] = 0
        return a, queries_equal(n)
    if kind == "alphabet2":
        return alphabet(m, (7, 250), rng), queries_ramp(n)
    if kind == "alphabet3":
        return alphabet(m, (0, 128, 256), rng), queries_ramp(n)
    raise ValueError(kind)
