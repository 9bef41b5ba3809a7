"""GPU: the pipelined whole-stage trip of the 32x32x64 matrix-core top-2 search (bf_mx32.hip, engine 3) against the VALU kernel
(engine 1), tables bit for bit and the merge state idle after every search, at the places where a DEFERRED fold can go wrong:
tile 1 of a wave (queries with (q & 63) >= 32) is folded a group late, behind tile 0's four MFMAs of the next group, and
tile 1 of a stage's last group is folded bare in front of the stage end.

Every planted pair is given to a tile-0 query AND to a tile-1 query that carries the same descriptor (with N = 33 only query 32
is in tile 1: it mirrors one of the planted tile-0 queries, another one in every search).  Pairs are planted in the last group of
a stage, in the first group of the next, across the boundary, at chunk boundaries for one worker and for many, in the last
whole group and the ragged tail of a short last stage; as nearest-below, nearest-above and as a tie that the lower row wins."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ONE_WORKER_N = 513 * 256       # more query blocks than 4 x 256 CUs hold: one worker per query block
STAGE, GROUP = 128, 32
VARIANTS = {"near_low": (3, 5), "near_high": (5, 3), "tie": (4, 4)}      # distances of the (lower row, higher row)


def _search(ctx, q, t, engine):
    import slamhip

    ctx.set_engine(engine)
    dq, dt = slamhip.DeviceDescriptors(ctx, q), slamhip.DeviceDescriptors(ctx, t)
    tab = slamhip.Top2Table(ctx, len(q))
    try:
        slamhip.knn2_device(ctx, dq.buf, len(q), dt.buf, len(t), tab.idx, tab.dist)
        out = tab.download()
    finally:
        ctx.set_engine(0)
        for o in (tab, dq, dt):
            o.free()
    assert ctx.state_dirty() == 0, "the search left its merge state dirty"
    return out


def _agree(ctx, q, t, what=""):
    a = _search(ctx, q, t, 1)
    b = _search(ctx, q, t, 3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), what
    return b


def _at(rng, row, d):
    """A descriptor at Hamming distance d from ``row``."""
    bits = np.unpackbits(row)
    bits[rng.permutation(256)[:d]] ^= 1
    return np.packbits(bits)


def _tiles(n):
    j = np.arange(n)
    return j[(j & 63) < 32].tolist(), j[(j & 63) >= 32].tolist()


def _plan(ctx, n, m):
    import slamhip

    plan, tbl = slamhip.mx_plan_describe(n, m, num_cu=ctx.plan_info(n, m)["cus"])
    assert plan["stage_rows"] == STAGE and plan["workers"] >= 1 and tbl[0] == 0 and tbl[-1] == m and list(tbl) == sorted(tbl)
    return plan, tbl


def _plant_and_check(ctx, rng, n, m, pairs, variant, turn=0):
    """pairs: [(lower row, higher row)], disjoint.  Each pair goes to a tile-0 query and to a tile-1 query with the same descriptor."""
    d_lo, d_hi = VARIANTS[variant]
    used, kept = set(), []
    for p in pairs:                                              # a row holds one planted descriptor
        if not used & set(p):
            kept.append(p)
            used |= set(p)
    pairs = kept
    q = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    t0, t1 = _tiles(n)
    assert len(pairs) <= len(t0) and t1
    want = {}
    for i, (lo, hi) in enumerate(pairs):
        assert 0 <= lo < hi < m
        j0 = t0[i]
        t[lo], t[hi] = _at(rng, q[j0], d_lo), _at(rng, q[j0], d_hi)
        rows, ds = ([lo, hi], [d_lo, d_hi]) if d_lo <= d_hi else ([hi, lo], [d_hi, d_lo])
        want[j0] = (rows, ds)
        if len(t1) >= len(pairs):
            j1 = t1[-1 - i]
        elif i == turn % len(pairs):
            j1 = t1[0]
        else:
            continue
        q[j1] = q[j0]
        want[j1] = (rows, ds)
    assert len(want) >= len(pairs) + 1
    idx, dist = _agree(ctx, q, t, (n, m, variant))
    for j, (rows, ds) in want.items():
        assert idx[j].tolist() == rows and dist[j].tolist() == ds, (n, m, variant, j, idx[j], dist[j])


def _boundaries(m):
    """Stage starts, the start of the last (possibly ragged) group and of the whole group in front of it, and the end."""
    last = (m - 1) // GROUP * GROUP
    return sorted({b for b in list(range(STAGE, m, STAGE)) + [last, last - GROUP] if 0 < b < m} | {m})


@pytest.mark.parametrize("n", [33, 64, 65, 300])
@pytest.mark.parametrize("m", [96, 127, 128, 129, 160, 287, 1024 + 33])
def test_pairs_around_group_and_stage_boundaries_of_a_short_train_set(gpu_ctx, n, m):
    _plan(gpu_ctx, n, m)
    rng = np.random.default_rng(1000 * m + n)
    inside = [p for b in _boundaries(m) for p in ((b - 2, b - 1), (b, b + 1)) if 0 <= p[0] and p[1] < m]    # last group | first of next
    across = [(b - 1, b) for b in _boundaries(m) if b < m]
    turn = 0
    for variant in VARIANTS:
        for pairs in (inside, across):
            _plant_and_check(gpu_ctx, rng, n, m, pairs, variant, turn)
            turn += 1


@pytest.mark.parametrize("n,m", [(300, 16384 + 77), (ONE_WORKER_N, 4000)], ids=["many_workers", "one_worker"])
def test_pairs_around_chunk_boundaries(gpu_ctx, n, m):
    plan, tbl = _plan(gpu_ctx, n, m)
    assert plan["workers"] == 1 if n == ONE_WORKER_N else plan["workers"] > 8
    k = len(tbl) // 2
    cuts = [tbl[k + i] for i in range(4)]
    assert cuts[0] > 1024 and cuts[-1] < m - 2 and min(np.diff(cuts)) >= 4
    rng = np.random.default_rng(n + m)
    for variant in VARIANTS:
        _plant_and_check(gpu_ctx, rng, n, m, [p for b in cuts for p in ((b - 2, b - 1), (b, b + 1))], variant)
        _plant_and_check(gpu_ctx, rng, n, m, [(b - 1, b) for b in cuts], variant)


@pytest.mark.parametrize("shift", [0, GROUP], ids=["inside_a_stage", "across_a_stage"])
def test_threshold_falls_in_a_group_for_tile_0_while_tile_1_still_folds_it(gpu_ctx, shift):
    """Group g brings the 2nd-best distance down to 12; group g + 1 holds a row at 11 (passes the new threshold), at 12 (a tie
    from a higher row: loses) and rows at 13 .. 38 that pass only the threshold from before group g.  The same descriptor sits
    in tile 0 (query 5) and in tile 1 (query 37): when tile 1 folds group g, tile 0 has folded it and has MFMAs of g + 1 in
    flight.  g = 2, g + 1 = 3 of stage 0, and shifted by a group: g = 3, g + 1 = group 0 of stage 1."""
    n, m = 64, 384
    plan, _ = _plan(gpu_ctx, n, m)
    rng = np.random.default_rng(96 + shift)
    q = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    q[37] = q[5]
    s = shift
    t[70 + s], t[83 + s] = _at(rng, q[5], 10), _at(rng, q[5], 12)
    t[96 + s], t[97 + s], t[101 + s] = _at(rng, q[5], 12), _at(rng, q[5], 13), _at(rng, q[5], 11)
    for r in range(102, 128):
        t[r + s] = _at(rng, q[5], 13 + (r - 102))
    idx, dist = _agree(gpu_ctx, q, t)
    for j in (5, 37):
        assert idx[j].tolist() == [70 + s, 101 + s] and dist[j].tolist() == [10, 11], j
    t[101 + s] = _at(rng, q[5], 12)                               # now the tie at the lower row keeps the second place
    idx, dist = _agree(gpu_ctx, q, t)
    for j in (5, 37):
        assert idx[j].tolist() == [70 + s, 83 + s] and dist[j].tolist() == [10, 12], j


def test_a_stage_in_which_only_tile_1_of_the_last_group_fires(gpu_ctx):
    """One worker per query block, chunks of two stages.  Every query is the descriptor v but queries 32 .. 63 (tile 1 of wave 0
    of block 0), which are w.  Rows 0 .. 3 bring every threshold down in the first group (v: distances 0 and 1, w: 2 and 3),
    every other row is random, so every later group is quiet - but two, each the LAST group of a stage that another stage of the
    chunk follows, where only tile 1 of that wave fires, in the fold that runs bare in front of the stage end: row 105 (w at
    distance 1; stage 0, whose end is an early exchange) and the same place in the first stage of a later chunk (w itself)."""
    n, m = ONE_WORKER_N, 4000
    plan, tbl = _plan(gpu_ctx, n, m)
    assert plan["workers"] == 1
    k = next(i for i in range(len(tbl) - 1) if tbl[i] >= 512 and tbl[i + 1] - tbl[i] == 2 * STAGE)
    row = tbl[k] + 3 * GROUP + 9                                   # the last group of the chunk's first stage
    assert tbl[1] == 2 * STAGE
    rng = np.random.default_rng(4000)
    v, w = rng.integers(0, 256, 32, dtype=np.uint8), rng.integers(0, 256, 32, dtype=np.uint8)
    q = np.tile(v, (n, 1))
    q[32:64] = w
    t = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    t[0], t[1], t[2], t[3] = v, _at(rng, v, 1), _at(rng, w, 2), _at(rng, w, 3)
    t[row] = w
    idx, dist = _agree(gpu_ctx, q, t)
    assert (idx[32:64] == [row, 2]).all() and (dist[32:64] == [0, 2]).all()
    assert (idx[:32] == [0, 1]).all() and (idx[64:] == [0, 1]).all()
    t[3 * GROUP + 9] = _at(rng, w, 1)
    idx, dist = _agree(gpu_ctx, q, t)
    assert (idx[32:64] == [row, 3 * GROUP + 9]).all() and (dist[32:64] == [0, 1]).all()
    assert (idx[:32] == [0, 1]).all() and (idx[64:] == [0, 1]).all()
