"""GPU: the stage tail of the matrix-core top-2 searches - bf_mx32.hip (engine 3) and bf_mx.hip (engine 2) against the VALU kernel
(engine 1), tables bit for bit, the merge state idle after every search, every matrix-core search run twice on one context.

Since the per-stage union of a query's lanes is gone, a stage ends with every lane's threshold at its OWN 2nd-best: what the
other lanes of the query found in the stage reaches a lane only at the next exchange.  The cases put the nearest and the second
nearest row where that matters: in rows 96 .. 127 of a stage (the last group of the 32x32 trip, whose tile 1 folds bare in front
of the stage end) and rows 0 .. 31 of the next, for a tile-0 and a tile-1 query with the same descriptor, as nearest-below,
nearest-above and exact tie; in the early-exchange stages of a worker, in a middle stage of an eight-stage chunk, at a chunk's
last stage and in the ragged tail; with equal distances in both lanes (32x32) and all four lanes (16x16) of a query."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ONE_WORKER_N = 513 * 256       # more query blocks than 4 x 256 CUs hold: one worker per query block
LONG_M = 10000 + 57            # one worker: eight-stage chunks up to row 8192, then shrinking ones and a ragged tail
STAGE, GROUP = 128, 32
VARIANTS = {"near_low": (3, 5), "near_high": (5, 3), "tie": (4, 4)}      # distances of the (lower row, higher row)


def _search(ctx, q, t, engine):
    import slamhip

    ctx.set_engine(engine)
    dq, dt = slamhip.DeviceDescriptors(ctx, q), slamhip.DeviceDescriptors(ctx, t)
    tab = slamhip.Top2Table(ctx, len(q))
    try:
        out = []
        for _ in range(1 if engine == 1 else 2):
            slamhip.knn2_device(ctx, dq.buf, len(q), dt.buf, len(t), tab.idx, tab.dist)
            out.append(tab.download())
            assert ctx.state_dirty() == 0, "the search left its merge state dirty"
    finally:
        ctx.set_engine(0)
        for o in (tab, dq, dt):
            o.free()
    for o in out[1:]:
        assert np.array_equal(o[0], out[0][0]) and np.array_equal(o[1], out[0][1]), ("second run differs", engine)
    return out[0]


def _agree(ctx, q, t, what=""):
    a = _search(ctx, q, t, 1)
    for engine in (3, 2):
        b = _search(ctx, q, t, engine)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (what, engine)
    return a


def _at(rng, row, d):
    """A descriptor at Hamming distance d from ``row``."""
    bits = np.unpackbits(row)
    bits[rng.permutation(256)[:d]] ^= 1
    return np.packbits(bits)


def _plan(ctx, n, m):
    import slamhip

    plan, tbl = slamhip.mx_plan_describe(n, m, num_cu=ctx.plan_info(n, m)["cus"])
    assert plan["stage_rows"] == STAGE and plan["workers"] >= 1 and tbl[0] == 0 and tbl[-1] == m and list(tbl) == sorted(tbl)
    return plan, list(tbl)


def _plant_and_check(ctx, rng, q, t, pairs, variant, turn=0):
    """pairs: [(lower row, higher row)].  Each disjoint pair goes to a tile-0 query (q & 63 < 32) and to a tile-1 query with
    the same descriptor (where tile-1 queries are scarce, to one pair, another one every turn)."""
    q, t = q.copy(), t.copy()
    n, m = len(q), len(t)
    d_lo, d_hi = VARIANTS[variant]
    used, kept = set(), []
    for p in pairs:
        if not used & set(p):
            kept.append(p)
            used |= set(p)
    j = np.arange(min(n, 4096))
    t0, t1 = j[(j & 63) < 32].tolist(), j[(j & 63) >= 32].tolist()
    kept = kept[:len(t0)]
    assert kept and t1
    want = {}
    for i, (lo, hi) in enumerate(kept):
        assert 0 <= lo < hi < m
        j0 = t0[i]
        t[lo], t[hi] = _at(rng, q[j0], d_lo), _at(rng, q[j0], d_hi)
        rows, ds = ([lo, hi], [d_lo, d_hi]) if d_lo <= d_hi else ([hi, lo], [d_hi, d_lo])
        want[j0] = (rows, ds)
        if len(t1) >= len(kept):
            j1 = t1[-1 - i]
        elif i == turn % len(kept):
            j1 = t1[0]
        else:
            continue
        q[j1] = q[j0]
        want[j1] = (rows, ds)
    assert len(want) >= len(kept) + 1
    idx, dist = _agree(ctx, q, t, (n, m, variant))
    for j, (rows, ds) in want.items():
        assert idx[j].tolist() == rows and dist[j].tolist() == ds, (n, m, variant, j, idx[j], dist[j])


def _around(b, m):
    """Pairs in the last group in front of row b, in the first group behind it, and across it."""
    return [p for p in ((b - 2, b - 1), (b - GROUP, b - 3), (b, b + 1), (b + 2, b + GROUP - 1), (b - 1, b), (b - GROUP + 1, b + GROUP - 2))
            if 0 <= p[0] and p[1] < m]


@pytest.mark.parametrize("n", [33, 64, 65, 300])
@pytest.mark.parametrize("m", [127, 128, 129, 255, 256, 257, 384, 1057, 1153])
def test_pairs_in_the_last_group_of_a_stage_and_the_first_of_the_next(gpu_ctx, n, m):
    _plan(gpu_ctx, n, m)
    rng = np.random.default_rng(1000 * m + n)
    q = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    last = (m - 1) // GROUP * GROUP                                           # the ragged tail's group, and the end
    cuts = sorted({b for b in list(range(STAGE, m, STAGE)) + [last] if 0 < b < m} | {m})
    pairs = [p for b in cuts for p in _around(b, m)]
    for turn, variant in enumerate(VARIANTS):
        _plant_and_check(gpu_ctx, rng, q, t, pairs[turn % 2::2] + pairs[(turn + 1) % 2::2], variant, turn)


@pytest.fixture(scope="module")
def long_rows():
    """One worker per query block over eight-stage chunks: the rows every case of that form starts from (copied, never changed)."""
    rng = np.random.default_rng(10057)
    return rng.integers(0, 256, (ONE_WORKER_N, 32), dtype=np.uint8), rng.integers(0, 256, (LONG_M, 32), dtype=np.uint8)


def _long_plan(ctx):
    plan, tbl = _plan(ctx, ONE_WORKER_N, LONG_M)
    assert plan["workers"] == 1 and tbl[:9] == [1024 * i for i in range(9)] and tbl[-1] - tbl[-2] < STAGE
    return tbl


PLACES = {
    # the stages whose end is an early exchange (after 128, 256 and 512 scanned rows) and the one between them
    "early_exchange_stages": [128, 256, 384, 512],
    # a middle stage of an eight-stage chunk: no exchange at either end
    "middle_of_a_chunk": [3 * 1024 + 3 * STAGE, 3 * 1024 + 4 * STAGE, 5 * 1024 + 5 * STAGE],
    # the last stage of a chunk and the first of the next
    "chunk_end": [1024, 4096, 8192],
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("place", sorted(PLACES) + ["ragged_tail"])
def test_pairs_around_the_stage_ends_of_one_worker(gpu_ctx, long_rows, place, variant):
    tbl = _long_plan(gpu_ctx)
    q, t = long_rows
    if place == "ragged_tail":
        last = (LONG_M - 1) // GROUP * GROUP
        cuts = [tbl[-2], last, LONG_M]
    else:
        cuts = PLACES[place]
    rng = np.random.default_rng(len(place) + 7 * len(variant))
    _plant_and_check(gpu_ctx, rng, q, t, [p for b in cuts for p in _around(b, LONG_M)], variant)


def test_the_last_fold_of_a_stage_lowers_a_threshold_the_next_stage_depends_on(gpu_ctx, long_rows):
    """Middle of an eight-stage chunk.  The last group of stage S brings the 2nd-best distance down to 12 - in tile 1 (query 37)
    that is the fold in front of the stage end; group 0 of stage S + 1 holds a row at 11 (passes the new threshold), at 12 (a tie
    from a higher row: loses) and rows at 13 .. 38 that pass only the threshold from before.  Then with 12 for the 11: the tie
    at the lower row keeps the second place."""
    _long_plan(gpu_ctx)
    q, t = (a.copy() for a in long_rows)
    rng = np.random.default_rng(3712)
    q[37] = q[5]
    s = 3 * 1024 + 4 * STAGE                                       # the first row of stage S + 1
    t[s - 58], t[s - 13] = _at(rng, q[5], 10), _at(rng, q[5], 12)
    t[s], t[s + 1], t[s + 5] = _at(rng, q[5], 12), _at(rng, q[5], 13), _at(rng, q[5], 11)
    for r in range(6, 32):
        t[s + r] = _at(rng, q[5], 13 + (r - 6))
    idx, dist = _agree(gpu_ctx, q, t)
    for j in (5, 37):
        assert idx[j].tolist() == [s - 58, s + 5] and dist[j].tolist() == [10, 11], j
    t[s + 5] = _at(rng, q[5], 12)
    idx, dist = _agree(gpu_ctx, q, t)
    for j in (5, 37):
        assert idx[j].tolist() == [s - 58, s - 13] and dist[j].tolist() == [10, 12], j


def test_a_stage_in_which_only_tile_1_of_the_last_group_fires(gpu_ctx):
    """Every query is the descriptor v but queries 32 .. 63 (tile 1 of wave 0 of block 0), which are w.  Rows 0 .. 3 bring every
    threshold down in the first group (v: distances 0 and 1, w: 2 and 3); every other row is random, so every later group is
    quiet - but the last group of a middle stage of an eight-stage chunk, where only tile 1 of that wave fires (row at distance 0
    from w), and then also the same place of an early-exchange stage."""
    n, m = ONE_WORKER_N, LONG_M
    _long_plan(gpu_ctx)
    row = 2 * 1024 + 3 * STAGE + 3 * GROUP + 9
    rng = np.random.default_rng(4001)
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


def test_many_workers_on_few_queries(gpu_ctx):
    """N = 64, M = 16461: as many workers as chunks, each exchanging at its chunk starts while the others fold."""
    n, m = 64, 16461
    plan, tbl = _plan(gpu_ctx, n, m)
    assert plan["workers"] > 8
    rng = np.random.default_rng(16461)
    q = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    k = len(tbl) // 3
    cuts = [tbl[k], tbl[2 * k], tbl[-2]]
    for turn, variant in enumerate(VARIANTS):
        _plant_and_check(gpu_ctx, rng, q, t, [p for b in cuts for p in _around(b, m)], variant, turn)


# the rows of one stage, by offset in it, that get a candidate at ONE distance: in the 32x32 kernel rows 8 i + 4 h + j of a group of
# 32 belong to lane half h, in the 16x16 kernel rows 4 g + r of a group of 16 to lane group g
EQUAL_ROWS = {
    "lanes_ascending": [1, 5, 9, 13],               # 16x16: lane groups 0 1 2 3; 32x32: halves 0 1 0 1
    "lanes_descending": [12, 24, 36, 48 + 3],       # 16x16: lane groups 3 2 1 0; 32x32: halves 1 0 1 0
    "one_group_each": [3, 32 + 22, 64 + 9, 96 + 28],
    "last_group_only": [96 + 4, 96 + 17, 96 + 26, 96 + 31],
}


@pytest.mark.parametrize("layout", sorted(EQUAL_ROWS))
def test_equal_distances_in_every_lane_of_a_query_go_to_the_lower_rows(gpu_ctx, long_rows, layout):
    """All lanes of one query get a candidate at distance 6 in ONE stage (a middle stage of an eight-stage chunk, and an
    early-exchange stage), for a tile-0 and a tile-1 query; the next stage holds one more at the same distance.  No lane knows
    the others' rows until the next exchange: the two LOWEST rows must come out, whichever lane holds them."""
    _long_plan(gpu_ctx)
    q, t = (a.copy() for a in long_rows)
    rng = np.random.default_rng(len(layout))
    want = {}
    for j0, s0 in ((7, 4 * 1024 + 2 * STAGE), (9, STAGE)):
        rows = [s0 + o for o in EQUAL_ROWS[layout]] + [s0 + STAGE + 2]
        for r in rows:
            t[r] = _at(rng, q[j0], 6)
        q[j0 + 32] = q[j0]
        want[j0] = want[j0 + 32] = sorted(rows)[:2]
    idx, dist = _agree(gpu_ctx, q, t, layout)
    for j, rows in want.items():
        assert idx[j].tolist() == rows and dist[j].tolist() == [6, 6], (layout, j, idx[j], dist[j])
