"""GPU: the group gates of a fired 32x32 tile (bf_mx32_scan.inc, engine 3) under both feeds (mxfeed 1 = expanded in the kernel,
2 = prepared image) against the VALU kernel (engine 1) and the CPU oracle: tables bit for bit, every search run twice, the
merge state idle after each.

One wave, M = 256 (two stages).  Every query but the target is the descriptor w, the target is v; rows 0 .. 7 of the first group
hold two near rows per lane half for each (v: accumulator indices 0 and 1, w: 2 and 3), so every threshold is warm after the
first group and every later group is quiet - but for what a case plants.  A planted row is near v only, so it passes in ONE lane
of ONE tile: the target's column, the lane half that holds the row.  Accumulator index i of lane half hk of group g of stage s
is row 128 s + 32 g + 8 (i >> 2) + 4 hk + (i & 3)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STAGE, GROUP, M = 128, 32, 256
FEEDS = (1, 2)
SIZES = (64, 33, 65)
TARGET = {0: 5, 1: 32}                                  # the target query of tile 0 / tile 1 (query 32 exists at every N)
NEAR = (40, 44, 46, 48)                                 # rows 0, 1 (lane half 0) and 4, 5 (lane half 1) from the target
VARIANTS = {"nearest": 20, "second": 42, "tie_with_second": 44}
GATE_GROUPS = ((0, 1, 14, 15), (2, 3, 4), (5, 6, 7), (8, 9, 10), (11, 12, 13))


def row_of(i, hk, g=2, s=0):
    return STAGE * s + GROUP * g + 8 * (i >> 2) + 4 * hk + (i & 3)


def _at(rng, row, d):
    bits = np.unpackbits(row)
    bits[rng.permutation(256)[:d]] ^= 1
    return np.packbits(bits)


def _run(ctx, q, t, engine, feed):
    """The search twice on one pair of buffers; both tables must be equal and the merge state idle after each."""
    import slamhip

    ctx.set_engine(engine)
    ctx.set_mx_feed(feed)
    dq, dt = slamhip.DeviceDescriptors(ctx, q), slamhip.DeviceDescriptors(ctx, t)
    tab = slamhip.Top2Table(ctx, len(q))
    try:
        outs = []
        for _ in range(2):
            slamhip.knn2_device(ctx, dq.buf, len(q), dt.buf, len(t), tab.idx, tab.dist)
            outs.append(tab.download())
            assert ctx.state_dirty() == 0, "the search left its merge state dirty"
    finally:
        ctx.set_engine(0)
        ctx.set_mx_feed(0)
        for o in (tab, dq, dt):
            o.free()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]), "two runs of one search differ"
    return outs[1]


def _check(ctx, q, t, feeds, what):
    """Engine 3 under every feed == engine 1 == the oracle.  Returns the table."""
    import slamhip
    from oracle import oracle

    assert slamhip.mx_tile_describe(len(q), len(t), 3) == 32
    ridx, rdist = oracle.bf_knn_c(q, t, 2)
    a = _run(ctx, q, t, 1, 0)
    assert np.array_equal(a[0], ridx) and np.array_equal(a[1], rdist), ("engine 1 against the oracle", what)
    for feed in feeds:
        b = _run(ctx, q, t, 3, feed)
        bad = np.nonzero((b[0] != ridx).any(axis=1) | (b[1] != rdist).any(axis=1))[0]
        assert bad.size == 0, (what, "feed", feed, "queries", bad[:4], b[0][bad[:4]], b[1][bad[:4]], "want", ridx[bad[:4]], rdist[bad[:4]])
    return ridx, rdist


def _scene(seed, n, tile, m=M, near=NEAR, near_w=NEAR):
    """(rng, q, t, target query): every query w but the target v, the warm rows planted, all else random."""
    rng = np.random.default_rng(seed)
    v, w = rng.integers(0, 256, 32, dtype=np.uint8), rng.integers(0, 256, 32, dtype=np.uint8)
    q = np.tile(w, (n, 1))
    j = TARGET[tile]
    q[j] = v
    t = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    for r, d in zip((0, 1, 4, 5), near):
        t[r] = _at(rng, v, d)
    for r, d in zip((2, 3, 6, 7), near_w):
        t[r] = _at(rng, w, d)
    return rng, q, t, j


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("feed", FEEDS)
@pytest.mark.parametrize("n", SIZES)
def test_one_passing_row_at_every_accumulator_index(gpu_ctx, n, feed, variant):
    """64 placements: index 0 .. 15 x lane half x tile x (a later group of the first stage | the first group of the second)."""
    d = VARIANTS[variant]
    for tile in (0, 1):
        rng, q, t0, j = _scene(7000 + 10 * n + tile, n, tile)
        for g, s in ((2, 0), (0, 1)):
            for hk in (0, 1):
                for i in range(16):
                    t = t0.copy()
                    r = row_of(i, hk, g, s)
                    t[r] = _at(rng, q[j], d)
                    idx, dist = _check(gpu_ctx, q, t, (feed,), (variant, "tile", tile, "index", i, "half", hk, "group", g, "stage", s))
                    want = {"nearest": ([r, 0], [d, 40]), "second": ([0, r], [40, d]), "tie_with_second": ([0, 1], [40, 44])}[variant]
                    assert idx[j].tolist() == want[0] and dist[j].tolist() == want[1], "the case itself"   # the lower row wins a tie


@pytest.mark.parametrize("n", SIZES)
def test_two_passing_rows_in_one_gate_group_and_in_two(gpu_ctx, n):
    cases = {
        "one group, one lane": ((2, 0), (4, 0)),
        "one group, two lanes": ((2, 0), (4, 1)),
        "the four-row group, one lane": ((1, 1), (14, 1)),
        "two groups, one lane": ((3, 0), (9, 0)),
        "two groups, two lanes": ((7, 1), (11, 0)),
    }
    for tile in (0, 1):
        rng, q, t0, j = _scene(7100 + 10 * n + tile, n, tile)
        for name, ((i0, h0), (i1, h1)) in cases.items():
            same = [grp for grp in GATE_GROUPS if i0 in grp and i1 in grp]
            assert bool(same) == name.startswith(("one group", "the four-row")), name
            t = t0.copy()
            r0, r1 = row_of(i0, h0), row_of(i1, h1)
            t[r0], t[r1] = _at(rng, q[j], 30), _at(rng, q[j], 20)
            idx, dist = _check(gpu_ctx, q, t, FEEDS, (name, "tile", tile))
            assert idx[j].tolist() == [r1, r0] and dist[j].tolist() == [20, 30]


@pytest.mark.parametrize("n", SIZES)
def test_a_row_passes_in_one_tile_while_the_other_stays_quiet(gpu_ctx, n):
    """The target's threshold is loose (near rows at 100 .. 108), every other query's tight (40 .. 48): a planted row at 60 passes
    the target's tile only, and only against that tile's own threshold."""
    for tile in (0, 1):
        rng, q, t0, j = _scene(7200 + 10 * n + tile, n, tile, near=(100, 104, 106, 108))
        for i, hk in ((0, 0), (4, 1), (6, 0), (9, 1), (12, 0), (15, 1)):
            t = t0.copy()
            r = row_of(i, hk)
            t[r] = _at(rng, q[j], 60)
            idx, dist = _check(gpu_ctx, q, t, FEEDS, ("tile", tile, "index", i, "half", hk))
            assert idx[j, 0] == r and dist[j, 0] == 60
            others = np.delete(np.arange(n), j)
            assert (idx[others] == [2, 3]).all() and (dist[others] == [40, 44]).all(), "the other tile's queries never see the row"


@pytest.mark.parametrize("n", SIZES)
def test_all_sixteen_rows_of_a_lane_pass(gpu_ctx, n):
    for tile in (0, 1):
        for hk in (0, 1):
            rng, q, t, j = _scene(7300 + 10 * n + 2 * tile + hk, n, tile)
            for i in range(16):
                t[row_of(i, hk)] = _at(rng, q[j], 10 + (15 - i))          # the nearest come last
            idx, dist = _check(gpu_ctx, q, t, FEEDS, ("tile", tile, "half", hk))
            assert idx[j].tolist() == [row_of(15, hk), row_of(14, hk)] and dist[j].tolist() == [10, 11]


@pytest.mark.parametrize("n", SIZES)
def test_the_cold_path_every_row_far(gpu_ctx, n):
    """Every train row is the complement of a row near the queries: all distances >= 129, no threshold ever leaves the pattern
    that lets everything pass, every tile fires and every row enters."""
    rng = np.random.default_rng(7400 + n)
    v = rng.integers(0, 256, 32, dtype=np.uint8)
    q = np.stack([_at(rng, v, int(k)) for k in rng.integers(0, 20, n)])
    t = np.stack([~_at(rng, v, int(k)) for k in rng.integers(0, 100, M)])
    idx, dist = _check(gpu_ctx, q, t, FEEDS, "cold")
    assert dist.min() >= 129


@pytest.mark.parametrize("m", [96, 127, 129, 160])
@pytest.mark.parametrize("n", SIZES)
def test_the_ragged_tail_never_lets_the_zero_rows_in(gpu_ctx, n, m):
    """The planted row is the last valid row; the target has four set bits, so the rows of zero bits that both feeds store behind M
    would be its nearest by far (distance 4) if they entered."""
    for tile in (0, 1):
        rng = np.random.default_rng(7500 + 1000 * m + 10 * n + tile)
        q = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        j = TARGET[tile]
        q[j] = 0
        q[j, [3, 11, 19, 30]] = (0x10, 0x01, 0x80, 0x04)
        t = rng.integers(0, 256, (m, 32), dtype=np.uint8)
        t[m - 1] = _at(rng, q[j], 20)
        idx, dist = _check(gpu_ctx, q, t, FEEDS, ("m", m, "tile", tile))
        assert idx[j, 0] == m - 1 and dist[j, 0] == 20 and dist[j, 1] > 20 and (idx < m).all()
