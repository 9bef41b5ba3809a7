"""GPU: the row gates of the matrix-core top-2 search (bf_mx.hip: in a tile that takes the update path, of a lane's four rows
only those at which some lane of the tile passes are keyed and merged), engine 2 against the VALU kernel (engine 1) and
against oracle.bf_knn_c, bit for bit, at the smallest shapes that reach each path.

The rows are tests/hamming_families.prefix_rows, so every distance is |a - b| and chosen.  The 16 queries of a tile share
one prefix b (5, 60, 115, 170, 225 for the five tiles of N = 70: one full wave and a partial tile), so a tile's gates are
decided by the train rows alone.  At these sizes every 128-row stage is a chunk of its own, scanned by a worker that
starts with open thresholds, and a lane's threshold comes from the rows of its own quarter (kg = lane >> 4 holds rows
4 kg + r of a group) until the stage ends.  So every stage opens with HOLDERS: in groups 0-2, for each tile and each
quarter, two rows at distances 10 and 11.  After them every lane of the tile lets a row in only below 11, and rows planted
for another tile are at least 40 away.  A PATTERN is planted in a later group of the stage, in one quarter: rows at
distances 9, 8, 7, 6 where the pattern passes, and rows AT 11 - ties with the lane's 2nd-best distance, which lose on the
index - in the pattern's own quarter and in the quarters below and above it.  Each tile gets one pattern, the last word on
its queries' top-2: a gate that skipped one of its rows would change the table.

`replay` restates the per-lane rules for one tile and a fresh worker per stage, and each case asserts with it that the
row gates that open in the pattern's group are exactly the named ones: none, only r = 0, only r = 3, two, all four.  (A
foreign bound that arrives at a chunk start can only close gates for rows that are not in the final top-2.)

Rows past the train set: tile 0's queries (b = 5) are at distance 5 from the zero rows that fill a short stage, nearer than
every real row, so a zero row that leaked past the select would head their table.

As tests/test_mx_ties_gpu.py this module shows agreement; the rule itself is pinned by tests/test_mx_rowgate_cpu.py."""
import numpy as np
import pytest

from oracle import oracle
from hamming_families import prefix_rows
from test_mx_ties_gpu import plan, same, search

pytestmark = pytest.mark.gpu

N = 70                              # one full wave and a partial tile (queries 64 .. 69)
TILE_B = (5, 60, 115, 170, 225)     # the prefix length of each tile's queries
FAR = 256                           # a train row at least 31 from every query
STAGE = 128
NONE, R0, R3, TWO, ALL = (), (0,), (3,), (1, 2), (0, 1, 2, 3)


def queries(n=N):
    return np.array([TILE_B[min(i // 16, 4)] for i in range(n)], np.int64)


def planted(m, patterns):
    """Prefix lengths of m train rows.  patterns: (tile, stage, group of the stage (3 .. 7), quarter kg, rows r that pass)."""
    a = np.full(m, FAR, np.int64)

    def put(row, v):
        if row < m:
            assert a[row] == FAR, "two planted rows collide"
            a[row] = v

    for s0 in range(0, m, STAGE):                          # holders: 5 tiles x 2 rows in the 12 slots of each quarter
        for kg in range(4):
            slots = [s0 + 16 * g + 4 * kg + r for g in range(3) for r in range(4)]
            for t, b in enumerate(TILE_B):
                put(slots[2 * t], b + 10)
                put(slots[2 * t + 1], b + 11)
    for t, stage, grp, kg, rs in patterns:
        base, b = STAGE * stage + 16 * grp, TILE_B[t]
        for j, r in enumerate(rs):
            put(base + 4 * kg + r, b + 9 - j)
        for r in range(4):                                 # ties with the lanes' 2nd-best distance, around the passing rows
            if r not in rs:
                put(base + 4 * kg + r, b + 11)
        put(base + 4 * ((kg - 1) % 4) + 1, b + 11)
        put(base + 4 * ((kg + 1) % 4) + 2, b + 11)
    return a


def replay(a, b):
    """{group: the rows r whose gate opens} for a tile whose queries all have prefix b: the kernel's per-lane rules, one
    fresh worker per stage, no foreign bound.  A lane is a quarter here (the 16 queries of the tile are alike)."""
    m, out = len(a), {}
    for s0 in range(0, m, STAGE):
        pair = [[] for _ in range(4)]                      # per quarter: the keys (distance, row) of its top-2
        x = [511] * 4                                      # exclusive threshold distances
        for g0 in range(s0, min(s0 + STAGE, m), 16):
            d = [[abs(int(a[g0 + 4 * kg + r]) - b) if g0 + 4 * kg + r < m else None for r in range(4)] for kg in range(4)]
            opened = tuple(r for r in range(4) if any(d[kg][r] is not None and d[kg][r] < x[kg] for kg in range(4)))
            if not opened:
                continue
            out[g0 // 16] = opened
            for kg in range(4):
                pair[kg] = sorted(pair[kg] + [(d[kg][r], g0 + 4 * kg + r) for r in opened if d[kg][r] is not None])[:2]
                if len(pair[kg]) == 2:
                    x[kg] = min(x[kg], pair[kg][1][0])
    return out


def run(ctx, a, b, check_plan):
    import slamhip

    q, t = prefix_rows(b), prefix_rows(a)
    n, m = len(q), len(t)
    p, tbl = plan(ctx, n, m)
    assert p["stage_rows"] == STAGE and tbl[0] == 0 and tbl[-1] == m
    check_plan(p, tbl)
    ridx, rdist = oracle.bf_knn_c(q, t, 2, threads=16)
    dq, dt = slamhip.DeviceDescriptors(ctx, q), slamhip.DeviceDescriptors(ctx, t)
    try:
        mx = search(ctx, dq, n, dt, m, 2)
        valu = search(ctx, dq, n, dt, m, 1)
    finally:
        dq.free()
        dt.free()
    assert same(mx, (ridx, rdist))
    assert same(mx, valu)
    return mx


def check_patterns(a, patterns, idx, dist):
    """The data does what the case says: in each pattern's group exactly the named gates open for its tile, and the pattern
    decides the tile's table - its passing rows head it, nearest first, then the first holders (distance 10)."""
    m = len(a)
    for t, stage, grp, kg, rs in patterns:
        b, g = TILE_B[t], 8 * stage + grp
        rs = tuple(r for r in rs if 16 * g + 4 * kg + r < m)
        assert replay(a, b).get(g, ()) == rs, (t, g, replay(a, b))
        rows = [16 * g + 4 * kg + r for r in rs][::-1][:2]                     # the later the row, the nearer
        holders = [r for r in range(m) if a[r] == b + 10][:2 - len(rows)]
        want = rows + holders
        sel = np.nonzero(queries() == b)[0]
        assert (idx[sel] == np.array(want)).all(), (t, want, idx[sel][0])
        assert (dist[sel] == np.abs(a[want] - b)).all()


# one pattern per tile; the stages, groups and quarters differ from tile to tile
CASES = {
    272: [(0, 0, 4, 1, NONE), (1, 0, 6, 0, R0), (2, 1, 3, 2, R3), (3, 1, 5, 3, TWO), (4, 1, 7, 0, ALL)],
    257: [(0, 1, 7, 3, R3), (1, 1, 4, 2, ALL), (2, 0, 5, 1, NONE), (3, 0, 3, 0, TWO), (4, 1, 6, 1, R0)],
    # the short last stage: 7 whole groups and one of 15 rows; the last pattern ends in the row before the end of the train set
    383: [(0, 2, 7, 3, TWO), (1, 2, 3, 1, R3), (2, 2, 4, 0, ALL), (3, 2, 5, 2, NONE), (4, 2, 6, 3, R0)],
}


@pytest.mark.parametrize("m", sorted(CASES))
def test_passing_row_patterns(gpu_ctx, m):
    """M = 272: two whole stages and one group; M = 257: one row in the last stage; M = 383: every pattern in the short last
    stage.  Each stage is a chunk of its own.  Rows past M are at distance 5 from tile 0's queries, whose table is headed by
    rows at 9 or 10 (M = 272, 257) or at 8 and 9 (M = 383)."""
    a = planted(m, CASES[m])

    def check(p, tbl):
        assert tbl == [0, 128, 256, m] and p["chunks"] == 3 and p["workers"] == 3 and p["qblocks"] == 1

    idx, dist = run(gpu_ctx, a, queries(), check)
    check_patterns(a, CASES[m], idx, dist)
    assert (dist[:16, 0] > 5).all() and (idx < m).all()                       # no zero row of the short stage in tile 0's table


def test_many_workers_and_foreign_bounds(gpu_ctx):
    """M = 2176, 1000 queries: 17 single-stage chunks of the 256-row regime, one worker each, so that foreign bounds arrive
    between gated updates; prefix lengths from few values, so that most rows tie."""
    rng = np.random.default_rng(2176)
    a = rng.choice(np.array([90, 100, 101, 102, 110, 140, 200]), 2176)
    b = 96 + rng.integers(0, 9, 1000)

    def check(p, tbl):
        assert p["chunk"] == 256 and p["workers"] >= 16 and p["qblocks"] == 4 and p["chunks"] == 17

    run(gpu_ctx, a, b, check)


def test_all_rows_equal(gpu_ctx):
    """Every row ties: no gate may open after the first two rows."""
    def check(p, tbl):
        assert tbl == [0, 128, 256, 272]

    idx, dist = run(gpu_ctx, np.full(272, 100), np.full(N, 100), check)
    assert (idx == np.array([0, 1])).all() and (dist == 0).all()


def test_strictly_descending_distances(gpu_ctx):
    """Every row is nearer than every row before it: every group fires in every tile and every row gate opens."""
    m = 250

    def check(p, tbl):
        assert tbl == [0, 128, m] and p["workers"] == 2

    idx, dist = run(gpu_ctx, m - np.arange(m), np.zeros(N, np.int64), check)
    assert (idx == np.array([m - 1, m - 2])).all() and (dist == np.array([1, 2])).all()
