"""GPU: the 32x32x64 matrix-core top-2 search (bf_mx32.hip, engine 3) against the VALU kernel (engine 1), tables bit for bit
and the merge state idle after every search: the lane and K maps on exact data at every distance 0..256, the cold-threshold
path (all dots negative), ragged query and train counts, nearest rows on both sides of a group, a stage and a chunk start,
tie-heavy families, a threshold that moves between two groups, the fused selection with kept rows and a train_base, and the
smallest shape the shipped engine sends to the matrix cores."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ONE_WORKER_N = 513 * 256       # more query blocks than 4 x 256 CUs hold: one worker per query block


def _search(ctx, q, t, engine, train_base=0):
    import slamhip

    ctx.set_engine(engine)
    dq, dt = slamhip.DeviceDescriptors(ctx, q), slamhip.DeviceDescriptors(ctx, t)
    tab = slamhip.Top2Table(ctx, len(q))
    try:
        slamhip.knn2_device(ctx, dq.buf, len(q), dt.buf, len(t), tab.idx, tab.dist, train_base)
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


def _bits(rows):
    return np.unpackbits(np.ascontiguousarray(rows), axis=-1)


def _planted(rng, d, complement):
    """64 queries that differ from one random row in bits 0..5 (query i: the binary code of i), 128 train rows: row p(r), p a
    bijection that moves with d, is query r % 64 with w further bits flipped outside bits 0..5 (and a few inside beyond 250),
    so dist(query i, row p(r)) = popcount(i ^ c_r) + w exactly.  complement: every train row inverted, dist -> 256 - dist."""
    base = _bits(rng.integers(0, 256, 32, dtype=np.uint8))
    code = (np.arange(64)[:, None] >> np.arange(6)) & 1
    qb = np.tile(base, (64, 1))
    qb[:, :6] ^= code.astype(np.uint8)
    w = min(d, 250)
    extra = (1 << (d - w)) - 1
    tb = np.tile(base, (128, 1))
    for r in range(128):
        c = (r % 64) ^ extra
        tb[r, :6] ^= ((c >> np.arange(6)) & 1).astype(np.uint8)
        tb[r, 6 + rng.permutation(250)[:w]] ^= 1
    if complement:
        tb ^= 1
    pos = (np.arange(128) * 37 + d) % 128
    t = np.empty((128, 32), np.uint8)
    t[pos] = np.packbits(tb, axis=-1)
    return np.packbits(qb, axis=-1), t, pos


def test_lane_and_k_maps_at_every_distance(gpu_ctx):
    """M = 128, N = 64: query i has rows p(i) and p(i + 64) at distance d exactly and every other row further away, for every
    d = 0..256, the rows at a place that moves with d: a wrong lane, row, nibble or K map cannot survive this."""
    rng = np.random.default_rng(3232)
    for d in range(257):
        q, t, pos = _planted(rng, d, False)
        idx, dist = _agree(gpu_ctx, q, t, d)
        if d <= 250:
            want = np.sort(np.stack([pos[:64], pos[64:]], 1), 1)
            assert np.array_equal(idx, want) and (dist == d).all(), d
        else:
            assert (dist == 250).all(), d
    # 251..256 as the nearest distances: equal queries, every row their complement but for two rows at distance d
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    q = np.tile(base, (64, 1))
    for d in range(251, 257):
        tb = np.tile(_bits(base) ^ 1, (128, 1))
        rows = sorted(((np.array([5, 77]) * 37 + d) % 128).tolist())
        for r in rows:
            tb[r, rng.permutation(256)[:256 - d]] ^= 1
        idx, dist = _agree(gpu_ctx, q, np.packbits(tb, axis=-1), d)
        assert (idx == (rows if d < 256 else [0, 1])).all() and (dist == d).all(), d      # at 256 every row ties


def test_cold_threshold_path_all_dots_negative(gpu_ctx):
    """Every train row is the complement of a query plus a few flips: all distances are at least 129, every dot is negative, and
    the threshold never comes down to where the fold's signed comparison is exact - the tiles fire unconditionally."""
    rng = np.random.default_rng(12932)
    for d in list(range(0, 122, 3)) + [121]:
        q, t, _ = _planted(rng, d, True)
        idx, dist = _agree(gpu_ctx, q, t, d)
        assert dist.min() >= 129, d
        assert (dist[:, 0] == 256 - d - 6).all()             # the row planted for the query whose code is the complement


@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 300])
def test_ragged_shapes(gpu_ctx, n):
    rng = np.random.default_rng(n)
    q = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    big = rng.integers(0, 256, (16384 + 77, 32), dtype=np.uint8)
    for m in (1, 2, 31, 32, 33, 127, 128, 129, 255, 1151, 16384 + 77):
        t = big[:m].copy()
        t[m - 1] = q[n // 2]                                 # the last row of the train set is somebody's nearest
        idx, dist = _agree(gpu_ctx, q, t, (n, m))
        assert idx[n // 2, 0] == m - 1 and dist[n // 2, 0] == 0


@pytest.mark.parametrize("n,m", [(300, 16384 + 77), (ONE_WORKER_N, 4000)], ids=["many_workers", "one_worker"])
def test_nearest_rows_on_both_sides_of_group_stage_and_chunk(gpu_ctx, n, m):
    import slamhip

    plan, tbl = slamhip.mx_plan_describe(n, m, num_cu=gpu_ctx.plan_info(n, m)["cus"])
    assert plan["workers"] == 1 if n == ONE_WORKER_N else plan["workers"] > 8
    k = len(tbl) // 2
    assert tbl[k] > 1024 and tbl[k + 3] < m
    rng = np.random.default_rng(n + m)
    q = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    want = {}
    combos = [(0, 3, 5), (1, 3, 5), (0, 4, 4), (1, 4, 4)]   # (the nearer row is the higher one, the two distances)
    # the last row of a group, of a stage (in the many-worker plan every stage is a chunk of its own) and of a chunk
    for case, lo in enumerate([31, 63, 95, 159, 127, 255, 383, 511] + [tbl[k + i] - 1 for i in range(4)]):
        swap, d1, d2 = combos[case % 4]
        near, second = (lo + 1, lo) if swap else (lo, lo + 1)
        j = 7 + 11 * case
        qb = _bits(q[j])
        a, b = qb.copy(), qb.copy()
        a[rng.permutation(256)[:d1]] ^= 1
        b[rng.permutation(256)[:d2]] ^= 1
        t[near], t[second] = np.packbits(a), np.packbits(b)
        want[j] = ([near, second] if d1 != d2 else sorted([near, second]), [d1, d2])
    idx, dist = _agree(gpu_ctx, q, t)
    for j, (rows, ds) in want.items():
        assert idx[j].tolist() == rows and dist[j].tolist() == ds, j


def _few_values(rng, n, m):
    vals = np.array([0x00, 0x0F], np.uint8)
    q, t = np.zeros((n, 32), np.uint8), np.zeros((m, 32), np.uint8)
    q[:, :4] = vals[rng.integers(0, 2, (n, 4))]
    t[:, :4] = vals[rng.integers(0, 2, (m, 4))]
    return q, t


def _duplicates(rng, n, m):
    q = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    who = rng.choice(n, min(n, 2048, m // 16), replace=False)
    v = q[who].copy()
    v[np.arange(len(who)), rng.integers(0, 32, len(who))] ^= np.uint8(1) << rng.integers(0, 8, len(who)).astype(np.uint8)
    rows = rng.choice(m, (len(who), 6), replace=False)
    for j in range(6):
        t[rows[:, j]] = v
    return q, t


def _all_equal(rng, n, m):
    v = rng.integers(0, 256, 32, dtype=np.uint8)
    return np.tile(v, (n, 1)), np.tile(v, (m, 1))


@pytest.mark.parametrize("fam", [_few_values, _duplicates, _all_equal], ids=lambda f: f.__name__.strip("_"))
@pytest.mark.parametrize("n,m", [(1000, 20001), (ONE_WORKER_N, 4000)], ids=["many_workers", "one_worker"])
def test_tie_families(gpu_ctx, fam, n, m):
    q, t = fam(np.random.default_rng(n + m), n, m)
    idx, _ = _agree(gpu_ctx, q, t)
    if fam is _all_equal:
        assert (idx == [0, 1]).all()


def test_threshold_moves_between_two_groups(gpu_ctx):
    """Group 2 (rows 64..95) brings the 2nd-best distance down to 12; group 3 holds rows at 11 (passes the new threshold), at 12
    (a tie from a higher row: loses) and at 13..40 (pass only the threshold from before group 2)."""
    rng = np.random.default_rng(96)
    n, m = 64, 256
    q = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    qb = _bits(q[5])

    def at(d):
        r = qb.copy()
        r[rng.permutation(256)[:d]] ^= 1
        return np.packbits(r)

    t[70], t[83] = at(10), at(12)
    t[96], t[97], t[101] = at(12), at(13), at(11)
    for r in range(102, 128):
        t[r] = at(13 + (r - 102))
    idx, dist = _agree(gpu_ctx, q, t)
    assert idx[5].tolist() == [70, 101] and dist[5].tolist() == [10, 11]
    t[101] = at(12)                                          # now the tie at row 83 keeps the second place
    idx, dist = _agree(gpu_ctx, q, t)
    assert idx[5].tolist() == [70, 83] and dist[5].tolist() == [10, 12]


def test_select_keep_and_train_base(gpu_ctx):
    import slamhip

    ctx = gpu_ctx
    rng = np.random.default_rng(77)
    n, m, base = 777, 5000, 123456
    q = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    t[4097] = q[17]
    res = {}
    for engine in (1, 3):
        ctx.set_engine(engine)
        dq, dt = slamhip.DeviceDescriptors(ctx, q), slamhip.DeviceDescriptors(ctx, t)
        tab = slamhip.Top2Table(ctx, n)
        keep = ctx.malloc(n)
        try:
            out = []
            for mode in (0, 2):
                cnt = slamhip.knn2_select_device(ctx, dq.buf, n, dt.buf, m, tab.idx, tab.dist, keep, mode=mode, param=0.8,
                                                 train_base=base)
                out += [np.asarray(cnt), keep.download(np.uint8, (n,))] + list(tab.download())
        finally:
            ctx.set_engine(0)
            for o in (tab, dq, dt, keep):
                o.free()
        assert ctx.state_dirty() == 0
        res[engine] = out
    for x, y in zip(res[1], res[3]):
        assert np.array_equal(x, y)
    assert res[3][2][17, 0] == base + 4097 and res[3][3][17, 0] == 0


def test_smallest_auto_routed_shape(gpu_ctx):
    import slamhip

    n, m = 8192, 16384
    plan, _ = slamhip.mx_plan_describe(n, m, num_cu=gpu_ctx.plan_info(n, m)["cus"])
    assert plan["auto"] == 1
    rng = np.random.default_rng(8192)
    q = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    t[9000] = t[3]
    q[9] = t[3]
    idx, _ = _agree(gpu_ctx, q, t)
    assert idx[9].tolist() == [3, 9000]
    auto = _search(gpu_ctx, q, t, 0)
    assert np.array_equal(auto[0], idx)


def test_engine_3_is_accepted_and_4_is_not(gpu_ctx):
    from slamhip._lib import SlamHipError

    try:
        gpu_ctx.set_engine(3)
        for bad in (4, -1):
            with pytest.raises(SlamHipError):
                gpu_ctx.set_engine(bad)
    finally:
        gpu_ctx.set_engine(0)
