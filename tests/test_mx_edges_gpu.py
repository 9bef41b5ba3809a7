"""GPU: the matrix-core top-2 search (bf_mx.hip) at the edges the VALU kernel's suite covers - train sets shorter than one
LDS stage, partial query tiles, both chunk regimes and shrinking tail chunks, one and 256 workers per query block, exact
ties on every chunk and stage boundary, train sets beyond 2^23 rows (MX and VALU passes merged in one call), the selections
and host calls at shapes the default engine sends to the MX kernel, the committed goldens, the routing boundary of
bf_mx_auto, and mixed traffic on one context.

Every search is compared bit for bit with oracle.bf_knn_c (all rows, or a sample of >= 512 plus the size-independent
properties of every row) and with the VALU kernel (engine 1), and must leave the merge state idle.  Cases that aim at a plan
regime derive their shape from slamhip.mx_plan_describe and assert that the regime is reached."""
import contextlib
import ctypes
import json
import os

import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

PASS = 1 << 23
INT_MAX = 2**31 - 1
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@contextlib.contextmanager
def engine(ctx, e):
    """Force the top-2 engine on ctx (0 auto, 1 VALU, 2 matrix cores) and always restore the shipped one."""
    ctx.set_engine(e)
    try:
        yield
    finally:
        ctx.set_engine(0)


def plan(ctx, n, m):
    import slamhip

    return slamhip.mx_plan_describe(n, m, num_cu=ctx.plan_info(n, m)["cus"])


def rand(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def flip(row, bits):
    out = np.unpackbits(row).copy()
    out[list(bits)] ^= 1
    return np.packbits(out)


def search(ctx, q, t, e, train_base=0, dt=None):
    """knn2_device on device-resident rows with engine e; the train rows may already be on the device (dt)."""
    import slamhip

    n, m = len(q), len(t) if dt is None else dt.rows
    dq = slamhip.DeviceDescriptors(ctx, q)
    own = dt is None
    if own:
        dt = slamhip.DeviceDescriptors(ctx, t)
    tab = slamhip.Top2Table(ctx, n)
    try:
        with engine(ctx, e):
            slamhip.knn2_device(ctx, dq.buf, n, dt.buf, m, tab.idx, tab.dist, train_base)
            out = tab.download()
    finally:
        for o in (tab, dq) + ((dt,) if own else ()):
            o.free()
    assert ctx.state_dirty() == 0, "the search left its merge state dirty"
    return out


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def with_base(idx, base):
    return np.where(idx >= 0, idx + base, idx).astype(np.int32)


def properties(q, t, idx, dist, base=0):
    """What every row of a top-2 table must satisfy whatever its size: ordered by (distance, index), distinct rows, and the
    reported distances are the true distances of the reported rows."""
    assert (dist[:, 0] <= dist[:, 1]).all()
    tie = dist[:, 0] == dist[:, 1]
    assert (idx[tie, 0] < idx[tie, 1]).all()
    assert (idx[:, 0] != idx[:, 1]).all()
    for col in (0, 1):
        d = np.bitwise_count(q ^ t[idx[:, col] - base]).sum(1)
        assert np.array_equal(d, dist[:, col]), col


def sample(rng, n, k=512):
    """k random query rows plus the first and last 64 (the partial tile and wave are where the tail is)."""
    s = set(rng.choice(n, min(n, k), replace=False).tolist()) | set(range(min(n, 64))) | set(range(max(0, n - 64), n))
    return np.array(sorted(s), np.int64)


RATIO_CASES = [(3, 4), (3, 5), (2, 2), (0, 1), (2, 4), (6, 8)]      # (d0, d1): exact ties of the ratio test at 0.75 and 0.5


def plant_ratio_cases(rng, q, t, queries):
    """Give each of these queries two close train rows at the distances of RATIO_CASES (in turn); the others are ~128 away."""
    rows = rng.choice(len(t), 2 * len(queries), replace=False)
    for j, i in enumerate(queries):
        d0, d1 = RATIO_CASES[j % len(RATIO_CASES)]
        t[rows[2 * j]] = flip(q[i], range(d0))
        t[rows[2 * j + 1]] = flip(q[i], range(8, 8 + d1))


def check_large(ctx, q, t, e, seed):
    """A large search on engine e: a sample against the oracle, every row's properties, every row against engine 1."""
    rng = np.random.default_rng(seed)
    idx, dist = search(ctx, q, t, e)
    sel = sample(rng, len(q))
    ridx, rdist = oracle.bf_knn_c(q[sel], t, 2, threads=16)
    assert np.array_equal(idx[sel], ridx) and np.array_equal(dist[sel], rdist)
    properties(q, t, idx, dist)
    assert same((idx, dist), search(ctx, q, t, 1))
    return idx, dist


# ---- 1. train-set geometry on the forced matrix-core engine ----------------------------------------------------------------

@pytest.mark.parametrize("m", [1, 2, 15, 16, 17, 127, 128, 129, 255, 256, 257, 1023, 1025])
def test_short_train_sets(gpu_ctx, m):
    """Train sets shorter than one LDS stage, one stage, a stage and a row: the zero rows of a short stage are masked."""
    ctx = gpu_ctx
    rng = np.random.default_rng(1000 + m)
    t = rand(rng, m)
    for n in (1, 64, 1000):
        p, tbl = plan(ctx, n, m)
        assert p["chunk"] == 256 and p["tail_chunks"] == p["chunks"]
        if m < p["stage_rows"]:                                 # the only stage is short
            assert p["chunks"] == 1 and tbl == [0, m]
        q = rand(rng, n)
        q[0] = t[m - 1]                                         # the last row, and an all-zero query: a leaked zero row is at 0
        q[-1] = 0
        ridx, rdist = oracle.bf_knn_c(q, t, 2, threads=16)
        got = search(ctx, q, t, 2)
        assert same(got, (ridx, rdist)), (n, m)
        assert same(got, search(ctx, q, t, 1)), (n, m)
        if m == 1:
            assert (got[0][:, 1] == -1).all() and (got[1][:, 1] == INT_MAX).all() and (got[0][:, 0] == 0).all()


def test_empty_train_set_on_the_mx_engine(gpu_ctx):
    import slamhip

    ctx = gpu_ctx
    q = rand(np.random.default_rng(0), 300)
    dq, dt = slamhip.DeviceDescriptors(ctx, q), slamhip.DeviceDescriptors(ctx, None, rows=0)
    tab = slamhip.Top2Table(ctx, 300)
    try:
        with engine(ctx, 2):
            slamhip.knn2_device(ctx, dq.buf, 300, dt.buf, 0, tab.idx, tab.dist)
            idx, dist = tab.download()
    finally:
        for o in (tab, dq, dt):
            o.free()
    assert ctx.state_dirty() == 0
    assert (idx == -1).all() and (dist == INT_MAX).all()


@pytest.mark.parametrize("n,m,chunk", [(1000, 150001, 256), (65537, 30001, 1024)])
def test_chunk_regimes(gpu_ctx, n, m, chunk):
    """Uniform chunks of 256 and of 1024 rows, each followed by shrinking tail chunks."""
    ctx = gpu_ctx
    p, tbl = plan(ctx, n, m)
    assert p["chunk"] == chunk and 1 <= p["tail_chunks"] < p["chunks"]
    sizes = np.diff(tbl)
    assert (sizes[:p["chunks"] - p["tail_chunks"]] == chunk).all() and (sizes[-p["tail_chunks"]:] < chunk).all()
    rng = np.random.default_rng(n + m)
    q, t = rand(rng, n), rand(rng, m)
    q[n - 1] = t[m - 1]
    q[0] = t[tbl[1] - 1]                                        # the last row of the first uniform chunk
    if n <= 4096:
        ridx, rdist = oracle.bf_knn_c(q, t, 2, threads=16)
        for e in (2, 1):
            assert same(search(ctx, q, t, e), (ridx, rdist)), e
    else:
        idx, _ = check_large(ctx, q, t, 2, seed=n)
        assert idx[n - 1, 0] == m - 1 and idx[0, 0] == tbl[1] - 1


# ---- 2. partial query tiles ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 15, 16, 17, 31, 33, 63, 65, 255, 257, 4097])
def test_query_tails(gpu_ctx, n):
    """Partial 16-query tiles compute a clamped duplicate of the last query: nothing of it may reach another query's row."""
    ctx = gpu_ctx
    m = 20011
    rng = np.random.default_rng(n)
    q, t = rand(rng, n), rand(rng, m)
    for i in range(n):                                          # each query has its own exact copy: every row's answer differs
        t[(7919 * i + 3) % m] = q[i]
    assert len(np.unique(q, axis=0)) == n
    p, _ = plan(ctx, n, m)
    assert p["qblocks"] == (n + 255) // 256
    ridx, rdist = oracle.bf_knn_c(q, t, 2, threads=16)
    for e in (2, 1):
        assert same(search(ctx, q, t, e), (ridx, rdist)), e
    assert (rdist[:, 0] == 0).all()


# ---- 3. worker-count extremes ----------------------------------------------------------------------------------------------

def test_256_workers_per_query_block(gpu_ctx):
    ctx = gpu_ctx
    n, m = 1000, 200000
    p, _ = plan(ctx, n, m)
    assert p["workers"] == min(256, p["chunks"]) == 256
    rng = np.random.default_rng(256)
    q, t = rand(rng, n), rand(rng, m)
    q[:100] = t[rng.choice(m, 100, replace=False)]
    ridx, rdist = oracle.bf_knn_c(q, t, 2, threads=16)
    for e in (2, 0, 1):
        assert same(search(ctx, q, t, e), (ridx, rdist)), e


def test_one_worker_per_query_block(gpu_ctx):
    """More query blocks than the device holds at once: one worker walks every chunk of its query block."""
    ctx = gpu_ctx
    n, m = (1 << 18) + 3, 16384
    p, _ = plan(ctx, n, m)
    assert p["workers"] == 1 and p["qblocks"] > ctx.plan_info(n, m)["cus"] * p["resident"] and p["chunk"] == 1024
    rng = np.random.default_rng(18)
    q, t = rand(rng, n), rand(rng, m)
    rows = rng.choice(m, 4096, replace=False)
    q[rng.choice(n, 4096, replace=False)] = t[rows]
    check_large(ctx, q, t, 2, seed=19)


# ---- 4. ties at every boundary ---------------------------------------------------------------------------------------------

def _boundary_rows(tbl, m, cap=320):
    rows = set()
    for b in tbl[1:-1]:
        rows |= {r for r in (b - 1, b, b + 127, b + 128) if 0 <= r < m}
        if len(rows) >= cap:
            break
    return sorted(rows)


@pytest.mark.parametrize("n,m", [(1000, 150001), (65537, 30001), (130, 20011)])
def test_one_row_on_every_boundary(gpu_ctx, n, m):
    """One row copied to both sides of every chunk boundary and of the stage boundaries inside the chunks: queries equal
    to it get its two lowest copies, at distance 0 - found by different workers and lanes out of index order."""
    ctx = gpu_ctx
    p, tbl = plan(ctx, n, m)
    assert p["chunks"] > 8
    rng = np.random.default_rng(m)
    q, t = rand(rng, n), rand(rng, m)
    rows = _boundary_rows(tbl, m)
    t[rows] = t[rows[-1]]
    where = [0, 15, 16, 63, 64, 255, n - 1] if n > 256 else [0, 15, 16, 63, 64, n - 1]
    q[where] = t[rows[0]]
    if n <= 4096:
        ridx, rdist = oracle.bf_knn_c(q, t, 2, threads=16)
        for e in (2, 1):
            assert same(search(ctx, q, t, e), (ridx, rdist)), e
        idx, dist = ridx, rdist
    else:
        idx, dist = check_large(ctx, q, t, 2, seed=m)
    for w in where:
        assert idx[w].tolist() == rows[:2] and dist[w].tolist() == [0, 0], w


@pytest.mark.parametrize("n,m", [(1000, 150001), (65537, 30001)])
def test_pairs_straddling_every_boundary(gpu_ctx, n, m):
    """A distinct row per boundary, once on each side of it: each query equal to one finds exactly that pair, in order."""
    ctx = gpu_ctx
    p, tbl = plan(ctx, n, m)
    rng = np.random.default_rng(m + 1)
    q, t = rand(rng, n), rand(rng, m)
    pairs = []
    for b in tbl[1:-1][:80]:                                   # chunk boundaries, then the stage boundary 128 rows in
        pairs.append((b - 1, b))
        if b + 128 < m and b + 128 not in tbl:
            pairs.append((b + 127, b + 128))
    assert any(b + 128 not in tbl for b in tbl[1:-1][:80]), "no stage boundary inside a chunk"
    qi = rng.choice(n, len(pairs), replace=False)
    for i, (a, b) in zip(qi, pairs):
        t[b] = t[a]
        q[i] = t[a]
    if n <= 4096:
        ridx, rdist = oracle.bf_knn_c(q, t, 2, threads=16)
        for e in (2, 1):
            assert same(search(ctx, q, t, e), (ridx, rdist)), e
        idx, dist = ridx, rdist
    else:
        idx, dist = check_large(ctx, q, t, 2, seed=m)
    for i, (a, b) in zip(qi, pairs):
        assert idx[i].tolist() == [a, b] and dist[i].tolist() == [0, 0], (i, a, b)


@pytest.mark.parametrize("m", [700, 20011])
def test_all_ties_and_extremes_on_the_mx_engine(gpu_ctx, m):
    """test_matching_gpu.test_all_ties_and_extremes's data on engine 2: all distances 0, all 256, a descending ladder."""
    ctx = gpu_ctx
    q = np.zeros((130, 32), np.uint8)
    t = np.zeros((m, 32), np.uint8)
    for e in (2, 1):
        idx, dist = search(ctx, q, t, e)
        assert (idx == [0, 1]).all() and (dist == 0).all(), e
    t[:] = 0xFF
    for e in (2, 1):
        idx, dist = search(ctx, q, t, e)
        assert (idx == [0, 1]).all() and (dist == 256).all(), e
    bits = np.ones((m, 256), np.uint8)                          # row i < 257 has the first 256 - i bits set, the rest all
    for i in range(257):
        bits[i, 256 - i:] = 0
    t = np.packbits(bits, axis=1)
    ridx, rdist = oracle.bf_knn_c(q, t, 2, threads=16)
    for e in (2, 1):
        assert same(search(ctx, q, t, e), (ridx, rdist)), e
    assert ridx[0].tolist() == [256, 255] and rdist[0].tolist() == [0, 1]


def test_every_distance_in_a_partial_tile(gpu_ctx):
    """Planted pairs at every distance 0..256 with N not a multiple of 16, the last tile holding planted queries."""
    ctx = gpu_ctx
    rng = np.random.default_rng(4243)
    n, m = 281, 16411
    q, t = rand(rng, n), rand(rng, m)
    q[:, :4] = 0xF0
    planted = {}
    for d in range(257):
        qi = (d + 24) % n                                       # distances 232..256 land in queries 256..280
        row = (97 * d + 13) % m
        t[row] = flip(q[qi], rng.permutation(256)[:d])
        planted[qi] = (d, row)
    ridx, rdist = oracle.bf_knn_c(q, t, 2, threads=16)
    for e in (2, 1):
        assert same(search(ctx, q, t, e), (ridx, rdist)), e
    for qi, (d, row) in planted.items():
        if d < 60:
            assert ridx[qi, 0] == row and rdist[qi, 0] == d


# ---- 5. train sets beyond one key range ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def big(gpu_ctx):
    """2^23 + 777 train rows, on the host and on the device, with planted rows: an exact copy of a query in pass 1, one row
    in pass 0 duplicated in pass 1, and one row on each side of the pass boundary."""
    import slamhip

    m = PASS + 777
    rng = np.random.default_rng(23)
    t = rand(rng, m)
    t[PASS + 9] = t[5]
    t[PASS] = t[PASS - 1]
    dt = slamhip.DeviceDescriptors(gpu_ctx, t)
    yield t, dt, {}
    dt.free()


def _big_queries(t, n, seed):
    rng = np.random.default_rng(seed)
    q = rand(rng, n)
    q[0] = t[len(t) - 1]
    q[1] = t[5]
    q[2] = t[PASS - 1]
    q[3] = flip(t[77], range(3))                                # a clear nearest row: the ratio test keeps it
    q[n - 1] = t[PASS + 400]
    return q


def _big_oracle(big, n, seed):
    """The queries of _big_queries and their oracle tables, computed once per module (5 * 10^9 pairs at n = 640)."""
    t, _, cache = big
    if (n, seed) not in cache:
        q = _big_queries(t, n, seed)
        cache[(n, seed)] = (q,) + oracle.bf_knn_c(q, t, 2, threads=16)
    return cache[(n, seed)]


@pytest.mark.parametrize("n,e", [(640, 0), (130, 2)])
def test_two_passes(gpu_ctx, big, n, e):
    """N = 640 on the default engine runs pass 0 on the MX kernel and pass 1 (777 rows) on the VALU kernel; N = 130 with
    engine 2 runs both on the MX kernel.  The merge orders ties across the passes by index, with a train_base."""
    ctx = gpu_ctx
    t, dt, _ = big
    m = len(t)
    p0, tbl0 = plan(ctx, n, PASS)
    p1, _ = plan(ctx, n, m - PASS)
    assert p0["chunk"] == 1024 and p0["workers"] == 256 and tbl0[-1] == PASS
    if e == 0:
        assert p0["auto"] == 1 and p1["auto"] == 0                # the engines differ between the passes
    q, ridx, rdist = _big_oracle(big, n, n)
    assert ridx[0, 0] == m - 1 and ridx[1].tolist() == [5, PASS + 9] and ridx[2].tolist() == [PASS - 1, PASS]
    base = 1000003
    for b in (0, base):
        got = search(ctx, q, None, e, train_base=b, dt=dt)
        assert same(got, (with_base(ridx, b), rdist)), b
        assert same(got, search(ctx, q, None, 1, train_base=b, dt=dt)), b


def test_two_pass_selection(gpu_ctx, big):
    """knn2_select_device beyond 2^23 rows (search in passes, then the selection) and slam_bf_match_host with the train
    rows on the device and the query rows kept there."""
    import slamhip

    ctx = gpu_ctx
    t, dt, _ = big
    n, m = 640, len(t)
    q, ridx, rdist = _big_oracle(big, n, n)
    keep_ratio = oracle.bf_ratio_c(ridx, rdist, 0.8)
    dq = slamhip.DeviceDescriptors(ctx, q)
    tab = slamhip.Top2Table(ctx, n)
    flags = ctx.malloc(n)
    kq = ctx.malloc(32 * n)
    try:
        for e in (0, 2, 1):
            with engine(ctx, e):
                cnt = slamhip.knn2_select_device(ctx, dq.buf, n, dt.buf, m, tab.idx, tab.dist, flags, mode=2, param=0.8,
                                                 train_base=7)
                fl = flags.download(np.uint8, (n,)).astype(bool)
                ti, td = tab.download()
                assert ctx.state_dirty() == 0
                cnt0 = slamhip.knn2_select_device(ctx, dq.buf, n, dt.buf, m, tab.idx, tab.dist, flags, mode=0)
                assert cnt0 == n and flags.download(np.uint8, (n,)).all()
                out = slamhip.matching._match_host(ctx, q, None, dt.buf, m, kq, 0, 0.0)
                assert ctx.state_dirty() == 0
            assert cnt == keep_ratio.sum() and np.array_equal(fl, keep_ratio), e
            assert same((ti, td), (with_base(ridx, 7), rdist)), e
            assert np.array_equal(kq.download(np.uint8, (n, 32)), q), e
            assert np.array_equal(out[0], np.arange(n)) and np.array_equal(out[1], ridx[:, 0]), e
            assert np.array_equal(out[2], rdist[:, 0].astype(np.float32)), e
    finally:
        for o in (tab, dq, flags, kq):
            o.free()
    assert keep_ratio[3] and keep_ratio.sum() < n


# ---- 6. selections and host calls at shapes the default engine runs on the MX kernel ---------------------------------------

def test_host_calls_on_the_mx_kernel(gpu_ctx):
    import slamhip

    ctx = gpu_ctx
    n, m = 8192, 16384
    assert plan(ctx, n, m)[0]["auto"] == 1
    rng = np.random.default_rng(8192)
    q, t = rand(rng, n), rand(rng, m)
    dup = rng.choice(n, 300, replace=False)
    q[dup] = t[rng.choice(m, 300, replace=False)]
    q[dup[:150], 0] ^= 0x11                                     # near-duplicates at distance 2: the filters keep something
    qs = np.setdiff1d(np.arange(n), dup)[:24]                   # planted ratio cases: two close rows each
    plant_ratio_cases(rng, q, t, qs)
    ei, ed = oracle.bf_knn_c(q, t, 2, threads=16)
    keep = oracle.bf_ratio_c(ei, ed, 0.75)
    for j, i in enumerate(qs):
        d0, d1 = RATIO_CASES[j % len(RATIO_CASES)]
        assert ed[i].tolist() == [d0, d1]
        assert keep[i] == (d0 < 0.75 * d1), (j, ed[i])        # 3 < 0.75 * 4 and 6 < 0.75 * 8 are false: the test is strict
    for e in (0, 1):
        with engine(ctx, e):
            assert same(slamhip.knn_match_arrays(q, t, 2, ctx=ctx), (ei, ed)), e
            for thr in (None, 30.0, 400.0):
                got = slamhip.match_arrays(t, q, thr, ctx=ctx)
                assert same(got, oracle.bf_match_c(t, q, thr, threads=16)), (e, thr)
                assert ctx.state_dirty() == 0
            rq, rt, rd = slamhip.ratio_test_arrays(q, t, 0.75, ctx=ctx)
            assert np.array_equal(rq, np.flatnonzero(keep)) and np.array_equal(rt, ei[keep, 0]), e
            assert np.array_equal(rd, ed[keep, 0].astype(np.float32)), e
            assert ctx.state_dirty() == 0
    # one train row: every query has a single neighbour (no second distance), on the forced MX engine
    ei1, ed1 = oracle.bf_knn_c(q, t[:1], 2, threads=16)
    keep1 = oracle.bf_ratio_c(ei1, ed1, 0.75)
    for e in (2, 1):
        with engine(ctx, e):
            assert same(slamhip.knn_match_arrays(q, t[:1], 2, ctx=ctx), (ei1, ed1)), e
            rq, rt, rd = slamhip.ratio_test_arrays(q, t[:1], 0.75, ctx=ctx)
        assert np.array_equal(rq, np.flatnonzero(keep1)) and (rt == 0).all(), e
        assert ctx.state_dirty() == 0


def test_cross_check_on_the_mx_kernel(gpu_ctx):
    """Forward and reverse search on device rows (both MX at 8192 x 16384 and 16384 x 8192 on engine 2), then
    slam_bf_cross_check; and the host call."""
    import slamhip

    ctx = gpu_ctx
    n, m = 8192, 16384
    rng = np.random.default_rng(316)
    q, t = rand(rng, n), rand(rng, m)
    q[:2000] = t[rng.choice(m, 2000, replace=False)]
    q[:1000, 3] ^= 0x01
    oi, od = oracle.bf_cross_check_c(q, t, threads=16)
    assert (oi >= 0).sum() >= 2000
    for e in (2, 1):
        with engine(ctx, e):
            dq, dt = slamhip.DeviceDescriptors(ctx, q), slamhip.DeviceDescriptors(ctx, t)
            fwd, rev = slamhip.Top2Table(ctx, n), slamhip.Top2Table(ctx, m)
            ci, cd = ctx.malloc(n * 4), ctx.malloc(n * 4)
            try:
                slamhip.knn2_device(ctx, dq.buf, n, dt.buf, m, fwd.idx, fwd.dist)
                slamhip.knn2_device(ctx, dt.buf, m, dq.buf, n, rev.idx, rev.dist)
                cnt = ctypes.c_int64(-1)
                assert ctx.lib.slam_bf_cross_check(ctx.handle, fwd.idx.ptr, fwd.dist.ptr, n, rev.idx.ptr, m, ci.ptr, cd.ptr,
                                                   ctypes.byref(cnt)) == 0
                gi, gd = ci.download(np.int32, (n,)), cd.download(np.int32, (n,))
            finally:
                for o in (ci, cd, fwd, rev, dq, dt):
                    o.free()
            assert ctx.state_dirty() == 0
            assert np.array_equal(gi, oi) and np.array_equal(gd, od) and cnt.value == (oi >= 0).sum(), e
            cq, ct, cdist = slamhip.cross_check_arrays(q, t, ctx=ctx)
            assert ctx.state_dirty() == 0
        assert np.array_equal(cq, np.flatnonzero(oi >= 0)) and np.array_equal(ct, oi[oi >= 0]), e
        assert np.array_equal(cdist, od[oi >= 0].astype(np.float32)), e


def test_collection_and_keyframe_database_on_the_mx_kernel(gpu_ctx):
    import slamhip

    ctx = gpu_ctx
    rng = np.random.default_rng(4711)
    sizes = [3000, 0, 5000, 1, 0, 255, 8128]
    imgs = [rand(rng, s) for s in sizes]
    total = sum(sizes)
    n = 8192
    assert total == 16384 and plan(ctx, n, total)[0]["auto"] == 1
    q = rand(rng, n)
    q[0], q[1], q[2] = imgs[3][0], imgs[6][8127], imgs[0][0]
    imgs[2][17] = imgs[0][0]                                    # equal rows in two images: the lower image comes first
    rimg, rtr, rdist = oracle.bf_knn_multi_c(q, imgs, 2, threads=16)
    assert rimg[2].tolist() == [0, 2] and rtr[2].tolist() == [0, 17]
    for e in (0, 1):
        with engine(ctx, e):
            assert same(slamhip.knn_match_collection(q, imgs, 2, ctx=ctx), (rimg, rtr, rdist)), e
            db = slamhip.KeyframeDatabase(ctx, capacity_rows=1000)
            try:
                for im in imgs:
                    db.add(im)
                assert same(db.query(q, 2), (rimg, rtr, rdist)), e
                assert same(db.query(q[:4097], 1), (rimg[:4097, :1], rtr[:4097, :1], rdist[:4097, :1])), e
            finally:
                db.free()
            assert ctx.state_dirty() == 0


def test_select_counts_with_a_partial_wave(gpu_ctx):
    """slam_bf_knn2_select_u256 fused into the MX kernel: flags and count with N % 64 != 0."""
    import slamhip

    ctx = gpu_ctx
    n, m = 8192 + 37, 16384
    assert n % 64 and plan(ctx, n, m)[0]["auto"] == 1
    rng = np.random.default_rng(37)
    q, t = rand(rng, n), rand(rng, m)
    q[-37:] = t[:37]                                            # the partial wave's queries all pass the ratio test
    q[rng.choice(n - 64, 500, replace=False)] = t[rng.choice(m, 500, replace=False)]
    planted = list(range(n - 64, n - 52)) + list(range(n - 30, n - 18))   # ratio ties in the last full wave and the partial one
    q[planted] = rand(rng, len(planted))
    plant_ratio_cases(rng, q, t, planted)
    ei, ed = oracle.bf_knn_c(q, t, 2, threads=16)
    assert [tuple(ed[i]) for i in planted] == [RATIO_CASES[j % len(RATIO_CASES)] for j in range(len(planted))]
    dq, dt = slamhip.DeviceDescriptors(ctx, q), slamhip.DeviceDescriptors(ctx, t)
    tab = slamhip.Top2Table(ctx, n)
    flags = ctx.malloc(n)
    try:
        for e in (0, 2, 1):
            with engine(ctx, e):
                for mode, param in ((2, 0.75), (2, 0.5), (0, 0.0)):
                    cnt = slamhip.knn2_select_device(ctx, dq.buf, n, dt.buf, m, tab.idx, tab.dist, flags, mode=mode, param=param)
                    fl = flags.download(np.uint8, (n,)).astype(bool)
                    assert ctx.state_dirty() == 0
                    want = oracle.bf_ratio_c(ei, ed, param) if mode == 2 else np.ones(n, bool)
                    assert cnt == want.sum() and np.array_equal(fl, want), (e, mode, param)
                    assert same(tab.download(), (ei, ed)), (e, mode)
    finally:
        for o in (tab, dq, dt, flags):
            o.free()


def test_mx_kernel_keeps_the_query_rows(gpu_ctx):
    """A frame-sized slam_bf_match_host with the train rows on the device: on engine 2 the MX kernel itself reads the query
    rows from pinned memory and leaves their device copy (its keep path), N not a multiple of 64."""
    import slamhip

    ctx = gpu_ctx
    n, m = 1000, 4096
    rng = np.random.default_rng(1000)
    q, t = rand(rng, n), rand(rng, m)
    q[:50] = t[100:150]
    plant_ratio_cases(rng, q, t, range(n - 12, n))
    ei, ed = oracle.bf_knn_c(q, t, 2, threads=16)
    dt = slamhip.DeviceDescriptors(ctx, t)
    kq = ctx.malloc(32 * n)
    try:
        for e in (2, 1):
            for mode, param in ((0, 0.0), (2, 0.75)):
                kq.upload(np.zeros((n, 32), np.uint8))
                with engine(ctx, e):
                    qi, ti, di = slamhip.matching._match_host(ctx, q, None, dt.buf, m, kq, mode, param)
                assert ctx.state_dirty() == 0
                assert np.array_equal(kq.download(np.uint8, (n, 32)), q), (e, mode)
                keep = oracle.bf_ratio_c(ei, ed, param) if mode == 2 else np.ones(n, bool)
                assert np.array_equal(qi, np.flatnonzero(keep)) and np.array_equal(ti, ei[keep, 0]), (e, mode)
                assert np.array_equal(di, ed[keep, 0].astype(np.float32)), (e, mode)
    finally:
        dt.free()
        kq.free()


# ---- 7. real and hand-derived data on the MX engine ------------------------------------------------------------------------

def test_image_descriptors_grown_past_the_host_call_limit(gpu_ctx):
    """Real ORB descriptors, each copied eight times with a few bits flipped: near ties everywhere, both sides > 4096."""
    import slamhip

    ctx = gpu_ctx
    g = np.load(os.path.join(GOLD, "image_descriptors.npz"))
    rng = np.random.default_rng(600)

    def grow(d, k):
        out = [d]
        for _ in range(k - 1):
            c = np.unpackbits(d, axis=1)
            pos = rng.integers(0, 256, (len(d), 3))
            np.put_along_axis(c, pos, 1 - np.take_along_axis(c, pos, 1), 1)
            out.append(np.packbits(c, axis=1))
        return np.concatenate(out)

    q, t = grow(g["desc1"], 8), grow(g["desc2"], 9)
    assert len(q) > 4096 and len(t) > 4096
    ridx, rdist = oracle.bf_knn_c(q, t, 2, threads=16)
    for e in (2, 1):
        assert same(search(ctx, q, t, e), (ridx, rdist)), e
        with engine(ctx, e):
            assert same(slamhip.knn_match_arrays(q, t, 2, ctx=ctx), (ridx, rdist)), e
        assert ctx.state_dirty() == 0


def test_goldens_on_the_mx_engine(gpu_ctx):
    """The committed top-2 goldens through the device path on engine 2."""
    import slamhip

    ctx = gpu_ctx

    def gold(name):
        with open(os.path.join(GOLD, name)) as f:
            return json.load(f)

    def d(rows):
        return np.array(rows, np.uint8).reshape(-1, 32)

    for name in ("kat_ladder.json", "kat_ties.json"):
        g = gold(name)
        idx, dist = search(ctx, d(g["query"]), d(g["train"]), 2)
        assert idx.tolist() == g["idx"] and dist.tolist() == g["dist"], name
    g = gold("kat_short_train.json")
    idx, dist = search(ctx, d(g["query"]), d(g["train_one"]), 2)
    assert idx.tolist() == g["idx_one"] and dist.tolist() == g["dist_one"]
    g = gold("kat_ratio.json")
    q, t = d(g["query"]), d(g["train"])
    dq, dt = slamhip.DeviceDescriptors(ctx, q), slamhip.DeviceDescriptors(ctx, t)
    tab = slamhip.Top2Table(ctx, len(q))
    flags = ctx.malloc(len(q))
    try:
        with engine(ctx, 2):
            for key, ratio in (("keep_075", 0.75), ("keep_050", 0.5)):
                cnt = slamhip.knn2_select_device(ctx, dq.buf, len(q), dt.buf, len(t), tab.idx, tab.dist, flags, mode=2,
                                                 param=ratio)
                fl = flags.download(np.uint8, (len(q),)).astype(bool)
                assert fl.tolist() == [bool(x) for x in g[key]] and cnt == sum(bool(x) for x in g[key]), key
    finally:
        for o in (tab, dq, dt, flags):
            o.free()
    assert ctx.state_dirty() == 0
    g = gold("kat_multi_image.json")
    imgs = [d(i) for i in g["images"]]
    idx, dist = search(ctx, d(g["query"]), np.concatenate(imgs), 2)
    img, tr = slamhip.split_image_index(idx, [len(i) for i in imgs])
    assert img.tolist() == g["img"] and tr.tolist() == g["train"] and dist.tolist() == g["dist"]


# ---- 8. the routing boundary of bf_mx_auto ---------------------------------------------------------------------------------

ROUTES = [((8191, 16384), 0), ((8192, 16383), 0), ((8192, 16384), 1),
          ((2999, 40000), 0), ((3000, 39999), 0), ((3000, 40000), 1),
          ((999, 65536), 0), ((1000, 65535), 0), ((1000, 65536), 1),
          ((499, 200000), 0), ((500, 199999), 0), ((500, 200000), 1)]


@pytest.mark.parametrize("shape,auto", ROUTES)
def test_routing_boundary(gpu_ctx, shape, auto):
    """Just inside and just outside each clause of bf_mx_auto: the default engine gives the oracle's answers either way."""
    ctx = gpu_ctx
    n, m = shape
    assert plan(ctx, n, m)[0]["auto"] == auto
    rng = np.random.default_rng(n * 7 + m)
    q, t = rand(rng, n), rand(rng, m)
    q[rng.choice(n, 200, replace=False)] = t[rng.choice(m, 200, replace=False)]
    check_large(ctx, q, t, 0, seed=n + m)


# ---- 9. one context, mixed traffic -----------------------------------------------------------------------------------------

def test_mixed_traffic_on_one_context(gpu_ctx, big):
    import slamhip

    ctx = gpu_ctx
    rng = np.random.default_rng(99)
    n, m = 8192, 16384
    assert plan(ctx, n, m)[0]["auto"] == 1
    q, t = rand(rng, n), rand(rng, m)
    q[:500] = t[rng.choice(m, 500, replace=False)]
    sel = sample(rng, n)
    ridx, rdist = oracle.bf_knn_c(q[sel], t, 2, threads=16)

    first = search(ctx, q, t, 0)                                                # 1. MX search
    assert same((first[0][sel], first[1][sel]), (ridx, rdist))
    properties(q, t, *first)
    try:                                                                        # 2. a knob routes to the VALU kernel
        ctx.set_tuning(feed=1)
        assert same(search(ctx, q, t, 0), first)
    finally:
        ctx.set_tuning()
    small_q, small_t = q[:700], t[:3000]
    dq, dt = slamhip.DeviceDescriptors(ctx, small_q), slamhip.DeviceDescriptors(ctx, small_t)
    try:
        k = 5                                                                   # 3. top-k
        ti, td = ctx.malloc(700 * k * 4), ctx.malloc(700 * k * 4)
        slamhip.knn_topk_device(ctx, dq.buf, 700, dt.buf, 3000, k, ti, td)
        got = ti.download(np.int32, (700, k)), td.download(np.int32, (700, k))
        ti.free()
        td.free()
        assert same(got, oracle.bf_knn_c(small_q, small_t, k, threads=16))
        assert ctx.state_dirty() == 0
        off = ctx.malloc(701 * 8)                                               # 4. radius
        ri, rd = ctx.malloc(700 * 3000 * 4), ctx.malloc(700 * 3000 * 4)
        total = slamhip.radius_device(ctx, dq.buf, 700, dt.buf, 3000, 100.0, off, 700 * 3000, ri, rd)
        offs = off.download(np.int64, (701,))
        gi, gd = ri.download(np.int32, (max(total, 1),))[:total], rd.download(np.int32, (max(total, 1),))[:total]
        for o in (off, ri, rd):
            o.free()
        dm = oracle.hamming_matrix_np(small_q, small_t)
        qi, tj = np.nonzero(dm <= 100)
        order = np.lexsort((tj, dm[qi, tj], qi))
        assert total == len(qi) and np.array_equal(offs, np.r_[0, np.cumsum(np.bincount(qi, minlength=700))])
        assert np.array_equal(gi, tj[order]) and np.array_equal(gd, dm[qi, tj][order])
        assert ctx.state_dirty() == 0
        tabs = [slamhip.Top2Table(ctx, 700), slamhip.Top2Table(ctx, 3000)]     # 5. batched search
        slamhip.knn2_device_batch(ctx, [(dq.buf, 700, dt.buf, 3000, tabs[0].idx, tabs[0].dist),
                                        (dt.buf, 3000, dq.buf, 700, tabs[1].idx, tabs[1].dist, 50)])
        b0, b1 = tabs[0].download(), tabs[1].download()
        for o in tabs:
            o.free()
        assert same(b0, oracle.bf_knn_c(small_q, small_t, 2, threads=16))
        r1 = oracle.bf_knn_c(small_t, small_q, 2, threads=16)
        assert same(b1, (with_base(r1[0], 50), r1[1]))
        assert ctx.state_dirty() == 0
    finally:
        dq.free()
        dt.free()
    n2 = 8192 + 37                                                              # 6. MX select
    q2 = np.concatenate([q, q[:37]])
    dq2, dt2 = slamhip.DeviceDescriptors(ctx, q2), slamhip.DeviceDescriptors(ctx, t)
    tab, flags = slamhip.Top2Table(ctx, n2), ctx.malloc(n2)
    try:
        cnt = slamhip.knn2_select_device(ctx, dq2.buf, n2, dt2.buf, m, tab.idx, tab.dist, flags, mode=2, param=0.75)
        i2, d2 = tab.download()
        fl = flags.download(np.uint8, (n2,)).astype(bool)
    finally:
        for o in (tab, flags, dq2, dt2):
            o.free()
    assert ctx.state_dirty() == 0
    assert same((i2[:n], d2[:n]), first) and same((i2[n:], d2[n:]), (first[0][:37], first[1][:37]))
    want = oracle.bf_ratio_c(i2, d2, 0.75)
    assert cnt == want.sum() and np.array_equal(fl, want)
    tb, dtb, _ = big                                                            # 7. the two-pass search
    qb = _big_queries(tb, 640, 7)
    bi, bd = search(ctx, qb, None, 0, dt=dtb)
    bsel = np.r_[0:8, rng.choice(640, 56, replace=False)]
    assert same((bi[bsel], bd[bsel]), oracle.bf_knn_c(qb[bsel], tb, 2, threads=16))
    assert bi[1].tolist() == [5, PASS + 9] and bi[2].tolist() == [PASS - 1, PASS]
    assert same(search(ctx, q, t, 0), first)                                    # 8. MX search again
