"""GPU suite for the radius search (bf_radius.hip, BFMatcher.radiusMatch): exact compressed rows against a reference built
from oracle.hamming_matrix_np, the (distance, train index) order with planted ties, the long-list sort path, train sets
beyond 2^23 rows, agreement with the top-k search, the capacity protocol, and every interface built on it."""
import ctypes

import numpy as np
import pytest

from hamming_families import ref_radius
from oracle import oracle

pytestmark = pytest.mark.gpu

PASS = 1 << 23
RADII = (-1.0, float("nan"), 0.0, 40.0, 64.5, 96.0, 104.0, 128.0, 255.0, 256.0, 1e9)


def rand_desc(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def assert_csr(got, want, what):
    off, idx, dist = got
    roff, ridx, rdist = want
    assert off.dtype == np.int64 and idx.dtype == np.int32 and dist.dtype == np.int32, what
    assert np.array_equal(off, roff), f"{what}: offsets differ (totals {off[-1]} vs {roff[-1]})"
    bad = np.nonzero((idx != ridx) | (dist != rdist))[0]
    assert bad.size == 0, f"{what}: {bad.size} entries differ, first at {bad[0]}: ({idx[bad[0]]}, {dist[bad[0]]}) vs ({ridx[bad[0]]}, {rdist[bad[0]]})"


class Csr:
    """Device offsets [n + 1] and idx / dist [cap] buffers."""

    def __init__(self, ctx, n, cap):
        self.n, self.cap = n, cap
        self.off = ctx.malloc((n + 1) * 8)
        self.idx = ctx.malloc(max(cap, 1) * 4)
        self.dist = ctx.malloc(max(cap, 1) * 4)

    def download(self, total):
        off = self.off.download(np.int64, (self.n + 1,))
        if total == 0:
            return off, np.zeros(0, np.int32), np.zeros(0, np.int32)
        return off, self.idx.download(np.int32, (total,)), self.dist.download(np.int32, (total,))

    def free(self):
        for b in (self.off, self.idx, self.dist):
            b.free()


@pytest.mark.parametrize("n,m", [(1, 1), (63, 65), (200, 200), (3, 4097), (4096, 4096)])
def test_exact_csr_against_the_reference(gpu_ctx, n, m):
    import slamhip

    rng = np.random.default_rng(31 * n + m)
    q, t = rand_desc(rng, n), rand_desc(rng, m)
    if m > 8:                                                      # planted duplicates and an exact match
        t[m // 2] = t[1]
        q[n // 2] = t[1]
    want = ref_radius(q, t, RADII)
    for r in RADII:
        got = slamhip.radius_match_arrays(q, t, r, ctx=gpu_ctx)
        assert_csr(got, want[r], f"{n}x{m} r={r}")
        assert gpu_ctx.state_dirty() == 0
    if (n, m) == (4096, 4096):                                     # the binomial estimate is only a sanity bound on the setup
        assert want[96.0][0][-1] < 0.001 * n * m and want[104.0][0][-1] > 1000
        assert want[256.0][0][-1] == n * m and want[-1.0][0][-1] == 0


def test_many_chunks(gpu_ctx):
    import slamhip

    n, m = 1024, 300_000
    assert slamhip.plan_describe_radius(n, m, num_cu=256)["chunks"] > 100
    rng = np.random.default_rng(5)
    q, t = rand_desc(rng, n), rand_desc(rng, m)
    t[250_000:250_010] = q[7]                                      # exact matches deep in the train set
    radii = (-1.0, float("nan"), 0.0, 64.5, 96.0, 104.0)
    want = ref_radius(q, t, radii)
    for r in radii:
        assert_csr(slamhip.radius_match_arrays(q, t, r, ctx=gpu_ctx), want[r], f"{n}x{m} r={r}")
    off, idx, dist = slamhip.radius_match_arrays(q, t, 0.0, ctx=gpu_ctx)
    assert idx[off[7]:off[8]].tolist() == list(range(250_000, 250_010)) and not dist[off[7]:off[8]].any()
    assert gpu_ctx.state_dirty() == 0


def flip(row, bits):
    """row with the given bit positions inverted"""
    out = row.copy()
    for b in bits:
        out[b // 8] ^= np.uint8(1 << (b % 8))
    return out


def test_ties_come_in_train_index_order(gpu_ctx):
    import slamhip

    rng = np.random.default_rng(11)
    q, t = rand_desc(rng, 5), rand_desc(rng, 3000)
    plant = rng.permutation(3000)[:300]                            # 300 rows at distances 3 and 5 from query 2, in random slots
    for j, row in enumerate(plant):
        t[row] = flip(q[2], rng.permutation(256)[:3 if j % 2 else 5])
    t[plant[:20:2]] = t[plant[0]]                                  # exact duplicates among them
    off, idx, dist = slamhip.radius_match_arrays(q, t, 5.0, ctx=gpu_ctx)
    i, d = idx[off[2]:off[3]], dist[off[2]:off[3]]
    assert len(i) >= 300 and set(plant.tolist()) <= set(i.tolist())
    key = d.astype(np.int64) << 32 | i
    assert (np.diff(key) > 0).all(), "not ordered by (distance, train index)"
    assert_csr((off, idx, dist), ref_radius(q, t, (5.0,))[5.0], "ties")


def test_long_lists_take_the_tiled_sort(gpu_ctx):
    import slamhip

    n, m = 4, 100_000
    assert m > slamhip.plan_describe_radius(n, m)["short_max"]
    rng = np.random.default_rng(12)
    q, t = rand_desc(rng, n), rand_desc(rng, m)
    t[::1000] = q[1]                                               # duplicates spread over many tiles
    want = ref_radius(q, t, (256.0, 120.0))
    for r in (256.0, 120.0):                                       # every list holds M entries / about 40 % of them
        got = slamhip.radius_match_arrays(q, t, r, ctx=gpu_ctx)
        assert_csr(got, want[r], f"long r={r}")
    assert np.array_equal(np.diff(want[256.0][0]), [m] * n)
    assert gpu_ctx.state_dirty() == 0


def test_train_sets_beyond_2_pow_23_rows(gpu_ctx):
    import slamhip

    n, m = 4, PASS + 4096
    rng = np.random.default_rng(13)
    q = rand_desc(rng, n)
    t = rand_desc(rng, m)
    near = [PASS - 1, PASS, PASS + 1, PASS + 4095, 12345]
    for j, row in enumerate(near):
        t[row] = flip(q[j % n], rng.permutation(256)[: 2 * j])      # distances 0, 2, 4, 6, 8
    t[PASS + 100] = t[PASS + 1]                                    # a tie beyond 2^23
    want = ref_radius(q, t, (40.0, 90.0), step=1 << 20)
    for r in (40.0, 90.0):
        got = slamhip.radius_match_arrays(q, t, r, ctx=gpu_ctx)
        assert_csr(got, want[r], f"passes r={r}")
    off, idx, dist = slamhip.radius_match_arrays(q, t, 40.0, ctx=gpu_ctx)
    assert idx[off[1]:off[2]].tolist()[:1] == [PASS] and dist[off[1]] == 2
    assert idx[off[2]:off[3]].tolist()[:2] == [PASS + 1, PASS + 100] and dist[off[2]:off[2] + 2].tolist() == [4, 4]
    assert gpu_ctx.state_dirty() == 0


def test_agrees_with_the_topk_search(gpu_ctx):
    import slamhip

    rng = np.random.default_rng(14)
    q, t = rand_desc(rng, 2000), rand_desc(rng, 20000)
    t[100:140] = q[3]                                              # one query with more than 32 exact matches
    kidx, kdist = slamhip.topk_match_arrays(q, t, 32, ctx=gpu_ctx)
    for r in (0.0, 90.0, 96.0, 100.5):
        off, idx, dist = slamhip.radius_match_arrays(q, t, r, ctx=gpu_ctx)
        checked = 0
        for i in range(q.shape[0]):
            c = int(off[i + 1] - off[i])
            if c > 32:
                assert (kdist[i] <= r).all()
                continue
            assert idx[off[i]:off[i + 1]].tolist() == kidx[i, :c].tolist(), (r, i)
            assert dist[off[i]:off[i + 1]].tolist() == kdist[i, :c].tolist(), (r, i)
            if c < 32:
                assert kdist[i, c] > r, (r, i)
            checked += 1
        assert checked >= 0.99 * q.shape[0]                        # (query 3 and the odd random one hold more than 32)


def test_train_base_rerun_and_capacity(gpu_ctx):
    import slamhip

    rng = np.random.default_rng(15)
    q, t = rand_desc(rng, 3000), rand_desc(rng, 50000)
    want = ref_radius(q, t, (100.0,))[100.0]
    dq, dt = slamhip.DeviceDescriptors(gpu_ctx, q), slamhip.DeviceDescriptors(gpu_ctx, t)
    total = int(want[0][-1])
    small, big = Csr(gpu_ctx, 3000, 0), Csr(gpu_ctx, 3000, total)
    try:
        # too small: the exact total, valid offsets, nothing else
        got = slamhip.radius_device(gpu_ctx, dq.buf, 3000, dt.buf, 50000, 100.0, small.off, 0, None, None, train_base=1000)
        assert got == total and total > 0
        assert np.array_equal(small.download(0)[0], want[0])
        assert gpu_ctx.state_dirty() == 0
        got = slamhip.radius_device(gpu_ctx, dq.buf, 3000, dt.buf, 50000, 100.0, small.off, total - 1, big.idx, big.dist, train_base=1000)
        assert got == total
        runs = []
        for _ in range(2):
            assert slamhip.radius_device(gpu_ctx, dq.buf, 3000, dt.buf, 50000, 100.0, big.off, total, big.idx, big.dist,
                                         train_base=1000) == total
            runs.append(big.download(total))
            assert gpu_ctx.state_dirty() == 0
        assert all(np.array_equal(a, b) for a, b in zip(runs[0], runs[1])), "two calls differ"
        assert_csr(runs[0], (want[0], want[1] + 1000, want[2]), "train_base")
    finally:
        for o in (small, big, dq, dt):
            o.free()


def test_empty_sides(gpu_ctx):
    import slamhip

    rng = np.random.default_rng(16)
    q = rand_desc(rng, 50)
    off, idx, dist = slamhip.radius_match_arrays(q, np.zeros((0, 32), np.uint8), 256.0, ctx=gpu_ctx)
    assert off.tolist() == [0] * 51 and idx.size == 0 and dist.size == 0
    off, idx, dist = slamhip.radius_match_arrays(np.zeros((0, 32), np.uint8), q, 256.0, ctx=gpu_ctx)
    assert off.tolist() == [0] and idx.size == 0
    assert gpu_ctx.state_dirty() == 0


def test_collection_and_keyframe_database(gpu_ctx):
    import slamhip

    rng = np.random.default_rng(17)
    imgs = [rand_desc(rng, r) for r in (500, 0, 1200, 77)]
    q = rand_desc(rng, 300)
    imgs[2][5] = imgs[0][9] = q[4]                                 # the same distance in two images: imgIdx decides
    cat = np.concatenate(imgs)
    want = ref_radius(q, cat, (96.0,))[96.0]
    starts = np.cumsum([0] + [len(x) for x in imgs])
    ref_img = np.searchsorted(starts, want[1], side="right") - 1
    off, img, local, dist = slamhip.radius_match_collection(q, imgs, 96.0, ctx=gpu_ctx)
    assert np.array_equal(off, want[0]) and np.array_equal(dist, want[2])
    assert np.array_equal(img, ref_img) and np.array_equal(local, want[1] - starts[ref_img])
    assert img[off[4]:off[4] + 2].tolist() == [0, 2] and local[off[4]:off[4] + 2].tolist() == [9, 5]
    db = slamhip.KeyframeDatabase(gpu_ctx, capacity_rows=256)
    try:
        for x in imgs:
            db.add(x)
        for r in (96.0, 256.0, 96.0):                              # grows its buffers, then reuses them
            got = db.query_radius(q, r)
            want_r = want if r == 96.0 else ref_radius(q, cat, (r,))[r]
            assert np.array_equal(got[0], want_r[0]) and np.array_equal(got[3], want_r[2])
            g = starts[got[1]] + got[2]
            assert np.array_equal(g, want_r[1])
        o, i, lo, d = db.query_radius(np.zeros((0, 32), np.uint8), 50.0)
        assert o.tolist() == [0] and i.size == 0
    finally:
        db.free()
    assert gpu_ctx.state_dirty() == 0


def test_dropin_radius_match(gpu_ctx):
    from feature_matchers import BruteForceFeatureMatcher

    rng = np.random.default_rng(18)
    q, t = rand_desc(rng, 200), rand_desc(rng, 200)
    t[17] = q[3]
    t[90] = q[3]
    want = ref_radius(q, t, (90.0,))[90.0]
    bf = BruteForceFeatureMatcher(norm_type=6)
    full = bf.radius_match(q, t, 90.0)
    assert len(full) == 200
    for i, lst in enumerate(full):
        a, b = want[0][i], want[0][i + 1]
        assert [m.trainIdx for m in lst] == want[1][a:b].tolist()
        assert [m.distance for m in lst] == want[2][a:b].astype(float).tolist()
        assert all(m.queryIdx == i and m.imgIdx == 0 for m in lst)
    assert [(m.trainIdx, m.distance) for m in full[3][:2]] == [(17, 0.0), (90, 0.0)]
    compact = bf.radius_match(q, t, 90.0, compact_result=True)
    fields = lambda lists: [[(m.queryIdx, m.trainIdx, m.imgIdx, m.distance) for m in lst] for lst in lists]  # noqa: E731
    assert fields([lst for lst in full if lst]) == fields(compact)
    assert len(compact) == int((np.diff(want[0]) > 0).sum())


def test_invalid_arguments_launch_nothing(gpu_ctx):
    from slamhip import _lib

    lib = gpu_ctx.lib
    h = gpu_ctx.handle
    rng = np.random.default_rng(19)
    q = gpu_ctx.upload(rand_desc(rng, 8))
    res = gpu_ctx.malloc(1024)
    tot = ctypes.c_int64(-5)
    try:
        calls = [
            (None, q.ptr, 8, q.ptr, 8, 10.0, 0, res.ptr, 8, res.ptr, res.ptr, ctypes.byref(tot)),
            (h, q.ptr, -1, q.ptr, 8, 10.0, 0, res.ptr, 8, res.ptr, res.ptr, ctypes.byref(tot)),
            (h, q.ptr, 8, q.ptr, -1, 10.0, 0, res.ptr, 8, res.ptr, res.ptr, ctypes.byref(tot)),
            (h, q.ptr, 8, q.ptr, 8, 10.0, 0, None, 8, res.ptr, res.ptr, ctypes.byref(tot)),
            (h, q.ptr, 8, q.ptr, 8, 10.0, 0, res.ptr, 8, res.ptr, res.ptr, None),
            (h, None, 8, q.ptr, 8, 10.0, 0, res.ptr, 8, res.ptr, res.ptr, ctypes.byref(tot)),
            (h, q.ptr, 8, None, 8, 10.0, 0, res.ptr, 8, res.ptr, res.ptr, ctypes.byref(tot)),
            (h, q.ptr, 8, q.ptr, 8, 10.0, 0, res.ptr, 8, None, res.ptr, ctypes.byref(tot)),
            (h, q.ptr, 8, q.ptr, 8, 10.0, 0, res.ptr, -1, res.ptr, res.ptr, ctypes.byref(tot)),
            (h, q.ptr, 8, q.ptr, 8, 10.0, -1, res.ptr, 8, res.ptr, res.ptr, ctypes.byref(tot)),
            (h, q.ptr, 8, q.ptr, 8, 10.0, 2**31 - 4, res.ptr, 8, res.ptr, res.ptr, ctypes.byref(tot)),
        ]
        for args in calls:
            assert lib.slam_bf_radius_u256(*args) == _lib.SLAM_ERR_INVALID, args
        assert tot.value == -5                                     # nothing was written, nothing launched
        hq = np.zeros((8, 32), np.uint8)
        ho = np.zeros(9, np.int64)
        assert lib.slam_bf_radius_u256_host(h, _lib.addr(hq), -2, _lib.addr(hq), 8, 10.0, _lib.addr(ho), 0, None, None,
                                            ctypes.byref(tot)) == _lib.SLAM_ERR_INVALID
        assert lib.slam_bf_radius_u256_host(h, _lib.addr(hq), 8, _lib.addr(hq), 8, 10.0, None, 0, None, None,
                                            ctypes.byref(tot)) == _lib.SLAM_ERR_INVALID
        assert lib.slam_bf_radius_u256_host(h, _lib.addr(hq), 8, _lib.addr(hq), 8, 10.0, _lib.addr(ho), 4, None, None,
                                            ctypes.byref(tot)) == _lib.SLAM_ERR_INVALID
        # the valid forms of the same call
        assert lib.slam_bf_radius_u256(h, q.ptr, 8, q.ptr, 8, 300.0, 0, res.ptr, 0, None, None, ctypes.byref(tot)) == 0
        assert tot.value == 64
        assert lib.slam_bf_radius_u256(h, None, 0, None, 0, 10.0, 0, res.ptr, 0, None, None, ctypes.byref(tot)) == 0
        assert tot.value == 0 and res.download(np.int64, (1,)).tolist() == [0]
    finally:
        q.free()
        res.free()
    assert gpu_ctx.state_dirty() == 0
