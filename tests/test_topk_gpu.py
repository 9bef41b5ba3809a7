"""GPU suite for the top-k search (bf_topk.hip, knnMatch with k up to 32): every new entry point bit-exact against the C
oracle's K-best insertion (oracle.bf_knn_c / bf_knn_multi_c), the hand-derived answers of tests/golden/kat_topk.json,
the top-2 search as a cross-check at k = 2, and the shared merge state left idle after every call."""
import ctypes
import json
import os

import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASS = 1 << 23
KS = (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 31, 32)
NO_IDX, NO_DIST = -1, 2**31 - 1


def rand_desc(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


class Tables:
    """Device [n, k] idx / dist tables."""

    def __init__(self, ctx, n, k):
        self.n, self.k = n, k
        self.idx = ctx.malloc(max(n * k, 1) * 4)
        self.dist = ctx.malloc(max(n * k, 1) * 4)

    def download(self):
        return self.idx.download(np.int32, (self.n, self.k)), self.dist.download(np.int32, (self.n, self.k))

    def free(self):
        self.idx.free()
        self.dist.free()


def device_topk(ctx, q, t, k, train_base=0):
    """knn_topk_device on freshly uploaded rows; returns the downloaded tables."""
    import slamhip

    dq, dt = slamhip.DeviceDescriptors(ctx, q), slamhip.DeviceDescriptors(ctx, t)
    tab = Tables(ctx, q.shape[0], k)
    try:
        slamhip.knn_topk_device(ctx, dq.buf, q.shape[0], dt.buf, t.shape[0], k, tab.idx, tab.dist, train_base=train_base)
        return tab.download()
    finally:
        for o in (tab, dq, dt):
            o.free()


def assert_oracle(q, t, k, idx, dist, what=""):
    ridx, rdist = oracle.bf_knn_c(q, t, k, threads=16)
    assert idx.shape == ridx.shape and dist.shape == rdist.shape, what
    bad = np.nonzero((idx != ridx).any(1) | (dist != rdist).any(1))[0]
    assert bad.size == 0, f"{what}: {bad.size} rows differ, first {bad[0]}: {idx[bad[0]]} {dist[bad[0]]} vs {ridx[bad[0]]} {rdist[bad[0]]}"


def assert_well_formed(q, t, idx, dist, train_base=0):
    """Every row sorted by (dist, idx), no index twice, and every distance recomputed from the descriptors."""
    valid = idx >= 0
    assert (dist[~valid] == NO_DIST).all()
    assert (valid[:, :-1] >= valid[:, 1:]).all()                   # neighbours first, then only missing ones
    key = dist.astype(np.int64) << 32 | (idx.astype(np.int64) & 0xFFFFFFFF)
    assert (np.diff(np.where(valid, key, np.iinfo(np.int64).max), axis=1) > 0)[valid[:, 1:]].all()
    rows = np.where(valid, idx - train_base, 0)
    d = np.bitwise_count(q[:, None, :] ^ t[rows]).sum(-1, dtype=np.int32)
    assert np.array_equal(np.where(valid, d, NO_DIST), dist)


@pytest.mark.parametrize("n,m", [(1, 1), (63, 65), (200, 200), (257, 511), (1000, 3), (3, 1000), (4096, 4096)])
def test_parity_with_the_oracle(gpu_ctx, n, m):
    import slamhip

    rng = np.random.default_rng(1000 * n + m)
    q, t = rand_desc(rng, n), rand_desc(rng, m)
    if m > 8:                                                      # planted duplicates: ties the index rule decides
        t[m // 2] = t[1]
        q[n // 2] = t[1]
    for k in KS:
        idx, dist = slamhip.topk_match_arrays(q, t, k, ctx=gpu_ctx)
        assert_oracle(q, t, k, idx, dist, f"{n}x{m} k={k}")
    assert gpu_ctx.state_dirty() == 0


def test_parity_on_the_device_entry_point_with_a_train_base(gpu_ctx):
    rng = np.random.default_rng(7)
    q, t = rand_desc(rng, 3000), rand_desc(rng, 20000)
    for k in (3, 8, 32):
        idx, dist = device_topk(gpu_ctx, q, t, k, train_base=1000)
        ridx, rdist = oracle.bf_knn_c(q, t, k, threads=16)
        assert np.array_equal(idx, np.where(ridx >= 0, ridx + 1000, -1)) and np.array_equal(dist, rdist), k
    assert gpu_ctx.state_dirty() == 0


def test_fewer_train_rows_than_k_and_empty_sides(gpu_ctx):
    import slamhip

    rng = np.random.default_rng(8)
    q = rand_desc(rng, 300)
    for m in (1, 2, 5, 31):
        t = rand_desc(rng, m)
        for k in (m + 1, 32):
            idx, dist = slamhip.topk_match_arrays(q, t, k, ctx=gpu_ctx)
            assert_oracle(q, t, k, idx, dist, f"M={m} k={k}")
            assert (idx[:, m:] == NO_IDX).all() and (dist[:, m:] == NO_DIST).all()
            idx, dist = device_topk(gpu_ctx, q, t, k)
            assert_oracle(q, t, k, idx, dist, f"device M={m} k={k}")
    idx, dist = slamhip.topk_match_arrays(q, np.zeros((0, 32), np.uint8), 6, ctx=gpu_ctx)
    assert idx.shape == (300, 6) and (idx == NO_IDX).all() and (dist == NO_DIST).all()
    idx, dist = device_topk(gpu_ctx, q, np.zeros((0, 32), np.uint8), 6)
    assert (idx == NO_IDX).all() and (dist == NO_DIST).all()
    idx, dist = slamhip.topk_match_arrays(np.zeros((0, 32), np.uint8), q, 9, ctx=gpu_ctx)
    assert idx.shape == (0, 9) and dist.shape == (0, 9)
    assert gpu_ctx.state_dirty() == 0


def test_ties_straddling_chunk_boundaries(gpu_ctx):
    import slamhip

    rng = np.random.default_rng(9)
    n, m = 64, 65536
    for k in (5, 32):
        plan = slamhip.plan_describe_topk(n, m, k, num_cu=gpu_ctx.plan_info(n, m)["cus"])
        assert plan["chunks"] >= 4, plan
        q, t = rand_desc(rng, n), rand_desc(rng, m)
        row = t[0].copy()
        b = plan["chunk"]
        pos = np.r_[np.arange(b - 50, b + 50), np.arange(2 * b - 3, 2 * b + 3)]     # 100 rows across the first boundary, more behind
        t[pos] = row
        q[:10] = row
        idx, dist = slamhip.topk_match_arrays(q, t, k, ctx=gpu_ctx)
        assert_oracle(q, t, k, idx, dist, f"ties k={k}")
        assert (idx[:10] == np.sort(np.r_[0, pos])[:k]).all() and (dist[:10] == 0).all()
        # spread: the same row every 600 rows, in many chunks
        t2 = rand_desc(rng, m)
        spread = np.arange(100) * 600 + 77
        t2[spread] = row
        idx, dist = slamhip.topk_match_arrays(q, t2, k, ctx=gpu_ctx)
        assert (idx[:10] == spread[:k]).all() and (dist[:10] == 0).all()
        assert_oracle(q, t2, k, idx, dist, f"spread ties k={k}")
    assert gpu_ctx.state_dirty() == 0


def test_real_image_descriptors(gpu_ctx):
    import slamhip

    z = np.load(os.path.join(ROOT, "tests", "golden", "image_descriptors.npz"))
    d1, d2 = z["desc1"], z["desc2"]
    for k in KS:
        idx, dist = slamhip.topk_match_arrays(d2, d1, k, ctx=gpu_ctx)
        assert_oracle(d2, d1, k, idx, dist, f"images k={k}")
        idx, dist = slamhip.topk_match_arrays(np.r_[d1, d2], np.r_[d2, d1, d1], k, ctx=gpu_ctx)
        assert_oracle(np.r_[d1, d2], np.r_[d2, d1, d1], k, idx, dist, f"images doubled k={k}")


@pytest.mark.parametrize("k", [8, 32])
def test_65536_squared_sampled(gpu_ctx, k):
    rng = np.random.default_rng(228)
    q, t = rand_desc(rng, 65536), rand_desc(rng, 65536)
    idx, dist = device_topk(gpu_ctx, q, t, k)
    assert gpu_ctx.state_dirty() == 0
    assert_well_formed(q, t, idx, dist)
    rows = np.random.default_rng(5).choice(65536, 512, replace=False)
    assert_oracle(q[rows], t, k, idx[rows], dist[rows], f"65536^2 k={k}")


def test_4096_by_2_20_sampled(gpu_ctx):
    rng = np.random.default_rng(229)
    q, t = rand_desc(rng, 4096), rand_desc(rng, 1 << 20)
    idx, dist = device_topk(gpu_ctx, q, t, 8)
    assert gpu_ctx.state_dirty() == 0
    assert_well_formed(q, t, idx, dist)
    rows = np.random.default_rng(6).choice(4096, 512, replace=False)
    assert_oracle(q[rows], t, 8, idx[rows], dist[rows], "4096 x 2^20 k=8")


def test_train_set_beyond_one_pass(gpu_ctx):
    rng = np.random.default_rng(11)
    n, m = 256, PASS + 4096
    q, t = rand_desc(rng, n), rand_desc(rng, m)
    # ties planted across the pass boundary: query 0 equals rows on both sides of it, query 1 sits at distance 1 from rows there
    for r in (PASS - 3, PASS + 2, 17, PASS + 4000):
        t[r] = q[0]
    near = q[1].copy()
    near[0] ^= 1
    for r in (PASS - 1, PASS, 5):
        t[r] = near
    for k in (3, 8, 32):
        idx, dist = device_topk(gpu_ctx, q, t, k, train_base=7)
        ridx, rdist = oracle.bf_knn_c(q, t, k, threads=16)
        assert np.array_equal(idx, np.where(ridx >= 0, ridx + 7, -1)) and np.array_equal(dist, rdist), k
        assert idx[0, :3].tolist() == [17 + 7, PASS - 3 + 7, PASS + 2 + 7] and dist[0, :3].tolist() == [0, 0, 0]
        if k > 3:
            assert idx[0, 3] == PASS + 4000 + 7 and dist[0, 3] == 0
        assert idx[1, :3].tolist() == [5 + 7, PASS - 1 + 7, PASS + 7] and dist[1, :3].tolist() == [1, 1, 1]
    assert gpu_ctx.state_dirty() == 0


def test_merge_of_partial_tables(gpu_ctx):
    rng = np.random.default_rng(12)
    n, parts = 1000, [300, 1, 2000, 700]
    q = rand_desc(rng, n)
    ts = [rand_desc(rng, m) for m in parts]
    ts[2][50] = ts[0][10]                                           # a tie between two parts
    q[3] = ts[0][10]
    cat = np.concatenate(ts)
    offs = np.r_[0, np.cumsum(parts)[:-1]]
    for k in (1, 4, 9, 32):
        pi = np.stack([np.where(i >= 0, i + o, -1) for (i, _), o in ((oracle.bf_knn_c(q, t, k), o) for t, o in zip(ts, offs))])
        pd = np.stack([oracle.bf_knn_c(q, t, k)[1] for t in ts])
        d_pi, d_pd = gpu_ctx.upload(np.ascontiguousarray(pi, np.int32)), gpu_ctx.upload(np.ascontiguousarray(pd, np.int32))
        tab = Tables(gpu_ctx, n, k)
        try:
            rc = gpu_ctx.lib.slam_bf_merge_topk(gpu_ctx.handle, d_pi.ptr, d_pd.ptr, len(ts), n, k, tab.idx.ptr, tab.dist.ptr)
            assert rc == 0
            idx, dist = tab.download()
        finally:
            for o in (tab, d_pi, d_pd):
                o.free()
        assert_oracle(q, cat, k, idx, dist, f"merge k={k}")


def test_collection_and_keyframe_database(gpu_ctx):
    import slamhip

    rng = np.random.default_rng(13)
    imgs = [rand_desc(rng, r) for r in (500, 0, 1200, 37, 2048)]
    imgs[2][100] = imgs[0][7]
    q = rand_desc(rng, 700)
    q[0] = imgs[0][7]
    db = slamhip.KeyframeDatabase(gpu_ctx, capacity_rows=1024)
    try:
        for im in imgs:
            db.add(im)
        for k in (3, 5, 16, 32):
            want = oracle.bf_knn_multi_c(q, imgs, k, threads=16)
            got = slamhip.topk_match_collection(q, imgs, k, ctx=gpu_ctx)
            got_db = db.query_topk(q, k)
            for w, g, d in zip(want, got, got_db):
                assert np.array_equal(w, g) and np.array_equal(w, d), k
        # the top-2 query on the same database still answers as before, after top-k queries grew its buffer
        want = oracle.bf_knn_multi_c(q, imgs, 2, threads=16)
        assert all(np.array_equal(w, g) for w, g in zip(want, db.query(q, 2)))
        assert db.query_topk(q[:0], 4)[0].shape == (0, 4)
    finally:
        db.free()
    assert gpu_ctx.state_dirty() == 0


def test_feature_matcher_knn_match_k5(gpu_ctx):
    from feature_matchers import BruteForceFeatureMatcher

    rng = np.random.default_rng(14)
    q, t = rand_desc(rng, 333), rand_desc(rng, 1234)
    t[9] = t[1000]
    q[2] = t[9]
    ridx, rdist = oracle.bf_knn_c(q, t, 5, threads=16)
    lists = BruteForceFeatureMatcher(norm_type=6).knn_match(q, t, k=5)
    assert len(lists) == 333
    for i, row in enumerate(lists):
        assert [m.trainIdx for m in row] == ridx[i].tolist()
        assert [m.distance for m in row] == rdist[i].tolist()
        assert all(m.queryIdx == i for m in row)
    short = BruteForceFeatureMatcher(norm_type=6).knn_match(q, t[:3], k=5)      # fewer train rows than k: up to k matches
    assert all(len(row) == 3 for row in short)
    two = BruteForceFeatureMatcher(norm_type=6).knn_match(q, t, k=2)            # k = 2 keeps the top-2 path
    assert [[m.trainIdx for m in row] for row in two] == ridx[:, :2].tolist()


def test_k2_equals_the_top2_search(gpu_ctx):
    import slamhip

    rng = np.random.default_rng(15)
    for n, m in [(1, 5), (77, 300), (512, 4096), (3000, 20000), (257, 70000), (4096, 4096)]:
        q, t = rand_desc(rng, n), rand_desc(rng, m)
        t[m // 3] = t[m // 2]
        q[0] = t[m // 2]
        dq, dt = slamhip.DeviceDescriptors(gpu_ctx, q), slamhip.DeviceDescriptors(gpu_ctx, t)
        a, b = Tables(gpu_ctx, n, 2), slamhip.Top2Table(gpu_ctx, n)
        try:
            slamhip.knn_topk_device(gpu_ctx, dq.buf, n, dt.buf, m, 2, a.idx, a.dist)
            slamhip.knn2_device(gpu_ctx, dq.buf, n, dt.buf, m, b.idx, b.dist)
            (ia, da), (ib, db_) = a.download(), b.download()
        finally:
            for o in (a, b, dq, dt):
                o.free()
        assert np.array_equal(ia, ib) and np.array_equal(da, db_), (n, m)
        assert gpu_ctx.state_dirty() == 0


def test_interleaved_topk_and_top2_on_one_context(gpu_ctx):
    import slamhip

    rng = np.random.default_rng(16)
    q, t = rand_desc(rng, 2000), rand_desc(rng, 30000)
    alone_k = device_topk(gpu_ctx, q, t, 9)
    alone_2 = slamhip.knn_match_arrays(q, t, 2, ctx=gpu_ctx)
    dq, dt = slamhip.DeviceDescriptors(gpu_ctx, q), slamhip.DeviceDescriptors(gpu_ctx, t)
    tk, t2 = Tables(gpu_ctx, 2000, 9), slamhip.Top2Table(gpu_ctx, 2000)
    try:
        for _ in range(3):                                          # queued back to back, no wait in between
            slamhip.knn_topk_device(gpu_ctx, dq.buf, 2000, dt.buf, 30000, 9, tk.idx, tk.dist)
            slamhip.knn2_device(gpu_ctx, dq.buf, 2000, dt.buf, 30000, t2.idx, t2.dist)
        got_k, got_2 = tk.download(), t2.download()
    finally:
        for o in (tk, t2, dq, dt):
            o.free()
    assert all(np.array_equal(a, b) for a, b in zip(alone_k, got_k))
    assert all(np.array_equal(a, b) for a, b in zip(alone_2, got_2))
    assert gpu_ctx.state_dirty() == 0


def test_argument_errors(gpu_ctx):
    from slamhip import _lib

    lib, ctx = gpu_ctx.lib, gpu_ctx
    q = ctx.upload(np.zeros((8, 32), np.uint8))
    out = ctx.malloc(8 * 33 * 4)
    h = ctx.handle
    for k in (0, 33, -1):
        assert lib.slam_bf_knn_u256(h, q.ptr, 4, q.ptr, 8, 0, k, out.ptr, out.ptr) == _lib.SLAM_ERR_INVALID
        assert lib.slam_bf_knn_u256(h, q.ptr, 0, q.ptr, 8, 0, k, out.ptr, out.ptr) == _lib.SLAM_ERR_INVALID   # even with no rows
        assert lib.slam_bf_merge_topk(h, out.ptr, out.ptr, 1, 4, k, out.ptr, out.ptr) == _lib.SLAM_ERR_INVALID
    assert lib.slam_bf_knn_u256(h, q.ptr + 4, 4, q.ptr, 8, 0, 4, out.ptr, out.ptr) == _lib.SLAM_ERR_INVALID     # misaligned query
    assert b"16-byte aligned" in lib.slam_last_error()
    assert lib.slam_bf_knn_u256(h, q.ptr, 4, q.ptr + 8, 4, 0, 4, out.ptr, out.ptr) == _lib.SLAM_ERR_INVALID     # misaligned train
    assert lib.slam_bf_knn_u256(h, q.ptr, 4, q.ptr, 8, 0, 4, out.ptr + 2, out.ptr) == _lib.SLAM_ERR_INVALID     # misaligned idx
    assert lib.slam_bf_knn_u256(h, q.ptr, 4, q.ptr, 8, 0, 4, out.ptr, out.ptr + 1) == _lib.SLAM_ERR_INVALID     # misaligned dist
    assert lib.slam_bf_merge_topk(h, out.ptr + 2, out.ptr, 1, 4, 4, out.ptr, out.ptr) == _lib.SLAM_ERR_INVALID
    assert lib.slam_bf_knn_u256(h, q.ptr, -1, q.ptr, 8, 0, 4, out.ptr, out.ptr) == _lib.SLAM_ERR_INVALID
    assert lib.slam_bf_knn_u256(h, q.ptr, 4, q.ptr, 8, 0, 4, None, out.ptr) == _lib.SLAM_ERR_INVALID
    assert lib.slam_bf_knn_u256(h, q.ptr, 4, q.ptr, 8, 2**31 - 4, 4, out.ptr, out.ptr) == _lib.SLAM_ERR_INVALID
    assert lib.slam_bf_merge_topk(h, out.ptr, out.ptr, 0, 4, 4, out.ptr, out.ptr) == _lib.SLAM_ERR_INVALID
    hq = np.zeros((4, 32), np.uint8)
    hi = np.zeros((4, 33), np.int32)
    for k in (0, 33):
        assert lib.slam_bf_knn_u256_host(h, _lib.addr(hq), 4, _lib.addr(hq), 4, k, _lib.addr(hi), _lib.addr(hi)) == _lib.SLAM_ERR_INVALID
    for o in (q, out):
        o.free()
    assert gpu_ctx.state_dirty() == 0


def test_known_answers_on_every_entry_point(gpu_ctx):
    import slamhip
    from feature_matchers import BruteForceFeatureMatcher

    with open(os.path.join(ROOT, "tests", "golden", "kat_topk.json")) as f:
        kat = json.load(f)
    bf = BruteForceFeatureMatcher(norm_type=6)
    for c in kat["cases"]:
        k, name = c["k"], c["name"]
        t = np.array(kat["trains"][c["train"]], np.uint8).reshape(-1, 32)
        q = np.array(c["query"], np.uint8).reshape(-1, 32)
        idx, dist = slamhip.topk_match_arrays(q, t, k, ctx=gpu_ctx)
        assert idx.tolist() == c["idx"] and dist.tolist() == c["dist"], name
        idx, dist = device_topk(gpu_ctx, q, t, k)
        assert idx.tolist() == c["idx"] and dist.tolist() == c["dist"], name
        img, local, dist = slamhip.topk_match_collection(q, [t], k, ctx=gpu_ctx)
        assert local.tolist() == c["idx"] and dist.tolist() == c["dist"], name
        db = slamhip.KeyframeDatabase(gpu_ctx)
        try:
            db.add(t)
            img, local, dist = db.query_topk(q, k)
            assert local.tolist() == c["idx"] and dist.tolist() == c["dist"], name
        finally:
            db.free()
        # two partial tables that each hold the full answer merge to it again (ties between equal keys resolve to one copy)
        pi = np.ascontiguousarray(np.stack([c["idx"], [[NO_IDX] * k] * len(c["idx"])]), np.int32)
        pd = np.ascontiguousarray(np.stack([c["dist"], [[NO_DIST] * k] * len(c["dist"])]), np.int32)
        d_pi, d_pd = gpu_ctx.upload(pi), gpu_ctx.upload(pd)
        tab = Tables(gpu_ctx, q.shape[0], k)
        try:
            assert gpu_ctx.lib.slam_bf_merge_topk(gpu_ctx.handle, d_pi.ptr, d_pd.ptr, 2, q.shape[0], k, tab.idx.ptr, tab.dist.ptr) == 0
            idx, dist = tab.download()
        finally:
            for o in (tab, d_pi, d_pd):
                o.free()
        assert idx.tolist() == c["idx"] and dist.tolist() == c["dist"], name
        if k >= 3:
            rows = bf.knn_match(q, t, k)
            assert [[m.trainIdx for m in r] for r in rows] == [[i for i in r if i >= 0] for r in c["idx"]], name
    assert gpu_ctx.state_dirty() == 0
