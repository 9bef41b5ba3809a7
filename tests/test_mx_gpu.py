"""GPU: the matrix-core top-2 search (bf_mx.hip: a +-1 FP4 dot product on the MFMA units) must give the VALU kernel's and the
oracle's tables bit for bit - every distance 0..256, ragged shapes, ties across chunk boundaries, the fused selection, the
kept query rows, a train_base - and leave the merge state idle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


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


def _match_host(ctx, q, d_train, m, keep_query):
    """One slam_bf_match_host call: host query rows, device train rows, query rows kept at keep_query, every match kept."""
    import ctypes

    from slamhip._lib import check

    n = len(q)
    q = np.ascontiguousarray(q)
    qi, ti, dist = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.float32)
    cnt = ctypes.c_int64(0)
    check(ctx.lib.slam_bf_match_host(ctx.handle, q.ctypes.data, n, None, d_train.ptr, m, keep_query.ptr, 0, 0.0,
                                     qi.ctypes.data, ti.ctypes.data, dist.ctypes.data, ctypes.byref(cnt)))
    c = cnt.value
    return qi[:c], ti[:c], dist[:c]


def _flip(row, bits):
    out = np.unpackbits(row).copy()
    out[bits] ^= 1
    return np.packbits(out)


def test_every_distance_is_exact(gpu_ctx):
    """Planted pairs at every distance 0..256 on asymmetric data: a wrong lane, nibble or K map cannot survive this."""
    from oracle import oracle

    rng = np.random.default_rng(4242)
    n, m = 257, 16411
    q = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    q[:, :4] = 0xF0                                          # asymmetric bytes: a transposed or permuted operand changes the dots
    for d in range(257):
        row = (97 * d + 13) % m
        t[row] = _flip(q[d], rng.permutation(256)[:d])
    ridx, rdist = oracle.bf_knn_c(q, t, 2, threads=8)
    idx, dist = _search(gpu_ctx, q, t, 2)
    assert np.array_equal(idx, ridx) and np.array_equal(dist, rdist)
    for d in range(0, 257, 16):                             # the planted row is found wherever it is the nearest
        if rdist[d, 0] == d and d < 60:
            assert idx[d, 0] == (97 * d + 13) % m


@pytest.mark.parametrize("n,m", [(1, 16384), (255, 1000), (257, 769), (1000, 5001), (3001, 16400), (5000, 20000), (700, 70001)])
def test_ragged_shapes_against_the_oracle(gpu_ctx, n, m):
    import slamhip
    from oracle import oracle

    rng = np.random.default_rng(n * 31 + m)
    q = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    # ties across chunk boundaries: one row copied to both sides of every boundary of the MX plan, and queries equal to it
    _, tbl = slamhip.mx_plan_describe(n, m, num_cu=gpu_ctx.plan_info(n, m)["cus"])
    for b in tbl[1:-1][:64]:
        t[b - 1] = t[7]
        t[b] = t[7]
    t[m - 1] = t[7]
    q[0] = t[7]
    ridx, rdist = oracle.bf_knn_c(q, t, 2, threads=8)
    for engine in (2, 0):
        idx, dist = _search(gpu_ctx, q, t, engine)
        assert np.array_equal(idx, ridx) and np.array_equal(dist, rdist), (engine, n, m)


def test_full_grid_engines_agree(gpu_ctx):
    rng = np.random.default_rng(65536)
    q = rng.integers(0, 256, (65536, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (65536, 32), dtype=np.uint8)
    t[40000] = t[3]
    q[9] = t[3]
    a = _search(gpu_ctx, q, t, 1)
    b = _search(gpu_ctx, q, t, 2)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert b[0][9].tolist() == [3, 40000]


def test_select_keep_and_train_base(gpu_ctx):
    import slamhip

    ctx = gpu_ctx
    rng = np.random.default_rng(77)
    n, m, base = 3000, 20000, 123456
    q = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    t[5000] = q[17]
    res = {}
    for engine in (1, 2):
        ctx.set_engine(engine)
        dq, dt = slamhip.DeviceDescriptors(ctx, q), slamhip.DeviceDescriptors(ctx, t)
        tab = slamhip.Top2Table(ctx, n)
        keep = ctx.malloc(n)
        try:
            out = {}
            for mode in (0, 2):
                cnt = slamhip.knn2_select_device(ctx, dq.buf, n, dt.buf, m, tab.idx, tab.dist, keep, mode=mode, param=0.8,
                                                 train_base=base)
                out[mode] = (cnt, keep.download(np.uint8, (n,))) + tab.download()
            # slam_bf_match_host (BruteForceFeatureMatcher.match's one-call form) with the train rows already on the device and
            # the query rows left in device memory for the next frame; mode 0 = no distance filter
            kq = ctx.malloc(32 * n)
            qi, ti, di = _match_host(ctx, q, dt.buf, m, kq)
            out["host"] = (qi, ti, di, kq.download(np.uint8, (n, 32)))
            kq.free()
        finally:
            ctx.set_engine(0)
            for o in (tab, dq, dt, keep):
                o.free()
        assert ctx.state_dirty() == 0
        res[engine] = out
    for key in (0, 2, "host"):
        for x, y in zip(res[1][key], res[2][key]):
            assert np.array_equal(np.asarray(x), np.asarray(y)), key
    assert res[2][0][2][17, 0] == base + 5000 and res[2][0][3][17, 0] == 0
    assert np.array_equal(res[2]["host"][3], q)
