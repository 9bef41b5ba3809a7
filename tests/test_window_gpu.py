"""GPU suite for the window-constrained top-2 search (bf_window.hip, knnMatch with a geometric mask): bit-exact results
against a restatement written here (oracle.hamming_matrix_np + the float32 window mask + a stable (distance, index) top-k),
on the host and the device paths, over fuzzed shapes and the edges of the window rule, and the overlay's match_in_windows."""
import numpy as np
import pytest

from hamming_families import ref_window
from oracle import oracle

pytestmark = pytest.mark.gpu

NONE_IDX, NONE_DIST = -1, np.iinfo(np.int32).max


def rand_desc(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def run_device(ctx, q, t, qxy, txy, radius, k, cells=0):
    import slamhip

    n, m = q.shape[0], t.shape[0]
    dq, dt = slamhip.DeviceDescriptors(ctx, q), slamhip.DeviceDescriptors(ctx, t)
    bufs = [ctx.malloc(max(n, 1) * 8), ctx.malloc(max(m, 1) * 8), ctx.malloc(max(n, 1) * 4 * k), ctx.malloc(max(n, 1) * 4 * k)]
    try:
        if n:
            bufs[0].upload(np.ascontiguousarray(qxy, np.float32))
        if m:
            bufs[1].upload(np.ascontiguousarray(txy, np.float32))
        rad = radius
        if np.ndim(radius) == 1:
            rad = ctx.malloc(max(m, 1) * 4)
            bufs.append(rad)
            if m:
                rad.upload(np.ascontiguousarray(radius, np.float32))
        slamhip.window_knn_device(ctx, dq.buf, n, dt.buf, m, bufs[0], bufs[1], rad, k, bufs[2], bufs[3], cells=cells)
        if n == 0:
            return np.zeros((0, k), np.int32), np.zeros((0, k), np.int32)
        return bufs[2].download(np.int32, (n, k)), bufs[3].download(np.int32, (n, k))
    finally:
        for b in bufs + [dq, dt]:
            b.free()


def check_both(ctx, q, t, qxy, txy, radius, k, rows=None, what=""):
    import slamhip

    want = ref_window(q, t, qxy, txy, radius, k, rows)
    sel = slice(None) if rows is None else rows
    for name, (idx, dist) in (("host", slamhip.window_match_arrays(q, t, qxy, txy, radius, k)),
                              ("device", run_device(ctx, q, t, qxy, txy, radius, k))):
        assert idx.shape == (q.shape[0], k) and idx.dtype == np.int32 and dist.dtype == np.int32, (what, name)
        gi, gd = idx[sel], dist[sel]
        bad = np.nonzero((gi != want[0]).any(1) | (gd != want[1]).any(1))[0]
        assert bad.size == 0, (f"{what} {name}: {bad.size} rows differ, first {bad[0]}: {gi[bad[0]]} {gd[bad[0]]} "
                               f"vs {want[0][bad[0]]} {want[1][bad[0]]}")
    return want


FUZZ = [(1, 1), (1, 7), (5, 1), (64, 64), (65, 300), (600, 600), (1000, 5000), (4096, 4096), (3000, 20000), (8192, 65536)]


@pytest.mark.parametrize("n,m", FUZZ)
@pytest.mark.parametrize("k", [1, 2])
def test_fuzzed_shapes(gpu_ctx, n, m, k):
    rng = np.random.default_rng(7 * n + 13 * m + k)
    plane = float(rng.choice([64.0, 640.0, 4096.0]))
    q, t = rand_desc(rng, n), rand_desc(rng, m)
    qxy = rng.uniform(0, plane, (n, 2)).astype(np.float32)
    txy = rng.uniform(0, plane, (m, 2)).astype(np.float32)
    radius = float(rng.choice([2.0, 16.0, 50.0]))
    rows = None if n * m <= 4096 * 20000 else np.sort(rng.choice(n, 1024, replace=False))
    check_both(gpu_ctx, q, t, qxy, txy, radius, k, rows, f"{n}x{m}")


def test_points_exactly_at_the_window_edge(gpu_ctx):
    rng = np.random.default_rng(1)
    m = 400
    t = rand_desc(rng, m)
    txy = (rng.integers(0, 200, (m, 2)) * 0.25).astype(np.float32)    # multiples of 1/4: every difference below is exact
    r = np.float32(2.5)
    offs = np.array([[r, 0], [-r, 0], [0, r], [0, -r], [r, r], [-r, -r], [r, -r], [r + 0.25, 0], [0, -r - 0.25]], np.float32)
    owner = np.repeat(np.arange(m), len(offs))
    qxy = (txy[owner] + np.tile(offs, (m, 1))).astype(np.float32)
    q = t[owner].copy()                                              # distance 0 to the row whose edge it sits on
    assert np.array_equal(np.abs(qxy - txy[owner]), np.abs(np.tile(offs, (m, 1))))
    idx, dist = check_both(gpu_ctx, q, t, qxy, txy, float(r), 2)
    on_edge = np.tile(np.arange(len(offs)) < 7, m)
    assert np.all(idx[on_edge, 0] == owner[on_edge]) and np.all(dist[on_edge, 0] == 0)
    assert np.all(idx[~on_edge, 0] != owner[~on_edge])


def test_empty_windows(gpu_ctx):
    rng = np.random.default_rng(2)
    q, t = rand_desc(rng, 300), rand_desc(rng, 500)
    txy = rng.uniform(0, 100, (500, 2)).astype(np.float32)
    qxy = rng.uniform(0, 100, (300, 2)).astype(np.float32)
    qxy[::2] += 1000.0                                               # every other query far from every window
    idx, dist = check_both(gpu_ctx, q, t, qxy, txy, 5.0, 2)
    assert np.all(idx[::2] == NONE_IDX) and np.all(dist[::2] == NONE_DIST)


def test_every_point_in_one_cell(gpu_ctx):
    rng = np.random.default_rng(3)
    n, m = 3000, 9000
    q, t = rand_desc(rng, n), rand_desc(rng, m)
    txy = (100.0 + rng.uniform(-0.5, 0.5, (m, 2))).astype(np.float32)
    qxy = (100.0 + rng.uniform(-1.5, 1.5, (n, 2))).astype(np.float32)
    check_both(gpu_ctx, q, t, qxy, txy, 1.0, 2)


def test_skewed_dense_and_empty_cells(gpu_ctx):
    rng = np.random.default_rng(4)
    hot, cold = 6000, 4000
    t = rand_desc(rng, hot + cold)
    txy = np.concatenate([rng.normal(300.0, 2.0, (hot, 2)), rng.uniform(0, 2000, (cold, 2))]).astype(np.float32)
    perm = rng.permutation(hot + cold)
    t, txy = t[perm], txy[perm]
    n = 5000
    q = rand_desc(rng, n)
    qxy = np.concatenate([rng.normal(300.0, 4.0, (n // 2, 2)), rng.uniform(0, 2000, (n - n // 2, 2))]).astype(np.float32)
    check_both(gpu_ctx, q, t, qxy, txy, 8.0, 2)
    check_both(gpu_ctx, q, t, qxy, txy, rng.uniform(1.0, 12.0, hot + cold).astype(np.float32), 2)


def test_duplicates_at_equal_distance_lower_index_wins(gpu_ctx):
    rng = np.random.default_rng(5)
    q, t = rand_desc(rng, 50), rand_desc(rng, 1000)
    txy = rng.uniform(0, 50, (1000, 2)).astype(np.float32)
    qxy = rng.uniform(0, 50, (50, 2)).astype(np.float32)
    t[5] = t[900] = t[901] = q[10]
    txy[5] = txy[900] = txy[901] = qxy[10]
    idx, dist = check_both(gpu_ctx, q, t, qxy, txy, 3.0, 2)
    assert idx[10].tolist() == [5, 900] and dist[10].tolist() == [0, 0]


def test_nan_negative_and_per_row_radii(gpu_ctx):
    rng = np.random.default_rng(6)
    n, m = 700, 1500
    q, t = rand_desc(rng, n), rand_desc(rng, m)
    txy = rng.uniform(0, 300, (m, 2)).astype(np.float32)
    qxy = rng.uniform(0, 300, (n, 2)).astype(np.float32)
    r = rng.uniform(0, 40, m).astype(np.float32)
    r[::7] = np.nan
    r[1::7] = -3.0
    r[2::7] = -0.0                                                   # not negative: keeps exact positions
    r[3::11] = 0.0
    txy[4::13, 0] = np.nan
    txy[5::13, 1] = np.inf
    qxy[::17, 1] = np.nan
    qxy[1::19, 0] = -np.inf
    qxy[9] = txy[2 * 7 + 2]                                          # exactly on a -0.0 centre
    idx, _ = check_both(gpu_ctx, q, t, qxy, txy, r, 2)
    assert np.all(idx[::17] == NONE_IDX)
    bad = np.nonzero(np.isnan(r) | (r < 0))[0]
    assert not np.isin(idx, bad).any()
    for scalar in (np.nan, -1.0, -0.0):
        idx, dist = check_both(gpu_ctx, q, t, qxy, txy, scalar, 2)
        if scalar != 0:
            assert np.all(idx == NONE_IDX) and np.all(dist == NONE_DIST)


def test_outside_the_plane_and_negative_coordinates(gpu_ctx):
    rng = np.random.default_rng(8)
    n, m = 2000, 3000
    q, t = rand_desc(rng, n), rand_desc(rng, m)
    txy = rng.uniform(-200, 100, (m, 2)).astype(np.float32)
    qxy = rng.uniform(-260, 160, (n, 2)).astype(np.float32)
    qxy[:20] = [[-1e30, 0]] * 10 + [[5e4, 5e4]] * 10
    check_both(gpu_ctx, q, t, qxy, txy, 12.0, 2)
    check_both(gpu_ctx, q, t, qxy, txy, rng.uniform(0, 30, m).astype(np.float32), 1)


@pytest.mark.parametrize("k", [1, 2])
def test_infinite_radius_equals_knn(gpu_ctx, k):
    import slamhip

    rng = np.random.default_rng(9 + k)
    for n, m in ((1, 1), (300, 2000), (2048, 20000)):
        q, t = rand_desc(rng, n), rand_desc(rng, m)
        t[m // 2] = t[0]
        qxy = rng.uniform(-1e6, 1e6, (n, 2)).astype(np.float32)
        txy = rng.uniform(0, 10, (m, 2)).astype(np.float32)
        want = slamhip.knn_match_arrays(q, t, k)
        for got in (slamhip.window_match_arrays(q, t, qxy, txy, np.inf, k), run_device(gpu_ctx, q, t, qxy, txy, np.inf, k),
                    slamhip.window_match_arrays(q, t, qxy, txy, np.full(m, np.inf, np.float32), k)):
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (n, m)


def test_tiny_sides(gpu_ctx):
    import slamhip

    rng = np.random.default_rng(10)
    q, t = rand_desc(rng, 40), rand_desc(rng, 1)
    qxy = rng.uniform(0, 10, (40, 2)).astype(np.float32)
    txy = np.array([[5.0, 5.0]], np.float32)
    check_both(gpu_ctx, q, t, qxy, txy, 3.0, 2)
    for k in (1, 2):
        idx, dist = slamhip.window_match_arrays(q, np.zeros((0, 32), np.uint8), qxy, np.zeros((0, 2), np.float32), 3.0, k)
        assert idx.shape == (40, k) and np.all(idx == NONE_IDX) and np.all(dist == NONE_DIST)
        idx, dist = run_device(gpu_ctx, q, np.zeros((0, 32), np.uint8), qxy, np.zeros((0, 2), np.float32), 3.0, k)
        assert np.all(idx == NONE_IDX) and np.all(dist == NONE_DIST)
        idx, dist = slamhip.window_match_arrays(np.zeros((0,)), t, np.zeros((0, 2)), txy, 3.0, k)
        assert idx.shape == (0, k) and dist.shape == (0, k)
        idx, _ = run_device(gpu_ctx, np.zeros((0, 32), np.uint8), t, np.zeros((0, 2), np.float32), txy, 3.0, k)
        assert idx.shape == (0, k)


def test_deterministic_whatever_the_grid(gpu_ctx):
    import slamhip

    rng = np.random.default_rng(11)
    n, m = 6000, 30000
    q, t = rand_desc(rng, n), rand_desc(rng, m)
    t[100:2100] = t[0]                                               # many equal keys but for the index
    txy = rng.uniform(0, 1000, (m, 2)).astype(np.float32)
    qxy = rng.uniform(0, 1000, (n, 2)).astype(np.float32)
    first = slamhip.window_match_arrays(q, t, qxy, txy, 20.0, 2)
    for cells in (0, 0, 1, 4, 37, 1 << 20):
        got = slamhip.window_match_arrays(q, t, qxy, txy, 20.0, 2, cells=cells)
        assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1]), cells
    rows = np.arange(0, n, 7)
    want = ref_window(q, t, qxy, txy, 20.0, 2, rows)
    assert np.array_equal(first[0][rows], want[0]) and np.array_equal(first[1][rows], want[1])


@pytest.mark.parametrize("radius", [8.0, 32.0, 100.0])
def test_golden_image_descriptors(gpu_ctx, radius):
    import os

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_descriptors.npz"))
    q, t, qxy, txy = g["desc2"], g["desc1"], g["kp2"], g["kp1"]
    for k in (1, 2):
        check_both(gpu_ctx, q, t, qxy, txy, radius, k, what=f"golden r={radius}")


def test_large_plane(gpu_ctx):
    import slamhip

    rng = np.random.default_rng(12)
    n = m = 65536
    q, t = rand_desc(rng, n), rand_desc(rng, m)
    qxy = rng.uniform(0, 4096, (n, 2)).astype(np.float32)
    txy = rng.uniform(0, 4096, (m, 2)).astype(np.float32)
    idx, dist = slamhip.window_match_arrays(q, t, qxy, txy, 16.0, 2)
    rows = np.sort(rng.choice(n, 2048, replace=False))
    want = ref_window(q, t, qxy, txy, 16.0, 2, rows)
    assert np.array_equal(idx[rows], want[0]) and np.array_equal(dist[rows], want[1])
    assert (idx[:, 0] >= 0).mean() > 0.5                             # (a query has a few candidates on average)


@pytest.mark.parametrize("thr", [None, 0, 20.0, 64.0])
def test_match_in_windows(gpu_ctx, thr):
    from feature_matchers import BruteForceFeatureMatcher, MatchList

    g = np.load(__import__("os").path.join(__import__("os").path.dirname(__file__), "golden", "image_descriptors.npz"))
    src, cur, sxy, cxy = g["desc1"], g["desc2"], g["kp1"], g["kp2"]
    bf = BruteForceFeatureMatcher(6)
    for radius in (32.0, np.linspace(4, 60, len(src)).astype(np.float32)):
        got = bf.match_in_windows(src, cur, sxy, cxy, radius, thr)
        assert isinstance(got, MatchList)
        idx, dist = ref_window(cur, src, cxy, sxy, radius, 1)
        qi = np.flatnonzero(idx[:, 0] >= 0)
        d = dist[qi, 0]
        if thr and qi.size:
            keep = d < max(2 * d.min(), thr)                          # feature_matchers.py:41-43
            qi, d = qi[keep], d[keep]
        assert got.queryIdx.tolist() == qi.tolist()
        assert got.trainIdx.tolist() == idx[qi, 0].tolist()
        assert got.distance.tolist() == d.astype(np.float32).tolist()
        assert [m.queryIdx for m in got] == qi.tolist()
    empty = bf.match_in_windows(src, np.zeros((0,)), sxy, np.zeros((0, 2)), 10.0)
    assert len(empty) == 0
