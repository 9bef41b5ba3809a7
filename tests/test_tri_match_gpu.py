"""The epipolar node search and new-map-point creation on the device: slam_tri_match_search against the numpy
reference and slam_tri_match_triangulate against the host twin of csrc/tri_point.h, bit for bit - matches, counts and every
table - over the shapes at which the scan can go wrong, the semantics of every gate, stability, the chain into PointSets and
search_by_projection, and the argument checks."""
import ctypes

import numpy as np
import pytest

import tri_match_cases as C
import tri_match_ref as R
import tri_match_twin as TW
from hamming_families import prefix_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tm(gpu_ctx):
    from slamhip import tri_match as module
    return module


def cat(images, key, dtype, tail=()):
    parts = [np.asarray(s[key], dtype).reshape((-1,) + tail) for s in images]
    return np.concatenate(parts) if parts else np.zeros((0,) + tail, dtype)


def make_set(tm, ctx, images):
    """(FeatureVectors, KeyframeViews, bins or None) of a list of image dicts."""
    from slamhip import FeatureVectors
    off = np.concatenate([[0], np.cumsum([len(s["nodes"]) for s in images])]).astype(np.int64)
    fv = FeatureVectors.from_nodes(cat(images, "desc", np.uint8, (32,)), cat(images, "nodes", np.int64), off, ctx=ctx)
    taken = cat([dict(taken=s.get("taken", np.zeros(len(s["nodes"]), np.uint8))) for s in images], "taken", np.uint8)
    views = tm.KeyframeViews(cat(images, "xy", np.float32, (2,)), cat(images, "level", np.int64), taken if any("taken" in s for s in images) else None,
                             ctx)
    bins = cat(images, "bins", np.int64) if all("bins" in s for s in images) and images else None
    return fv, views, bins


def run(tm, ctx, images1, images2, pairs, F=C.F_RECT, epipole=C.EPIPOLE_RECT, scan_order=0, **kw):
    P = len(pairs)
    F = np.broadcast_to(np.asarray(F, np.float64), (P, 3, 3)) if np.ndim(F) == 2 else np.asarray(F, np.float64)
    E = np.broadcast_to(np.asarray(epipole, np.float64), (P, 2)) if np.ndim(epipole) == 1 else np.asarray(epipole, np.float64)
    f1, v1, b1 = make_set(tm, ctx, images1)
    f2, v2, b2 = make_set(tm, ctx, images2)
    try:
        if b1 is None or b2 is None:
            b1 = b2 = None
        got = tm.search_for_triangulation(f1, f2, pairs, v1, v2, F, E, (C.SCALE, C.SIGMA2), b1, b2, return_tables=True, ctx=ctx,
                                          scan_order=scan_order, **kw)
    finally:
        for x in (f1, v1, f2, v2):
            x.free()
    return got, F, E


def check(tm, ctx, images1, images2, pairs, **kw):
    """The device against the reference for every pair: matches, counts and both tables, bit for bit."""
    (m, c, tabs), F, E = run(tm, ctx, images1, images2, pairs, **kw)
    rkw = {k: v for k, v in kw.items() if k in ("th_low", "chi2", "epipole_r2")}
    for p, (a, b) in enumerate(pairs):
        s1, s2 = dict(images1[a]), dict(images2[b])
        if not ("bins" in s1 and "bins" in s2 and all("bins" in s for s in images1) and all("bins" in s for s in images2)):
            s1.pop("bins", None)
        want, count, (idx, dist) = R.search(s1, s2, F[p], E[p], C.SCALE, C.SIGMA2, **rkw)
        assert np.array_equal(tabs[p][0], idx) and np.array_equal(tabs[p][1], dist), f"pair {p}: the top-2 tables differ"
        assert np.array_equal(m[p], want) and c[p] == count, f"pair {p}: the matches differ"
    return m, c, tabs


# ---- shapes ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n1,n2", [(0, 7), (7, 0), (1, 1), (65, 40), (200, 130)])
def test_sizes(tm, gpu_ctx, n1, n2):
    s1, s2 = C.random_pair(100 + n1, n1, n2, n_nodes=3)
    m, c, tabs = check(tm, gpu_ctx, [s1], [s2], [(0, 0)], th_low=80)
    assert len(m[0]) == n1 and (n1 * n2 == 0 or n1 == 1 or c[0] > 0)


def test_one_by_one_matches(tm, gpu_ctx):
    s = dict(desc=prefix_rows([10]), nodes=[3], xy=[[5.0, 6.0]], level=[0])
    m, c, tabs = check(tm, gpu_ctx, [s], [s], [(0, 0)], epipole=C.NO_EPIPOLE)
    assert m[0].tolist() == [0] and c.tolist() == [1] and tabs[0][0].tolist() == [[0, -1]] and tabs[0][1].tolist() == [[0, 2**31 - 1]]


def test_segments_of_1_4_and_5_rows(tm, gpu_ctx):
    """The ends of the four-row walk and its clamp: node k of side 2 holds 1, 4, 5, 8, 9 and 0 rows."""
    rng = np.random.default_rng(7)
    sizes = [1, 4, 5, 8, 9, 0]
    nodes2 = np.repeat(np.arange(6), sizes)
    n2 = len(nodes2)
    pool = rng.integers(0, 256, (1, 32), dtype=np.uint8)
    s1, _ = C.random_pair(8, 66, 1, n_nodes=6, masked=False, taken=False, pool=pool)
    _, s2 = C.random_pair(9, 1, n2, n_nodes=6, masked=False, taken=False, pool=pool)
    s2["nodes"] = rng.permutation(nodes2).astype(np.int32)
    s1["xy"][:, 1] = 3.0
    s2["xy"][:, 1] = 3.0                                      # every row on one line: the segment sizes decide the candidates
    s2["xy"][:, 0] = 10.0
    m, c, tabs = check(tm, gpu_ctx, [s1], [s2], [(0, 0)], th_low=256)
    for k, size in enumerate(sizes):
        have = (tabs[0][0][s1["nodes"] == k] >= 0).sum(1)
        assert (have == min(size, 2)).all()


def test_8192_rows_in_one_node(tm, gpu_ctx):
    s1, s2 = C.random_pair(21, 8192, 8192, n_nodes=1, masked=False, taken=False)
    m, c, tabs = check(tm, gpu_ctx, [s1], [s2], [(0, 0)])
    assert c[0] > 500


def test_three_pairs_one_empty_two_sharing_an_image(tm, gpu_ctx):
    kw = dict(n_nodes=4, bins=True, pool=C.POOL)
    images1 = [C.random_pair(31, 150, 1, **kw)[0], C.random_pair(32, 0, 1, **kw)[0], C.random_pair(33, 70, 1, **kw)[0]]
    images2 = [C.random_pair(34, 1, 90, **kw)[1], C.random_pair(35, 1, 260, **kw)[1]]
    F = np.stack([C.F_RECT, 2.0 * C.F_RECT, C.F_RECT])
    E = np.stack([C.EPIPOLE_RECT, C.NO_EPIPOLE, [100.0, 9.0]])
    pairs = [(0, 1), (1, 0), (2, 1)]
    m, c, _ = check(tm, gpu_ctx, images1, images2, pairs, F=F, epipole=E, th_low=80)
    assert [len(x) for x in m] == [150, 0, 70] and c[1] == 0 and c[0] > 0 and c[2] > 0
    one, cnt, _ = check(tm, gpu_ctx, [images1[2]], [images2[1]], [(0, 0)], F=F[2], epipole=E[2], th_low=80)
    assert np.array_equal(one[0], m[2]) and cnt[0] == c[2]     # rows of different pairs never meet


def test_batch_at_the_pair_limit(tm, gpu_ctx):
    rng = np.random.default_rng(41)
    P = tm.PAIRS_MAX
    images = []
    for _ in range(64):
        s = dict(desc=rng.integers(0, 256, (2, 32), dtype=np.uint8), nodes=np.array([0, 0], np.int32),
                 xy=np.array([[4.0, 3.0], [9.0, 6.0]], np.float32), level=np.zeros(2, np.int32))
        images.append(s)
    pairs = [(int(a), int(b)) for a, b in rng.integers(0, 64, (P, 2))]
    f, v, _ = make_set(tm, gpu_ctx, images)
    try:
        F, E = np.broadcast_to(C.F_RECT, (P, 3, 3)), np.broadcast_to(C.NO_EPIPOLE, (P, 2))
        m, c = tm.search_for_triangulation(f, f, pairs, v, v, F, E, (C.SCALE, C.SIGMA2), th_low=256, ctx=gpu_ctx)
        for p in (0, 1, 2047, 4094, 4095):
            want, count, _ = R.search(images[pairs[p][0]], images[pairs[p][1]], C.F_RECT, C.NO_EPIPOLE, C.SCALE, C.SIGMA2, th_low=256)
            assert np.array_equal(m[p], want) and c[p] == count
        assert (c == 2).all()                                 # row 0 meets row 0 and row 1 row 1: the lines y2 = y1
        with pytest.raises(ValueError):
            tm.search_for_triangulation(f, f, pairs + [(0, 0)], v, v, np.broadcast_to(C.F_RECT, (P + 1, 3, 3)),
                                        np.broadcast_to(C.NO_EPIPOLE, (P + 1, 2)), ctx=gpu_ctx)
        from slamhip._lib import addr
        from slamhip.bow_match import _groups
        g = _groups(f, f.device, None)
        tv = v._struct(gpu_ctx, f.n)
        prm, keep = tm._params(C.CAMERA, None)
        big = np.zeros((P + 1, 2), np.int32)
        bigF, bigE = np.zeros((P + 1, 9)), np.zeros((P + 1, 2))
        out = gpu_ctx.malloc(1 << 16)
        try:
            rc = gpu_ctx.lib.slam_tri_match_search(gpu_ctx.handle, ctypes.byref(g), ctypes.byref(g), ctypes.byref(tv), ctypes.byref(tv), addr(big),
                                                   P + 1, addr(bigF), addr(bigE), ctypes.byref(prm), 0, out.ptr, out.ptr + 32768, None, None)
            assert rc == -1                                   # 4097 pairs: INVALID
        finally:
            out.free()
            del keep
    finally:
        f.free()
        v.free()


# ---- semantics ------------------------------------------------------------------------------------------------------------------

def two_rows(d1, d2, xy1, xy2, level2=None, **extra):
    s1 = dict(desc=prefix_rows(d1), nodes=np.zeros(len(d1), np.int32), xy=np.asarray(xy1, np.float32), level=np.zeros(len(d1), np.int32))
    s2 = dict(desc=prefix_rows(d2), nodes=np.zeros(len(d2), np.int32), xy=np.asarray(xy2, np.float32),
              level=np.zeros(len(d2), np.int32) if level2 is None else np.asarray(level2, np.int32))
    s1.update({k[:-1]: v for k, v in extra.items() if k.endswith("1")})
    s2.update({k[:-1]: v for k, v in extra.items() if k.endswith("2")})
    return s1, s2


def test_the_gate_is_inside_the_search_not_behind_it(tm, gpu_ctx):
    """The nearest descriptor fails the line gate, a farther one passes: the farther is matched.  search_by_bow followed by a
    filter on its match gives no match at all: the nearest hides the one the epipolar line picks."""
    from slamhip import FeatureVectors, search_by_bow
    # side-1 row at y = 30; side 2: distance 1 at y = 60 (off the line), distance 3 at y = 30.5 (on it), distance 2 at y = 90
    s1, s2 = two_rows([100], [101, 103, 102], [[50.0, 30.0]], [[50.0, 60.0], [80.0, 30.5], [20.0, 90.0]])
    m, c, tabs = check(tm, gpu_ctx, [s1], [s2], [(0, 0)], epipole=C.NO_EPIPOLE)
    assert m[0].tolist() == [1] and tabs[0][0].tolist() == [[1, -1]] and tabs[0][1][0, 0] == 3
    f1, f2 = FeatureVectors.from_nodes(s1["desc"], s1["nodes"], ctx=gpu_ctx), FeatureVectors.from_nodes(s2["desc"], s2["nodes"], ctx=gpu_ctx)
    try:
        bow, _, btab = search_by_bow(f1, f2, [(0, 0)], ratio=1e9, return_tables=True, ctx=gpu_ctx)
    finally:
        f1.free()
        f2.free()
    assert bow[0].tolist() == [0]                             # the nearest descriptor ...
    _, on = R.gates(C.F_RECT, C.NO_EPIPOLE, s1["xy"], s2["xy"], s2["level"], C.SCALE, C.SIGMA2)
    assert not on[0, bow[0][0]]                               # ... fails the gate: filtering afterwards leaves nothing
    assert not on[0, btab[0][0][0, 1]]                        # and so does its second neighbour: the top-2 never saw row 1
    assert on[0, 1]


def test_on_the_line_zero_and_nan_f(tm, gpu_ctx):
    s1, s2 = two_rows([100, 50], [100, 50], [[5.0, 30.0], [6.0, 60.0]], [[300.0, 30.0], [7.0, 60.0]])
    m, c, _ = check(tm, gpu_ctx, [s1], [s2], [(0, 0)], epipole=C.NO_EPIPOLE)          # exactly on the line: num = 0
    assert m[0].tolist() == [0, 1]
    nanF = C.F_RECT.copy()
    nanF[0, 0] = np.nan
    for F in (np.zeros((3, 3)), nanF, np.full((3, 3), np.inf)):
        m, c, tabs = check(tm, gpu_ctx, [s1], [s2], [(0, 0)], F=F, epipole=C.NO_EPIPOLE)
        assert (m[0] == -1).all() and c[0] == 0 and (tabs[0][0] == -1).all()
    m, c, _ = check(tm, gpu_ctx, [s1], [s2], [(0, 0)], epipole=C.NO_EPIPOLE, chi2=0.0)  # strict: 0 < 0 passes nothing
    assert c[0] == 0


def test_epipole_gate_by_level(tm, gpu_ctx):
    """The rejected disc grows with the level: its radius is sqrt(100 * scale[l]) = 10 px at level 0 and 13.1 px at level 3.
    The same pixel 12 px from the epipole is kept as a level-0 feature and removed as a level-3 one."""
    e = np.array([100.0, 30.0])
    for level, kept in ((0, True), (3, False)):
        s1, s2 = two_rows([100], [100], [[5.0, 30.0]], [[112.0, 30.0]], level2=[level])
        m, c, _ = check(tm, gpu_ctx, [s1], [s2], [(0, 0)], epipole=e)
        assert (m[0][0] == 0) == kept
        m, c, _ = check(tm, gpu_ctx, [s1], [s2], [(0, 0)], epipole=[np.nan, 30.0])
        assert m[0][0] == 0                                   # a NaN epipole removes none
    s1, s2 = two_rows([100], [100], [[5.0, 30.0]], [[110.0, 30.0]])
    m, _, _ = check(tm, gpu_ctx, [s1], [s2], [(0, 0)], epipole=e)
    assert m[0][0] == 0                                       # at exactly 10 px on level 0: 100 < 100 is false, it stays
    m, _, _ = check(tm, gpu_ctx, [s1], [s2], [(0, 0)], epipole=e, epipole_r2=np.nextafter(100.0, 200.0))
    assert m[0][0] == -1


def test_taken_and_negative_nodes_on_either_side(tm, gpu_ctx):
    xy1, xy2 = [[5.0, 30.0], [6.0, 30.0]], [[7.0, 30.0], [8.0, 30.0]]
    base = lambda: two_rows([100, 60], [101, 61], xy1, xy2)  # noqa: E731
    s1, s2 = base()
    assert check(tm, gpu_ctx, [s1], [s2], [(0, 0)])[0][0].tolist() == [0, 1]
    s1, s2 = base()
    s1["taken"] = np.array([1, 0], np.uint8)
    m, _, tabs = check(tm, gpu_ctx, [s1], [s2], [(0, 0)])
    assert m[0].tolist() == [-1, 1] and tabs[0][0][0].tolist() == [-1, -1]
    s1, s2 = base()
    s2["taken"] = np.array([1, 0], np.uint8)
    m, _, tabs = check(tm, gpu_ctx, [s1], [s2], [(0, 0)])
    assert m[0].tolist() == [-1, 1] and tabs[0][0][0].tolist() == [1, -1]      # row 0 falls to side-2 row 1 (d 39), loses it to row 1
    for side in (0, 1):
        s = base()
        s[side]["nodes"] = np.array([-1, 0], np.int32)
        m, _, _ = check(tm, gpu_ctx, [s[0]], [s[1]], [(0, 0)])
        assert m[0][0] == -1 and m[0][1] == 1
    s1, s2 = base()
    s1["nodes"] = s2["nodes"] = np.array([-5, -5], np.int32)                   # equal negative ids do not match
    assert (check(tm, gpu_ctx, [s1], [s2], [(0, 0)])[0][0] == -1).all()


def test_contested_rows(tm, gpu_ctx):
    xy1 = [[5.0, 30.0], [6.0, 30.0], [7.0, 30.0]]
    s1, s2 = two_rows([103, 101, 102], [100], xy1, [[9.0, 30.0]])
    m, c, _ = check(tm, gpu_ctx, [s1], [s2], [(0, 0)])
    assert m[0].tolist() == [-1, 0, -1] and c[0] == 1          # the smallest d0 keeps it
    s1, s2 = two_rows([102, 98, 102], [100], xy1, [[9.0, 30.0]])
    m, c, _ = check(tm, gpu_ctx, [s1], [s2], [(0, 0)])
    assert m[0].tolist() == [0, -1, -1]                         # equal d0: the lowest side-1 row


def test_rotation_bins_on_and_off(tm, gpu_ctx):
    n = 24
    xy = np.stack([np.arange(n), np.full(n, 30.0)], 1)
    d = list(range(5, 5 + 8 * n, 8))
    bins1 = np.zeros(n, np.uint8)
    bins2 = np.array([0] * 20 + [7, 7, 9, 11], np.uint8)       # 20 matches in bin 0; 2 in bin 25 (10 * 2 >= 20 stays), 1 and 1 (go)
    s1, s2 = two_rows(d, d, xy, xy, bins1=bins1, bins2=bins2)
    m, c, _ = check(tm, gpu_ctx, [s1], [s2], [(0, 0)], th_low=0)
    assert c[0] == 22 and m[0][22:].tolist() == [-1, -1]
    s1.pop("bins")
    m, c, _ = check(tm, gpu_ctx, [s1], [s2], [(0, 0)], th_low=0)
    assert c[0] == n


def test_open_gates_give_node_top2(tm, gpu_ctx):
    from slamhip import FeatureVectors, node_top2
    s1, s2 = C.random_pair(55, 300, 280, n_nodes=5, taken=False)
    (m, c, tabs), _, _ = run(tm, gpu_ctx, [s1], [s2], [(0, 0)], epipole=C.NO_EPIPOLE, chi2=np.inf, th_low=40)
    f1, f2 = FeatureVectors.from_nodes(s1["desc"], s1["nodes"], ctx=gpu_ctx), FeatureVectors.from_nodes(s2["desc"], s2["nodes"], ctx=gpu_ctx)
    try:
        idx, dist = node_top2(f1, f2, [(0, 0)], ctx=gpu_ctx)[0]
    finally:
        f1.free()
        f2.free()
    near = (idx[:, 0] >= 0) & (dist[:, 0] <= 40)
    assert near.sum() > 50 and (~near).sum() > 20
    assert np.array_equal(tabs[0][0][near, 0], idx[near, 0]) and np.array_equal(tabs[0][1][near, 0], dist[near, 0])
    assert (tabs[0][0][~near, 0] == -1).all()


def test_epi_match_arrays_is_the_masked_knn(tm, gpu_ctx):
    s1, s2 = C.random_pair(77, 120, 90, n_nodes=3)
    for k in (1, 2):
        idx, dist = tm.epi_match_arrays(s1["desc"], s2["desc"], s1["nodes"], s2["nodes"], s1["xy"], s2["xy"], s2["level"], C.F_RECT,
                                        C.EPIPOLE_RECT, (C.SCALE, C.SIGMA2), k=k, query_taken=s1["taken"], train_taken=s2["taken"], ctx=gpu_ctx)
        widx, wdist = R.tables(s1, s2, C.F_RECT, C.EPIPOLE_RECT, C.SCALE, C.SIGMA2, th_low=256)
        assert np.array_equal(idx, widx[:, :k]) and np.array_equal(dist, wdist[:, :k])
    assert (widx[:, 1] >= 0).sum() > 10


# ---- stability --------------------------------------------------------------------------------------------------------------------

def test_same_bits_twice_under_both_scan_orders_and_after_search_by_bow(tm, gpu_ctx):
    from slamhip import FeatureVectors, search_by_bow
    kw = dict(n_nodes=7, bins=True, pool=C.POOL)
    images1 = [C.random_pair(61, 500, 1, **kw)[0], C.random_pair(62, 130, 1, **kw)[0]]
    images2 = [C.random_pair(63, 1, 400, **kw)[1]]
    pairs = [(0, 0), (1, 0)]
    first = check(tm, gpu_ctx, images1, images2, pairs, th_low=80)
    # a bow search of larger pairs in between leaves its claim words in the workspace
    big1, big2 = C.random_pair(64, 3000, 3000, n_nodes=3, taken=False)
    f1, f2 = FeatureVectors.from_nodes(big1["desc"], big1["nodes"], ctx=gpu_ctx), FeatureVectors.from_nodes(big2["desc"], big2["nodes"], ctx=gpu_ctx)
    try:
        search_by_bow(f1, f2, [(0, 0)] * 3, th_low=256, ratio=1e9, ctx=gpu_ctx)
    finally:
        f1.free()
        f2.free()
    for order in (0, 1, 0):
        again = check(tm, gpu_ctx, images1, images2, pairs, th_low=80, scan_order=order)
        for p in range(2):
            assert np.array_equal(again[0][p], first[0][p]) and np.array_equal(again[2][p][0], first[2][p][0])
            assert np.array_equal(again[2][p][1], first[2][p][1])
        assert np.array_equal(again[1], first[1])


# ---- B: the geometry ------------------------------------------------------------------------------------------------------------

def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


def tri_check(tm, ctx, xy1, xy2, l1, l2, m12, T1, T2):
    """triangulate_matches for one pair against the twin, bit for bit."""
    from slamhip.proj_match import camera_centres
    n1, n2 = len(xy1), len(xy2)
    s1 = dict(desc=np.zeros((n1, 32), np.uint8), nodes=np.zeros(n1, np.int32), xy=xy1, level=l1)
    s2 = dict(desc=np.zeros((n2, 32), np.uint8), nodes=np.zeros(n2, np.int32), xy=xy2, level=l2)
    f1, v1, _ = make_set(tm, ctx, [s1])
    f2, v2, _ = make_set(tm, ctx, [s2])
    try:
        pts, created = tm.triangulate_matches(f1, f2, [(0, 0)], v1, v2, [m12], T1[None], T2[None], C.CAMERA, (C.SCALE, C.SIGMA2), ctx=ctx)
    finally:
        for x in (f1, v1, f2, v2):
            x.free()
    got = pts[0]
    m12 = np.asarray(m12)
    has = (m12 >= 0) & (m12 < n2)
    j = np.where(has, m12, 0)
    O1, O2 = camera_centres(T1[None])[0], camera_centres(T2[None])[0]
    want = TW.triangulate_centres(T1, T2, O1, O2, C.CAMERA, C.SCALE, C.SIGMA2, np.asarray(xy1, np.float32)[has], np.asarray(xy2, np.float32)[j[has]],
                                  np.asarray(l1)[has], np.asarray(l2)[j[has]]) if n2 else None
    assert (got["status"][~has] == 1).all()
    if has.any():
        assert got["status"][has].tolist() == want["status"].tolist()
        for k in ("X", "normal", "dmin2", "dmax2"):
            assert same_bits(got[k][has], want[k])
    bad = got["status"] != 0
    for k in ("X", "normal", "dmin2", "dmax2"):
        assert np.isnan(got[k][bad]).all() and np.isfinite(got[k][~bad]).all()
    assert created[0] == (~bad).sum()
    return got


def test_every_status_on_the_device(tm, gpu_ctx):
    seen = []
    for T1, T2, p1, p2, l1, l2, status in C.status_cases():
        got = tri_check(tm, gpu_ctx, [p1], [p2], [l1], [l2], [0], T1, T2)
        assert got["status"][0] == status
        seen.append(status)
    assert seen == [0, 2, 3, 4, 5, 6, 7, 8]


def test_geometry_on_the_300_match_scene_and_65_rows(tm, gpu_ctx):
    s1, s2, _, truth = C.make_scene(11, 300, 300)
    m12 = np.full(300, -1, np.int32)
    m12[truth["rows1"]] = truth["rows2"]
    m12[::11] = -1
    m12[5] = 300                                              # out of range: no match, no read
    level2 = s2["level"].copy()
    level2[::9] += 4
    got = tri_check(tm, gpu_ctx, s1["xy"], s2["xy"], s1["level"], level2, m12, C.POSES[0], C.POSES[1])
    assert {0, 1, 8} <= set(got["status"].tolist()) and (got["status"] == 0).sum() > 200
    ok = got["status"] == 0
    point_of_row = np.full(300, -1)
    point_of_row[truth["rows1"]] = np.arange(300)
    assert np.linalg.norm(got["X"][ok] - truth["X"][point_of_row[ok]], axis=1).max() < 0.5
    got = tri_check(tm, gpu_ctx, s1["xy"][:65], s2["xy"], s1["level"][:65], s2["level"], np.minimum(m12[:65], 299), C.POSES[0], C.POSES[1])
    assert len(got["status"]) == 65
    tri_check(tm, gpu_ctx, s1["xy"][:3], np.zeros((0, 2), np.float32), s1["level"][:3], np.zeros(0, np.int32), [0, -1, 2], C.POSES[0], C.POSES[1])


# ---- the chain --------------------------------------------------------------------------------------------------------------------

def test_keyframes_to_points_to_projection_search(tm, gpu_ctx):
    """Two keyframes of 200 rows seeing 150 common points: create_new_map_points, PointSets from its UNCOMPACTED arrays,
    search_by_projection into a third frame: the created points are found there, the NaN rows come back with status 1."""
    from slamhip import FrameGrids, PointSets, search_by_projection
    from backend import Backend
    s1, s2, s3, truth = C.make_scene(3, 150, 200)
    f, v, bins = make_set(tm, gpu_ctx, [s1, s2])
    try:
        pts, matched, created = tm.create_new_map_points(f, f, [(0, 1)], v, v, C.POSES[0][None], C.POSES[1][None], C.CAMERA,
                                                         (C.SCALE, C.SIGMA2), bins, bins, ctx=gpu_ctx)
        d = pts[0]
        F = R.fundamental(C.POSES[0], C.POSES[1], C.CAMERA)
        want, count, _ = R.search(s1, s2, tm.fundamental_from_poses(C.POSES[0], C.POSES[1], C.CAMERA), tm.epipole_in_second(C.POSES[0], C.POSES[1], C.CAMERA),
                                  C.SCALE, C.SIGMA2)
        assert np.allclose(F, tm.fundamental_from_poses(C.POSES[0], C.POSES[1], C.CAMERA), rtol=1e-12, atol=1e-18)
        assert np.array_equal(d["matches12"], want) and matched[0] == count
        right = (d["matches12"][truth["rows1"]] == truth["rows2"]) & (d["status"][truth["rows1"]] == 0)
        assert right.sum() >= 0.9 * 150 and created[0] == (d["status"] == 0).sum() >= right.sum()
        made = d["status"] == 0
        assert made.sum() < 200 and np.isnan(d["X"][~made]).all()
        out = Backend().create_new_map_points(f, 0, [1], np.stack([C.POSES[0], C.POSES[1]]), *C.CAMERA, views=v, bins=bins,
                                              scale=(C.SCALE, C.SIGMA2))
        assert np.array_equal(out[0][0], np.flatnonzero(made)) and np.array_equal(out[0][1], d["matches12"][made]) and same_bits(out[0][2], d["X"][made])
        # uncompacted into PointSets: descriptors and levels are side 1's
        ps = PointSets(d["X"], s1["desc"], dmin2=d["dmin2"], dmax2=d["dmax2"], normal=d["normal"], bins=s1["bins"], ctx=gpu_ctx)
        fr = FrameGrids.from_arrays(s3["desc"], s3["xy"], s3["level"], C.SIZE, bins=s3["bins"], ctx=gpu_ctx)
        try:
            m13, c13, tabs = search_by_projection(ps, fr, [(0, 0)], C.POSES[2][None], camera=C.CAMERA, scale=(C.SCALE, C.SIGMA2), th=4.0,
                                                  return_tables=True, ctx=gpu_ctx)
        finally:
            ps.free()
            fr.free()
        assert (tabs[0]["status"][~made] == 1).all() and (m13[0][~made] == -1).all()
        # the range is UpdateNormalAndDepth's own (no 0.8 / 1.2 margin): a level-0 point is out of range (status 3) from a
        # camera farther away than keyframe 1 was; every other created point is searched and found at its row
        found = m13[0][truth["rows1"]] == truth["rows3"]
        st3 = tabs[0]["status"][truth["rows1"]]
        searched = right & (st3 == 0)
        print("created %d, searched %d and found %d of them in the third frame" % (right.sum(), searched.sum(), (found & searched).sum()))
        assert set(st3[right].tolist()) <= {0, 3} and (s1["level"][truth["rows1"]][right & (st3 == 3)] == 0).all()
        assert searched.sum() >= 0.8 * right.sum() and (found & searched).sum() >= 0.95 * searched.sum()
    finally:
        f.free()
        v.free()


# ---- errors -----------------------------------------------------------------------------------------------------------------------

def test_invalid_calls_launch_nothing_and_leave_the_context_usable(tm, gpu_ctx):
    from slamhip._lib import BowGroups, TriParams, TriViews, addr
    s1, s2 = C.random_pair(71, 40, 60, n_nodes=3)
    f, v, _ = make_set(tm, gpu_ctx, [s1, s2])
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    out = gpu_ctx.malloc(1 << 16)
    try:
        gpu_ctx.sync()
        before = out.download(np.uint8, (1 << 16,))
        pairs = np.array([[0, 1], [1, 0]], np.int32)
        F, E = np.ascontiguousarray(np.broadcast_to(C.F_RECT.reshape(9), (2, 9))), np.ascontiguousarray(np.broadcast_to(C.NO_EPIPOLE, (2, 2)))
        T, O = np.ascontiguousarray(np.broadcast_to(C.POSES[0], (2, 3, 4))), np.zeros((2, 3))
        long_off = np.array([0, tm.ROWS_MAX + 1], np.int64)

        def groups(off=f.offsets, B=2, desc=f.device[0].ptr):
            return BowGroups(desc, f.device[1].ptr, f.device[2].ptr, f.device[3].ptr, None, addr(off), B)

        tv = v._struct(gpu_ctx, f.n)
        s, s2t = C.SCALE, C.SIGMA2

        def params(n_levels=8, th_low=50, chi2=3.84, scale=addr(s), sigma2=addr(s2t), cos_max=0.9998):
            return TriParams(*C.CAMERA, chi2, 100.0, cos_max, 5.991, 1.8, scale, sigma2, n_levels, th_low)

        g, prm = groups(), params()

        def search(g1=g, g2=g, v1=tv, v2=tv, p=addr(pairs), P=2, F_=addr(F), E_=addr(E), prm=prm, order=0, m=out.ptr, c=out.ptr + 4096,
                   i=None, dd=None, ctx=h):
            ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
            return lib.slam_tri_match_search(ctx, ref(g1), ref(g2), ref(v1), ref(v2), p, P, F_, E_, ref(prm), order, m, c, i, dd)

        def tri(off=addr(f.offsets), B=2, v1=tv, p=addr(pairs), P=2, m=out.ptr, T1=addr(T), O1=addr(O), prm=prm, X=out.ptr + 8192,
                created=out.ptr + 4096, ctx=h):
            ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
            return lib.slam_tri_match_triangulate(ctx, off, B, addr(f.offsets), 2, ref(v1), ref(tv), p, P, m, T1, addr(T), O1, addr(O), ref(prm),
                                                  X, out.ptr + 16384, out.ptr + 24576, out.ptr + 32768, created)

        bad = [search(ctx=None), search(g1=None), search(g2=None), search(v1=None), search(v2=None), search(p=None), search(F_=None),
               search(E_=None), search(prm=None), search(P=tm.PAIRS_MAX + 1), search(P=-1), search(g1=groups(long_off, 1)),
               search(g1=groups(desc=None)), search(v1=TriViews(None, tv.d_level, None)), search(v2=TriViews(tv.d_xy, None, None)),
               search(p=addr(np.array([[0, 2], [0, 0]], np.int32))), search(order=2), search(prm=params(n_levels=0)),
               search(prm=params(n_levels=17)), search(prm=params(th_low=-1)), search(prm=params(th_low=257)),
               search(prm=params(chi2=float("nan"))), search(prm=params(scale=None)), search(prm=params(sigma2=None)), search(m=None),
               search(c=None), search(i=out.ptr + 8192),
               tri(ctx=None), tri(off=None), tri(off=addr(long_off), B=1), tri(v1=None), tri(v1=TriViews(None, tv.d_level, None)), tri(p=None),
               tri(P=tm.PAIRS_MAX + 1), tri(m=None), tri(T1=None), tri(O1=None), tri(prm=None), tri(prm=params(n_levels=0)),
               tri(prm=params(cos_max=float("nan"))), tri(X=None), tri(created=None)]
        assert bad == [-1] * len(bad)
        gpu_ctx.sync()
        assert np.array_equal(out.download(np.uint8, (1 << 16,)), before)        # nothing was written
        assert gpu_ctx.state_dirty() == 0
        assert search() == 0 and tri() == 0                                      # the same calls with valid arguments succeed
        gpu_ctx.sync()
        want, count, _ = R.search(s1, s2, C.F_RECT, C.NO_EPIPOLE, C.SCALE, C.SIGMA2)
        assert np.array_equal(out.download(np.int32, (100,))[:40], want)
        for call in (lambda: tm.search_for_triangulation(f, f, [(0, 2)], v, v, C.F_RECT, C.NO_EPIPOLE),
                     lambda: tm.search_for_triangulation(f, f, [(0, 1)], v, v, np.zeros((2, 3, 3)), C.NO_EPIPOLE),
                     lambda: tm.search_for_triangulation(f, f, [(0, 1)], v, v, C.F_RECT, C.NO_EPIPOLE, th_low=300),
                     lambda: tm.search_for_triangulation(f, f, [(0, 1)], v, v, C.F_RECT, C.NO_EPIPOLE, bins1=np.zeros(100, int)),
                     lambda: tm.triangulate_matches(f, f, [(0, 1)], v, v, [np.zeros(41, int)], C.POSES[0][None], C.POSES[1][None], C.CAMERA),
                     lambda: tm.KeyframeViews(np.zeros((3, 2)), [0, 1, 16], ctx=gpu_ctx),
                     lambda: tm.KeyframeViews(np.zeros((3, 2)), [0, 1, 2], taken=[0, 1], ctx=gpu_ctx)):
            with pytest.raises(ValueError):
                call()
        assert gpu_ctx.state_dirty() == 0
    finally:
        out.free()
        f.free()
        v.free()
