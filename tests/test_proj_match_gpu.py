"""The projection search on the device against tests/proj_match_ref.py bit for bit: matches, counts and every
table, at the smallest shapes where each path can go wrong."""
import ctypes

import numpy as np
import pytest

import proj_match_cases as C
import proj_match_ref as R
from hamming_families import prefix_rows

pytestmark = pytest.mark.gpu

I34 = np.eye(4)[:3]
ONE = R.scale_tables(1, 1.0)
S12 = R.scale_tables(8, 1.2)
S2 = R.scale_tables(4, 2.0)
FIELDS = ("range", "normal", "level", "bins")


@pytest.fixture(scope="module")
def pm(built):
    from slamhip import proj_match as module
    return module


def cat(dicts, key, shape, dtype):
    parts = [np.asarray(d[key], dtype).reshape(shape) for d in dicts]
    return np.concatenate(parts) if parts else np.zeros((0,) + tuple(shape[1:]), dtype)


def upload(pm, ctx, pts, frames, size=C.SIZE, cell=16):
    """PointSets and FrameGrids of lists of the reference's dicts (every dict of a list carries the same optional fields)."""
    off1 = np.concatenate([[0], np.cumsum([len(p["xyz"]) for p in pts])]).astype(np.int64)
    off2 = np.concatenate([[0], np.cumsum([len(f["level"]) for f in frames])]).astype(np.int64)
    has = lambda ds, k: bool(ds) and ds[0].get(k) is not None  # noqa: E731
    rng = cat(pts, "range", (-1, 2), np.float64) if has(pts, "range") else None
    ps = pm.PointSets(cat(pts, "xyz", (-1, 3), np.float64), cat(pts, "desc", (-1, 32), np.uint8), off1,
                      dmin2=None if rng is None else rng[:, 0], dmax2=None if rng is None else rng[:, 1],
                      normal=cat(pts, "normal", (-1, 3), np.float64) if has(pts, "normal") else None,
                      level=cat(pts, "level", (-1,), np.int64) if has(pts, "level") else None,
                      bins=cat(pts, "bins", (-1,), np.int64) if has(pts, "bins") else None, ctx=ctx)
    fg = pm.FrameGrids.from_arrays(cat(frames, "desc", (-1, 32), np.uint8), cat(frames, "xy", (-1, 2), np.float32),
                                   cat(frames, "level", (-1,), np.int64), size, off2,
                                   bins=cat(frames, "bins", (-1,), np.int64) if has(frames, "bins") else None,
                                   taken=cat(frames, "taken", (-1,), np.int64) if has(frames, "taken") else None, cell=cell, ctx=ctx)
    return ps, fg


def compare(got, want, where=""):
    m, c, t = got
    assert np.array_equal(m, want[0]) and m.dtype == np.int32, where
    assert int(c) == want[1], where
    for k in ("status", "u", "v", "lp", "idx", "dist"):
        assert C.same_bits(t[k], want[2][k]), (where, k)


def run(pm, ctx, pts, frames, pairs, poses, centres, th, camera=C.CAMERA, bounds=C.BOUNDS, scale=S12, size=C.SIZE, cell=16, ref=True, **kw):
    """One call on the device, every pair compared with the reference; returns the device's (matches, counts, tables)."""
    ps, fg = upload(pm, ctx, pts, frames, size, cell)
    try:
        got = pm.search_by_projection(ps, fg, pairs, poses, centres, camera, bounds, scale, th, return_tables=True, ctx=ctx,
                                      level_offsets=kw.get("offsets"), **{k: v for k, v in kw.items() if k != "offsets"})
    finally:
        ps.free()
        fg.free()
    th = np.broadcast_to(np.asarray(th, np.float64), (len(pairs),))
    if ref:
        for p, (a, b) in enumerate(pairs):
            want = R.search(pts[a], frames[b], poses[p], centres[p], th[p], camera, bounds, *scale, **kw)
            compare((got[0][p], got[1][p], got[2][p]), want, f"pair {p}")
    return got


def rows(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def cloud(rng, n, fields=(), z=(2.0, 8.0)):
    """n points whose projections under the identity pose cover the image and a little more."""
    u, v, d = rng.uniform(-30, C.SIZE[0] + 30, n), rng.uniform(-30, C.SIZE[1] + 30, n), rng.uniform(*z, n)
    p = dict(xyz=np.stack([(u - 320) / 256 * d, (v - 240) / 256 * d, d], 1), desc=rows(rng, n))
    dist = np.linalg.norm(p["xyz"], axis=1)
    if "range" in fields:
        p["range"] = np.stack([(0.5 * dist) ** 2, (dist * rng.uniform(0.9, 4.0, n)) ** 2], 1)
    if "normal" in fields:
        nr = p["xyz"] + rng.normal(0, 2.0, (n, 3))                  # about the viewing direction: some beyond 60 degrees
        p["normal"] = nr / np.linalg.norm(nr, axis=1)[:, None]
    if "level" in fields:
        p["level"] = rng.integers(0, 8, n).astype(np.int32)
    if "bins" in fields:
        p["bins"] = rng.integers(0, 32, n)
    return p


def features(rng, n, bins=False, taken=False, size=C.SIZE):
    f = dict(desc=rows(rng, n), xy=np.stack([rng.uniform(0, size[0], n), rng.uniform(0, size[1], n)], 1).astype(np.float32),
             level=rng.integers(0, 8, n).astype(np.int32))
    if bins:
        f["bins"] = rng.integers(0, 32, n)
    if taken:
        f["taken"] = (rng.uniform(size=n) < 0.2).astype(np.uint8)
    return f


# ---- sizes and pair counts ----------------------------------------------------------------------------------------------

def test_every_small_size_in_one_call(pm, gpu_ctx):
    rng = np.random.default_rng(501)
    pts = [cloud(rng, n, FIELDS) for n in (0, 1, 63, 64, 65)]
    frames = [features(rng, n, bins=True, taken=True) for n in (0, 1, 64, 65)]
    pairs = [(a, b) for a in range(5) for b in range(4)]
    poses = [C.random_pose(rng, 0.05, 0.1) for _ in pairs]
    centres = [rng.normal(0, 0.1, 3) for _ in pairs]
    got = run(pm, gpu_ctx, pts, frames, pairs, poses, centres, rng.uniform(20, 60, len(pairs)), ratio=1.0, th_high=256)
    assert sum(int(c) for c in got[1]) > 20
    assert [len(m) for m in got[0]] == [len(pts[a]["xyz"]) for a, _ in pairs]


@pytest.mark.parametrize("fields", [(), ("level",), ("range",), ("normal", "bins")])
def test_one_and_two_pairs_with_each_optional_field(pm, gpu_ctx, fields):
    rng = np.random.default_rng(502)
    pts = [cloud(rng, 300, fields), cloud(rng, 130, fields)]
    frames = [features(rng, 500, bins="bins" in fields), features(rng, 257, bins="bins" in fields)]
    for pairs in ([(0, 0)], [(1, 0), (0, 1)], [(0, 0), (1, 0), (0, 0)], [(1, 1), (1, 0)]):         # sharing a frame; sharing a point set
        poses = [C.random_pose(rng, 0.05, 0.1) for _ in pairs]
        got = run(pm, gpu_ctx, pts, frames, pairs, poses, [np.zeros(3)] * len(pairs), 25.0, ratio=0.95, th_high=256)
        assert sum(int(c) for c in got[1]) > 5


def test_full_sets_and_the_last_point_wins_its_claim(pm, gpu_ctx):
    rng = np.random.default_rng(503)
    n = 8192
    p, f = cloud(rng, n), features(rng, n)
    f["level"][:] = 0
    # point 8191 and point 5 both sit on frame row 8000 with the row's descriptor but for 1 and 3 bits: 8191 is nearer and keeps it
    f["xy"][8000] = (100.5, 200.25)
    for i, flips in ((8191, 1), (5, 3)):
        p["xyz"][i] = ((100.5 - 320) / 256 * 4.0, (200.25 - 240) / 256 * 4.0, 4.0)
        p["desc"][i] = C.flip_bits(rng, f["desc"][8000:8001], flips)[0]
    got = run(pm, gpu_ctx, [p], [f], [(0, 0)], [I34], [np.zeros(3)], 12.0, ratio=1.0, th_high=256)
    assert got[0][0][8191] == 8000 and got[0][0][5] == -1 and got[2][0]["idx"][5, 0] == 8000


def test_4096_tiny_pairs_and_one_too_many(pm, gpu_ctx):
    rng = np.random.default_rng(504)
    pts = [cloud(rng, int(n)) for n in rng.integers(0, 5, 64)]
    frames = [features(rng, int(n)) for n in rng.integers(0, 7, 64)]
    pairs = [(int(a), int(b)) for a, b in zip(rng.integers(0, 64, 4096), rng.integers(0, 64, 4096))]
    got = run(pm, gpu_ctx, pts, frames, pairs, [I34] * 4096, [np.zeros(3)] * 4096, 200.0, ref=False, th_high=256)
    cache = {}
    for p, (a, b) in enumerate(pairs):
        if (a, b) not in cache:
            cache[a, b] = R.search(pts[a], frames[b], I34, np.zeros(3), 200.0, C.CAMERA, C.BOUNDS, *S12, th_high=256)
        compare((got[0][p], got[1][p], got[2][p]), cache[a, b], f"pair {p}")
    assert sum(int(c) for c in got[1]) > 1000
    ps, fg = upload(pm, gpu_ctx, pts, frames)
    try:
        with pytest.raises(ValueError):
            pm.search_by_projection(ps, fg, pairs + [(0, 0)], [I34] * 4097, ctx=gpu_ctx)
    finally:
        ps.free()
        fg.free()


# ---- windows ---------------------------------------------------------------------------------------------------------------

def at_pixels(uv, desc, z=4.0, **extra):
    """Points that project exactly onto the pixels uv (multiples of 1/64) under the identity pose: X = (u - 320) z / 256."""
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    return dict(xyz=np.stack([(uv[:, 0] - 320) / 256 * z, (uv[:, 1] - 240) / 256 * z, np.full(len(uv), z)], 1), desc=desc, **extra)


def test_window_edges_are_strict(pm, gpu_ctx):
    f32 = np.float32
    u, v, r = 200.0, 100.0, 8.0
    inside = lambda x, to: float(np.nextafter(f32(x), f32(to)))  # noqa: E731
    xy = [(u + r, v), (u - r, v), (u, v + r), (u, v - r),                                       # exactly on the window: out
          (inside(u + r, 0), v), (inside(u - r, 1e9), v), (u, inside(v + r, 0)), (u, inside(v - r, 1e9)),   # the next f32 inside: in
          (u + r, v + r), (inside(u + r, 0), inside(v + r, 0)), (u, v)]
    fr = dict(desc=prefix_rows(np.arange(10, 10 + len(xy))), xy=np.array(xy, f32), level=np.zeros(len(xy), np.int32))
    pts = at_pixels([(u, v)] * 11, prefix_rows(np.arange(10, 21)))
    for cell in (1, 16, 640):
        got = run(pm, gpu_ctx, [pts], [fr], [(0, 0)], [I34], [np.zeros(3)], r, scale=ONE, cell=cell, ratio=100.0)
        t = got[2][0]
        assert (t["u"] == u).all() and (t["v"] == v).all()
        assert not np.isin(t["idx"], [0, 1, 2, 3, 8]).any()
        assert t["idx"][4].tolist() == [4, 5] and t["idx"][10].tolist() == [10, 9] and t["idx"][0].tolist() == [4, 5]


def test_cell_edges_corners_and_one_crowded_cell(pm, gpu_ctx):
    rng = np.random.default_rng(506)
    W, H = C.SIZE
    edge = [(x, y) for x in (0.0, 15.999, 16.0, 16.001, 31.999, 32.0, W - 16.0, W - 0.001, float(W), W + 5.0, -3.0)
            for y in (0.0, 15.999, 16.0, 32.0, H - 16.0, H - 0.001, float(H), H + 7.0, -2.0)]
    fr = dict(desc=rows(rng, len(edge)), xy=np.array(edge, np.float32), level=np.zeros(len(edge), np.int32))
    crowd = features(rng, 300)
    crowd["xy"] = (np.array([[160.0, 160.0]]) + rng.uniform(0, 15.9, (300, 2))).astype(np.float32)      # every row in one cell of 16
    uv = np.array(edge)[::2] + rng.uniform(-3, 3, (len(edge[::2]), 2))
    pts_edge = at_pixels(np.round(uv * 64) / 64, rows(rng, len(uv)))
    pts_crowd = at_pixels(np.round((160 + rng.uniform(-10, 26, (70, 2))) * 64) / 64, rows(rng, 70))
    big = (-50.0, W + 50.0, -50.0, H + 50.0)
    ref = None
    for cell in (1, 7, 16, 64, max(W, H)):
        got = run(pm, gpu_ctx, [pts_edge, pts_crowd], [fr, crowd], [(0, 0), (1, 1)], [I34, I34], [np.zeros(3)] * 2, [9.0, 12.0], bounds=big,
                  scale=ONE, cell=cell, ratio=1.0, th_high=256, ref=ref is None)
        if ref is None:
            ref = got
            assert (got[2][0]["idx"][:, 0] >= 0).sum() > 20 and (got[2][1]["idx"][:, 1] >= 0).sum() > 30
        else:                                                                                           # identical bits for every cell
            for p in range(2):
                assert np.array_equal(got[0][p], ref[0][p]) and got[1][p] == ref[1][p]
                assert all(C.same_bits(got[2][p][k], ref[2][p][k]) for k in ref[2][p])


def test_cells_and_order_are_host_readable(pm, gpu_ctx):
    rng = np.random.default_rng(507)
    f = [features(rng, 200), features(rng, 77)]
    f[0]["xy"][:4] = [(-5, -5), (700, 500), (639.99, 479.99), (16, 16)]
    _, fg = upload(pm, gpu_ctx, [], f, cell=16)
    try:
        assert fg.grid == (40, 30) and fg.offsets.tolist() == [0, 200, 277]
        xy = np.concatenate([f[0]["xy"], f[1]["xy"]]).astype(np.float64)
        want = np.clip(np.floor(xy[:, 1] / 16), 0, 29).astype(np.int32) * 40 + np.clip(np.floor(xy[:, 0] / 16), 0, 39).astype(np.int32)
        cells, order = fg.cells, fg.order
        assert np.array_equal(cells, want) and cells[:4].tolist() == [0, 29 * 40 + 39, 29 * 40 + 39, 41]
        for b, (lo, hi) in enumerate(((0, 200), (200, 277))):
            assert np.array_equal(order[lo:hi], np.argsort(want[lo:hi], kind="stable"))
            assert np.array_equal(fg.cells_sorted[lo:hi], want[lo:hi][order[lo:hi]])
            assert np.array_equal(fg.xy_sorted[lo:hi], f[b]["xy"][order[lo:hi]])
    finally:
        fg.free()


def test_frame_grids_of_an_orb_result(pm, gpu_ctx):
    """One image kept on the device is grouped from its resident descriptor block, a batch from the host copies: both are the
    grid of the same arrays."""
    from slamhip.orb import orb_extract_arrays
    rng = np.random.default_rng(509)
    images = rng.integers(0, 256, (2, 120, 160), dtype=np.uint8)
    for batch in (images[0], images):
        res = orb_extract_arrays(batch, n_features=200, ctx=gpu_ctx, keep_on_device=True)
        try:
            assert res.counts.min() > 20
            got = pm.FrameGrids.from_orb(res, cell=16, ctx=gpu_ctx)
            want = pm.FrameGrids.from_arrays(np.concatenate(res.descriptors), np.concatenate(res.xy), np.concatenate(res.level), (160, 120),
                                             np.concatenate([[0], np.cumsum(res.counts)]), np.concatenate(res.bin), ctx=gpu_ctx)
            try:
                assert got.size == (160, 120) and got.offsets.tolist() == want.offsets.tolist() and got.grid == (10, 8)
                for name in ("order", "cells", "cells_sorted", "xy_sorted", "descriptors_sorted"):
                    assert C.same_bits(getattr(got, name), getattr(want, name)), name
                assert np.array_equal(got.descriptors_sorted[:int(res.counts[0])], res.descriptors[0][got.order[:int(res.counts[0])]])
            finally:
                got.free()
                want.free()
        finally:
            res.free()


def test_whole_image_window_is_the_dense_top2(pm, gpu_ctx):
    from feature_matchers import BruteForceFeatureMatcher
    rng = np.random.default_rng(508)
    q, t = rows(rng, 150), rows(rng, 333)
    t[7] = t[200]
    q[3] = t[200]                                                                                       # a tie goes to the lower row
    idx, dist = pm.proj_match_arrays(q, t, rng.uniform(0, 640, (150, 2)), rng.uniform(0, 640, (333, 2)), 1e6, C.SIZE, ctx=gpu_ctx)
    ridx, rdist = BruteForceFeatureMatcher(norm_type=6).knn_match_arrays(q, t, k=2)
    assert np.array_equal(idx, ridx) and np.array_equal(dist, rdist) and idx[3].tolist() == [7, 200]
    one = pm.proj_match_arrays(q, t, rng.uniform(0, 640, (150, 2)), rng.uniform(0, 640, (333, 2)), 1e6, C.SIZE, k=1, ctx=gpu_ctx)
    assert np.array_equal(one[0], ridx[:, :1])


# ---- gates -----------------------------------------------------------------------------------------------------------------

def test_gate_edges_never_match_and_never_fault(pm, gpu_ctx):
    xyz, rng_, nrm, status, lp = C.edge_points()
    n = len(xyz)
    pts = dict(xyz=xyz, desc=prefix_rows(np.full(n, 40)), range=rng_, normal=nrm)
    fr = dict(desc=prefix_rows([40, 41, 42]), xy=np.array([(320, 240), (0, 240), (320, 0)], np.float32), level=np.array([3, 3, 2], np.int32))
    got = run(pm, gpu_ctx, [pts], [fr], [(0, 0)], [I34], [np.zeros(3)], 2.0, scale=S2, ratio=100.0)
    t = got[2][0]
    assert t["status"].tolist() == status.tolist() and t["lp"].tolist() == lp.tolist()
    dead = status != 0
    assert (got[0][0][dead] == -1).all() and (t["idx"][dead] == -1).all() and (t["dist"][dead] == 2**31 - 1).all()
    assert (t["idx"][~dead & (lp == 3), 0] >= 0).all()
    ps, _ = upload(pm, gpu_ctx, [pts], [])
    try:
        only = pm.project_points(ps, [0, 0], [I34, I34], [np.zeros(3)] * 2, C.CAMERA, C.BOUNDS, S2, 2.0, ctx=gpu_ctx)
    finally:
        ps.free()
    for o in only:
        assert all(C.same_bits(o[k], t[k]) for k in ("status", "u", "v", "lp"))


# ---- levels, selection, one-to-one, rotation -------------------------------------------------------------------------------

def test_level_rule_under_both_defaults_clamps_and_taken(pm, gpu_ctx):
    xy = np.tile(np.array([[320.0, 240.0]], np.float32), (8, 1))
    fr = dict(desc=prefix_rows([50] * 8), xy=xy, level=np.array([0, 1, 2, 3, 0, 1, 2, 3], np.int32), taken=np.array([0, 1, 0, 0, 0, 0, 0, 0], np.uint8))
    z = np.array([[0.0, 0.0, 4.0]] * 3)
    with_range = dict(xyz=z, desc=prefix_rows([50] * 3), range=np.array([[1.0, 256.0], [1.0, 16.0], [1.0, 4096.0]]))   # lp = 2, 0, 3
    got = run(pm, gpu_ctx, [with_range], [fr], [(0, 0)], [I34], [np.zeros(3)], 1.0, scale=S2, ratio=100.0)
    assert got[2][0]["lp"].tolist() == [2, 0, 3]
    assert got[2][0]["idx"].tolist() == [[2, 5], [0, 4], [2, 3]]                 # lp-1 .. lp without taken row 1; lp = 0: level 0 only
    with_level = dict(xyz=z, desc=prefix_rows([50] * 3), level=np.array([2, 0, 3], np.int32))
    got = run(pm, gpu_ctx, [with_level], [fr], [(0, 0)], [I34], [np.zeros(3)], 1.0, scale=S2, ratio=100.0)
    assert got[2][0]["idx"].tolist() == [[2, 3], [0, 4], [2, 3]]                 # lp-1 .. lp+1
    run(pm, gpu_ctx, [with_level], [fr], [(0, 0)], [I34], [np.zeros(3)], 1.0, scale=S2, offsets=(-2, 1))
    run(pm, gpu_ctx, [with_level], [fr], [(0, 0)], [I34], [np.zeros(3)], 1.0, scale=S2, level_rule=False)


def test_selection_rules(pm, gpu_ctx):
    xy = np.array([[320.0, 240.0], [323.0, 240.0], [320.0, 244.0], [330.0, 240.0], [316.5, 236.5]], np.float32)
    pts = at_pixels([(320, 240)], prefix_rows([101]))
    call = lambda level, th, **kw: run(pm, gpu_ctx, [pts], [dict(desc=prefix_rows([100, 104, 90, 100, 131]), xy=xy, level=np.array(level, np.int32))],  # noqa: E731
                                       [(0, 0)], [I34], [np.zeros(3)], th, scale=ONE, **kw)[0][0].tolist()
    assert call([0, 0, 1, 0, 0], 4.0) == [0]
    assert call([0, 0, 1, 0, 0], 4.0, ratio=0.3) == [-1]                         # a same-level second neighbour rejects
    assert call([0, 1, 1, 0, 0], 4.0, ratio=0.3) == [0]                          # on another level it passes
    assert call([0, 0, 1, 0, 0], 1.0, ratio=0.0) == [0]                          # a missing second neighbour passes
    assert call([0, 0, 1, 0, 0], 1.0, th_high=1) == [0]                          # d0 == th_high is kept
    assert call([0, 0, 1, 0, 0], 1.0, th_high=0) == [-1]


def test_one_row_two_points_equal_distance(pm, gpu_ctx):
    fr = dict(desc=prefix_rows([50, 90]), xy=np.array([[320.0, 240.0], [321.0, 240.0]], np.float32), level=np.zeros(2, np.int32))
    pts = dict(xyz=np.array([[0.0, 0.0, 4.0], [0.0, 0.0, 8.0], [0.0, 0.0, 2.0]]), desc=prefix_rows([53, 47, 52]))
    got = run(pm, gpu_ctx, [pts, dict(xyz=pts["xyz"][:2], desc=pts["desc"][:2])], [fr], [(0, 0), (1, 0)], [I34, I34], [np.zeros(3)] * 2, 2.0,
              scale=ONE, ratio=10.0)
    assert got[0][0].tolist() == [-1, -1, 0] and got[0][1].tolist() == [0, -1] and got[1].tolist() == [1, 1]


@pytest.mark.parametrize("turns,kept", [([0] * 10 + [5] * 10 + [9] * 10 + [20] * 10, {0, 5, 9}),        # a four-way tie: the three lower bins
                                        ([3] * 20 + [7] * 2 + [8] * 1, {3, 7}),                           # 10 %: 2 of 20 stays, 1 of 20 goes
                                        ([31] * 30 + [0] * 3 + [1] * 3 + [2] * 3, {31, 0, 1})])
def test_rotation_histogram_ties_and_ten_percent(pm, gpu_ctx, turns, kept):
    n = len(turns)
    rng = np.random.default_rng(511)
    uv = np.stack([20.0 + 15 * np.arange(n), np.full(n, 100.0)], 1)
    desc = rows(rng, n)
    bins2 = rng.integers(0, 32, n)
    fr = dict(desc=desc, xy=uv.astype(np.float32), level=np.zeros(n, np.int32), bins=bins2)
    pts = at_pixels(uv, desc, bins=(bins2 + np.array(turns)) % 32)
    got = run(pm, gpu_ctx, [pts], [fr], [(0, 0)], [I34], [np.zeros(3)], 3.0, scale=ONE, bounds=(0.0, 2000.0, 0.0, 480.0), size=(2000, 480))
    assert (got[0][0] >= 0).tolist() == [t in kept for t in turns]


# ---- SearchBySim3 --------------------------------------------------------------------------------------------------------

def test_search_by_sim3_against_its_restatement(pm, gpu_ctx):
    rng = np.random.default_rng(512)
    pts1, fr2, T2, row2 = C.make_scene(31, 400, 100)            # a map as keyframe 2 sees it
    n = 400
    # keyframe 1 sees the same landmarks in its own, scaled and moved, world: x1 = s R x2 + t in camera coordinates
    s, S = 1.3, None
    S = np.c_[s * C.random_pose(rng, 0.2, 0.0)[:, :3], rng.normal(0, 0.3, 3)]
    T1 = C.random_pose(rng, 0.1, 0.2)
    cam2 = pts1["xyz"] @ T2[:, :3].T + T2[:, 3]
    cam1 = cam2 @ S[:, :3].T + S[:, 3]
    seen1 = (cam1[:, 2] > 0.5)
    w1 = (cam1 - T1[:, 3]) @ T1[:, :3]                           # the landmarks in the world of keyframe 1
    uv1 = np.stack([256 * cam1[:, 0] / cam1[:, 2] + 320, 256 * cam1[:, 1] / cam1[:, 2] + 240], 1)
    perm1 = rng.permutation(n)
    fr1 = dict(desc=C.flip_bits(rng, pts1["desc"], 10)[perm1], xy=uv1[perm1].astype(np.float32), level=np.zeros(n, np.int32))
    row1 = np.argsort(perm1)
    fr2 = dict(fr2, level=np.zeros(len(fr2["level"]), np.int32))
    some1, some2 = np.flatnonzero(seen1)[::2], np.arange(0, n, 3)           # the map points each keyframe holds
    P1 = dict(xyz=w1[some1], desc=pts1["desc"][some1])
    P2 = dict(xyz=pts1["xyz"][some2], desc=pts1["desc"][some2])
    rows1, rows2 = row1[some1], row2[some2]
    ps1, fg1 = upload(pm, gpu_ctx, [P1], [fr1])
    ps2, fg2 = upload(pm, gpu_ctx, [P2], [fr2])
    try:
        out = pm.search_by_sim3(ps1, fg1, [rows1], ps2, fg2, [rows2], [(0, 0)], [T1], [T2], [S], C.CAMERA, scale=S12, th=7.5, ctx=gpu_ctx)
    finally:
        for o in (ps1, fg1, ps2, fg2):
            o.free()
    A12, A21 = R.compose(R.invert(S), T1), R.compose(S, T2)
    kw = dict(ratio=np.inf)
    m12 = R.search(P1, fr2, A12, -np.linalg.solve(A12[:, :3], A12[:, 3]), 7.5, C.CAMERA, C.BOUNDS, *S12, **kw)[0]
    m21 = R.search(P2, fr1, A21, -np.linalg.solve(A21[:, :3], A21[:, 3]), 7.5, C.CAMERA, C.BOUNDS, *S12, **kw)[0]
    i, k = R.mutual(m12, rows1, m21, rows2)
    assert np.array_equal(out[0][0], i) and np.array_equal(out[0][1], k) and out[0][0].dtype == np.int32
    both = np.intersect1d(some1, some2)                                      # the landmarks both keyframes hold ...
    inside = (np.abs(uv1[both, 0] - 320) < 300) & (np.abs(uv1[both, 1] - 240) < 220)        # ... well inside both images: these must agree
    assert (some1[i] == some2[k]).all() and np.isin(both[inside], some1[i]).mean() > 0.9 and inside.sum() > 30


# ---- errors, determinism ------------------------------------------------------------------------------------------------------

def test_invalid_calls_launch_nothing_and_leave_the_context_usable(pm, gpu_ctx):
    from slamhip._lib import ProjFrames, ProjParams, ProjPoints, addr
    rng = np.random.default_rng(513)
    pts, fr = [cloud(rng, 40), cloud(rng, 60)], [features(rng, 50), features(rng, 30)]
    ps, fg = upload(pm, gpu_ctx, pts, fr)
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    out = gpu_ctx.malloc(1 << 16)
    try:
        gpu_ctx.sync()
        before = out.download(np.uint8, (1 << 16,))
        pairs = np.array([[0, 1], [1, 0]], np.int32)
        poses = np.ascontiguousarray(np.stack([I34, I34]))
        zeros, th = np.zeros((2, 3)), np.array([5.0, 5.0])
        s, s2 = S12
        long_off, down_off = np.array([0, 8193], np.int64), np.array([0, 50, 40], np.int64)

        def params(**kw):
            d = dict(fx=256.0, fy=256.0, cx=320.0, cy=240.0, min_x=0.0, max_x=640.0, min_y=0.0, max_y=480.0, cos2_limit=0.25, ratio=0.9,
                     h_scale=addr(s), h_scale2=addr(s2), n_levels=8, th_high=100, level_rule=1, lo=-1, hi=0, pad=0)
            d.update(kw)
            return ProjParams(**d)

        def points(**kw):
            sp = ps._struct(gpu_ctx)
            for k, v in kw.items():
                setattr(sp, k, v)
            return sp

        def frames(**kw):
            sf = fg._struct(gpu_ctx)
            for k, v in kw.items():
                setattr(sf, k, v)
            return sf

        def search(sp=None, sf=None, p=addr(pairs), A=addr(poses), Ow=addr(zeros), t=addr(th), P=2, prm=None, m=out.ptr, c=out.ptr + 4096,
                   tabs=(None,) * 6, ctx=h, no_points=False, no_frames=False, no_params=False):
            sp, sf, prm = sp or points(), sf or frames(), prm or params()
            return lib.slam_proj_match_search(ctx, None if no_points else ctypes.byref(sp), None if no_frames else ctypes.byref(sf), p, A, Ow, t, P,
                                              None if no_params else ctypes.byref(prm), m, c, *tabs)

        o = out.ptr
        bad = [search(ctx=None), search(no_points=True), search(no_frames=True), search(no_params=True), search(p=None), search(A=None),
               search(Ow=None), search(t=None), search(P=4097), search(P=-1), search(m=None), search(c=None),
               search(sp=points(h_offsets=addr(long_off), B=1)), search(sf=frames(h_offsets=addr(down_off), B=2)),
               search(sp=points(d_xyz=None)), search(sp=points(d_desc=None)), search(sf=frames(d_desc=None)), search(sf=frames(d_meta=None)),
               search(sf=frames(cell=0)), search(sf=frames(cell=-16)), search(sf=frames(W=0)),
               search(p=addr(np.array([[0, 2], [0, 0]], np.int32))), search(p=addr(np.array([[-1, 0], [0, 0]], np.int32))),
               search(p=addr(np.array([[2, 0], [0, 0]], np.int32))),
               search(prm=params(lo=1, hi=0)), search(prm=params(n_levels=0)), search(prm=params(n_levels=17)), search(prm=params(h_scale=None)),
               search(prm=params(ratio=float("nan"))), search(t=addr(np.array([5.0, 0.0]))), search(t=addr(np.array([-1.0, 5.0]))),
               search(t=addr(np.array([float("nan"), 5.0]))), search(tabs=(o + 8192, None, None, None, None, None)),
               search(tabs=(None, None, None, None, o + 8192, None)),
               lib.slam_proj_match_project(h, ctypes.byref(points()), addr(pairs[:, 0].copy()), addr(poses), addr(zeros), addr(th), 2,
                                           ctypes.byref(params()), None, None, None, None),
               lib.slam_proj_match_project(h, ctypes.byref(points()), addr(np.array([0, 2], np.int32)), addr(poses), addr(zeros), addr(th), 2,
                                           ctypes.byref(params()), o, o, o, o),
               lib.slam_proj_match_grid(h, o, o, o, None, addr(long_off), 1, 640, 480, 16, *[o] * 7),
               lib.slam_proj_match_grid(h, o, o, o, None, addr(fg.offsets), 2, 640, 480, 0, *[o] * 7),
               lib.slam_proj_match_grid(h, None, o, o, None, addr(fg.offsets), 2, 640, 480, 16, *[o] * 7),
               lib.slam_proj_match_grid(h, o, o, o, None, None, 2, 640, 480, 16, *[o] * 7),
               lib.slam_proj_match_grid(h, o, o, o, None, addr(fg.offsets), 2, 1 << 20, 1 << 20, 1, *[o] * 7)]
        assert bad == [-1] * len(bad)
        for call in (lambda: pm.search_by_projection(ps, fg, [(0, 2)], [I34], ctx=gpu_ctx),
                     lambda: pm.search_by_projection(ps, fg, [(0, 0)], [I34], th=0.0, ctx=gpu_ctx),
                     lambda: pm.search_by_projection(ps, fg, [(0, 0)], [I34], level_offsets=(1, 0), ctx=gpu_ctx),
                     lambda: pm.search_by_projection(ps, fg, [(0, 0)], [I34, I34], ctx=gpu_ctx),
                     lambda: pm.proj_match_arrays(pts[0]["desc"], fr[0]["desc"], np.zeros((40, 2)), fr[0]["xy"], 5.0, C.SIZE, k=3, ctx=gpu_ctx)):
            with pytest.raises(ValueError):
                call()
        gpu_ctx.sync()
        assert np.array_equal(out.download(np.uint8, (1 << 16,)), before)        # nothing was written
        assert gpu_ctx.state_dirty() == 0
        assert search(prm=params(level_rule=0)) == 0                             # the same call with valid arguments succeeds
        want = R.search(pts[0], fr[1], I34, np.zeros(3), 5.0, C.CAMERA, C.BOUNDS, *S12)
        assert np.array_equal(out.download(np.int32, (100,))[:40], want[0])
        assert out.view(4096, 8).download(np.int32, (2,))[0] == want[1]
    finally:
        out.free()
        ps.free()
        fg.free()
    # empty sets are no error
    got = run(pm, gpu_ctx, [cloud(rng, 0), cloud(rng, 9)], [features(rng, 0), features(rng, 9)], [(0, 1), (1, 0), (0, 0)], [I34] * 3, [np.zeros(3)] * 3, 50.0)
    assert [len(m) for m in got[0]] == [0, 9, 0] and got[1].tolist() == [0, 0, 0] and (got[0][1] == -1).all()
    ps, fg = upload(pm, gpu_ctx, [cloud(rng, 3)], [features(rng, 3)])
    try:
        assert pm.search_by_projection(ps, fg, [], np.zeros((0, 3, 4)), ctx=gpu_ctx)[0] == []
    finally:
        ps.free()
        fg.free()


def test_two_runs_give_the_same_bits(pm, gpu_ctx):
    rng = np.random.default_rng(514)
    pts = [cloud(rng, 700, FIELDS), cloud(rng, 300, FIELDS)]
    fr = [features(rng, 900, bins=True, taken=True)]
    fr[0]["desc"][::3] = fr[0]["desc"][0]                                       # mass ties: many equal keys but for the row
    pts[0]["desc"][::2] = fr[0]["desc"][0]
    pairs, poses = [(0, 0), (1, 0), (0, 0)], [C.random_pose(rng, 0.05, 0.1) for _ in range(3)]
    a = run(pm, gpu_ctx, pts, fr, pairs, poses, [np.zeros(3)] * 3, 40.0, ratio=1.0, th_high=256)
    b = run(pm, gpu_ctx, pts, fr, pairs, poses, [np.zeros(3)] * 3, 40.0, ratio=1.0, th_high=256, ref=False, cell=7)
    for p in range(3):
        assert np.array_equal(a[0][p], b[0][p]) and a[1][p] == b[1][p] and all(C.same_bits(a[2][p][k], b[2][p][k]) for k in a[2][p])


# ---- the chain -----------------------------------------------------------------------------------------------------------------

def test_map_to_projection_matches_to_pose(pm, gpu_ctx):
    """A synthetic map seen from a perturbed pose -> search_by_projection -> optimize_pose: the pose from the device's matches
    is the pose from the reference's matches bit for bit, and the projection search hands the refinement more inliers than
    SearchByBoW leaves for the same pair."""
    from backend import Backend
    from slamhip import bow, bow_match
    from test_bow_gpu import random_tree
    rng = np.random.default_rng(515)
    pts, fr, pose, row_of_point = C.make_scene(77, 600, 300)
    first = pose.copy()
    first[:, 3] += rng.normal(0, 0.02, 3)                        # the first estimate: a few pixels off
    fx, fy, cx, cy = C.CAMERA
    P = {k: pts[k] for k in ("xyz", "desc", "range", "normal", "bins")}
    centre = -first[:, :3].T @ first[:, 3]
    want = R.search(P, fr, first, centre, 15.0, C.CAMERA, C.BOUNDS, *S12)
    ps, fg = upload(pm, gpu_ctx, [P], [fr])
    be = Backend()
    try:
        (i1, i2), = be.match_by_projection(ps, fg, [0], [first], fx, fy, cx, cy, th=15.0, centres=[centre])
        got = pm.search_by_projection(ps, fg, [(0, 0)], [first], [centre], C.CAMERA, th=15.0, ctx=gpu_ctx)
    finally:
        ps.free()
        fg.free()
    assert np.array_equal(got[0][0], want[0]) and got[1][0] == want[1]
    r1 = np.flatnonzero(want[0] >= 0).astype(np.int32)
    assert np.array_equal(i1, r1) and np.array_equal(i2, want[0][r1])
    assert len(i1) > 400 and (row_of_point[i1] == i2).mean() > 0.98
    T0 = np.vstack([first, [0, 0, 0, 1]])
    res = be.optimize_pose(T0, pts["xyz"][i1], fr["xy"][i2].astype(np.float64), fx, fy, cx, cy)
    ref = be.optimize_pose(T0, pts["xyz"][r1], fr["xy"][want[0][r1]].astype(np.float64), fx, fy, cx, cy)
    assert C.same_bits(res.pose, ref.pose) and res.n_inliers == ref.n_inliers
    assert np.abs(res.pose[:3] - pose).max() < 1e-2                        # half the perturbation of the first estimate
    # SearchByBoW on the same pair: the map points' descriptors against the frame's through a vocabulary
    tree = random_tree(rng, 6, 4, p_leaf=0.1)
    vocab = bow.Vocabulary.from_arrays(**tree)
    try:
        m, c = bow_match.search_by_bow_descriptors(vocab, pts["desc"], fr["desc"], pts["bins"], fr["bins"], levels_up=2, ctx=gpu_ctx)
    finally:
        vocab.free()
    j1 = np.flatnonzero(m >= 0)
    bow_res = be.optimize_pose(T0, pts["xyz"][j1], fr["xy"][m[j1]].astype(np.float64), fx, fy, cx, cy) if len(j1) >= 3 else None
    assert res.n_inliers > (bow_res.n_inliers if bow_res is not None else 0)
