"""The fusion search and the map-point refresh on the device against tests/fuse_ref.py bit for bit on every
output, at the smallest shapes where each path can go wrong, on the cases that tell Fuse from SearchByProjection, and as the
chain new points -> fuse -> merge -> refresh -> projection search."""
import ctypes

import numpy as np
import pytest

import fuse_cases as C
import fuse_ref as F

pytestmark = pytest.mark.gpu

INF_BOUNDS = (-np.inf, np.inf, -np.inf, np.inf)
UNIT = (1.0, 1.0, 0.0, 0.0)


@pytest.fixture(scope="module")
def fz(built):
    from slamhip import fuse as module
    return module


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def cat(dicts, key, tail, dtype):
    parts = [np.asarray(d[key], dtype).reshape((-1,) + tail) for d in dicts]
    return np.concatenate(parts) if parts else np.zeros((0,) + tail, dtype)


def run(fz, ctx, sets, frames, lists, pairs, poses, centres, camera=C.CAMERA, size=C.SIZE, cell=16, **kw):
    """``fuse_points`` for point-set dicts and frame dicts; returns (results, counts)."""
    from slamhip import FrameGrids, PointSets
    off1 = np.concatenate([[0], np.cumsum([len(s["id"]) for s in sets])]).astype(np.int64)
    off2 = np.concatenate([[0], np.cumsum([len(f["level"]) for f in frames])]).astype(np.int64)
    has = lambda k: bool(sets) and sets[0].get(k) is not None  # noqa: E731
    rng = cat(sets, "range", (2,), np.float64) if has("range") else None
    ps = PointSets(cat(sets, "xyz", (3,), np.float64), cat(sets, "desc", (32,), np.uint8), off1, dmin2=None if rng is None else rng[:, 0],
                   dmax2=None if rng is None else rng[:, 1], normal=cat(sets, "normal", (3,), np.float64) if has("normal") else None,
                   level=cat(sets, "level", (), np.int64) if has("level") else None, ctx=ctx)
    fr = ob = None
    try:
        fr = FrameGrids.from_arrays(cat(frames, "desc", (32,), np.uint8), cat(frames, "xy", (2,), np.float32), cat(frames, "level", (), np.int64),
                                    size, off2, cell=cell, ctx=ctx)
        ob = fz.MapObservations.from_lists(lists, ctx)
        return fz.fuse_points(ps, cat(sets, "id", (), np.int64), fr, cat(frames, "point", (), np.int64), ob, pairs, poses, centres, camera=camera,
                              scale=(C.SCALE, C.SCALE2), return_tables=True, ctx=ctx, **kw)
    finally:
        for x in (ps, fr, ob):
            if x is not None:
                x.free()


def same(got, want, count=None):
    for k in ("row", "dist", "status", "other", "lp"):
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    assert np.array_equal(bits(got["u"]), bits(want["u"])) and np.array_equal(bits(got["v"]), bits(want["v"]))
    if count is not None:
        assert np.array_equal(count, want["count"])


def flat(fz, ctx, points, frames, lists, pairs, th=3.0, **kw):
    """Device and reference for hand-built points and frames under the identity pose and the unit camera; the two agree."""
    P = len(pairs)
    res, cnt = run(fz, ctx, [points], frames, lists, pairs, np.broadcast_to(C.I34, (P, 3, 4)), np.zeros((P, 3)), camera=UNIT, bounds=INF_BOUNDS,
                   th=th, **kw)
    ref_kw = {("offsets" if k == "level_offsets" else k): v for k, v in kw.items()}
    for (a, b), r, c in zip(pairs, res, cnt):
        same(r, F.search(points, frames[b], b, lists, C.I34, np.zeros(3), th, UNIT, INF_BOUNDS, C.SCALE, C.SCALE2, **ref_kw), c)
    return res, cnt


# ---- shapes -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def W():
    return C.world(21, 65, n_frames=3, n_dup=5, n_clutter=10)


def world_case(W):
    """Sets of 0, 1, 63, 64 and 65 points; the world's three frames, an empty frame and a frame of one row."""
    idx = [np.arange(0), np.arange(3, 4), np.arange(63), np.arange(2, 66), np.arange(5, 70)]
    sets = [C.subset(W["pts"], i) for i in idx]
    f1 = W["frames"][1]
    r = int(W["row_of"][1][60])
    frames = W["frames"] + [C.flat_frame(np.zeros((0, 2)), [], np.zeros((0, 32))),
                            dict(desc=f1["desc"][r:r + 1], xy=f1["xy"][r:r + 1], level=f1["level"][r:r + 1], point=np.array([-1], np.int32))]
    poses = np.concatenate([W["poses"], W["poses"][[1, 1]]])
    centres = np.concatenate([W["centres"], W["centres"][[1, 1]]])
    pairs = [(0, 1), (1, 1), (2, 1), (3, 1), (4, 1), (4, 3), (4, 4), (0, 3), (4, 0), (2, 2)]
    return idx, sets, frames, poses, centres, pairs


def world_ref(W, sets, frames, poses, centres, pairs, **kw):
    return [F.search(sets[a], frames[b], b, W["lists"], poses[b], centres[b], kw.get("th", 3.0), C.CAMERA, C.BOUNDS, C.SCALE, C.SCALE2)
            for a, b in pairs]


def test_set_and_frame_sizes_against_the_reference_and_the_construction(fz, gpu_ctx, W):
    idx, sets, frames, poses, centres, pairs = world_case(W)
    res, cnt = run(fz, gpu_ctx, sets, frames, W["lists"], pairs, poses[[b for _, b in pairs]], centres[[b for _, b in pairs]])
    want = world_ref(W, sets, frames, poses, centres, pairs)
    for (a, b), r, c, w in zip(pairs, res, cnt, want):
        same(r, w, c)
        assert len(r["row"]) == len(idx[a]) and r["frame"] == b and np.array_equal(r["id"], idx[a])
        if b < 3:                                        # the world's own frames: the answer is known by construction
            st, row, ot = C.expected(W, idx[a], b)
            assert np.array_equal(r["status"], st) and np.array_equal(r["row"], row) and np.array_equal(r["other"], ot)
    assert cnt[0].tolist() == [0, 0, 0] and cnt[5].tolist() == [0, 0, 0] and (res[5]["status"] == 6).all()
    assert cnt[6].sum() == 1 and (res[6]["status"] == 0).sum() == 1          # the one-row frame: landmark 60 finds its row
    assert cnt[:, 1].sum() > 0 and cnt[:, 0].sum() > 0 and (res[4]["status"] == 5).any()


def test_cell_sizes_and_runs_give_equal_bits(fz, gpu_ctx, W):
    idx, sets, frames, poses, centres, pairs = world_case(W)
    shared = [(2, 1), (3, 1), (4, 1)]                    # three pairs sharing a frame
    A, O = poses[[1, 1, 1]], centres[[1, 1, 1]]
    first = run(fz, gpu_ctx, sets, frames, W["lists"], shared, A, O, cell=16)
    for cell in (16, 1, 1000):
        res, cnt = run(fz, gpu_ctx, sets, frames, W["lists"], shared, A, O, cell=cell)
        assert np.array_equal(cnt, first[1])
        for r, r0 in zip(res, first[0]):
            same(r, r0)
    alone = run(fz, gpu_ctx, sets, frames, W["lists"], [(3, 1)], A[:1], O[:1])
    same(alone[0][0], first[0][1])
    assert np.array_equal(alone[1][0], first[1][1])


def test_sim3_pose_and_margins(fz, gpu_ctx, W):
    """[sR | t] with s = 2 and the centre given: the distances double, the default margins (0.64, 1.44) put most points out of
    range, margins of (0.1, 9) keep them; both as the reference says."""
    idx, sets, frames, poses, centres, pairs = world_case(W)
    S = poses[1].copy()
    S *= 2.0
    for margins in ((0.64, 1.44), (0.1, 9.0), (1.0, 1.0)):
        res, cnt = run(fz, gpu_ctx, sets, frames, W["lists"], [(4, 1)], S[None], centres[1][None], margins=margins)
        want = F.search(sets[4], frames[1], 1, W["lists"], S, centres[1], 3.0, C.CAMERA, C.BOUNDS, C.SCALE, C.SCALE2, margins=margins)
        same(res[0], want, cnt[0])
        assert ((res[0]["status"] == 3).sum() > 5) == (margins != (0.1, 9.0))


def test_backend_search_in_neighbors_is_the_four_steps(fz, gpu_ctx):
    """Both directions in one call, the merge, the refresh of the survivors whose lists changed, and their PointSets."""
    from backend import Backend
    from slamhip import FrameGrids, PointSets
    Wd = C.world(31, 70, n_frames=3, n_dup=8, n_clutter=15)
    sets = C.keyframe_sets(Wd)
    ps_d = [C.subset(Wd["pts"], i) for i in sets]
    fr_d = Wd["frames"]
    off1 = np.concatenate([[0], np.cumsum([len(i) for i in sets])]).astype(np.int64)
    off2 = np.concatenate([[0], np.cumsum([len(f["level"]) for f in fr_d])]).astype(np.int64)
    rng = cat(ps_d, "range", (2,), np.float64)
    ps = PointSets(cat(ps_d, "xyz", (3,), np.float64), cat(ps_d, "desc", (32,), np.uint8), off1, dmin2=rng[:, 0], dmax2=rng[:, 1],
                   normal=cat(ps_d, "normal", (3,), np.float64), ctx=gpu_ctx)
    fr = FrameGrids.from_arrays(cat(fr_d, "desc", (32,), np.uint8), cat(fr_d, "xy", (2,), np.float32), cat(fr_d, "level", (), np.int64), C.SIZE, off2,
                                ctx=gpu_ctx)
    ob = fz.MapObservations.from_lists(Wd["lists"], gpu_ctx)
    out = None
    try:
        out = Backend().search_in_neighbors(ps, np.concatenate(sets), fr, cat(fr_d, "point", (), np.int64), ob, Wd["pts"]["xyz"], 0, [1, 2],
                                            Wd["poses"], *C.CAMERA, scale=(C.SCALE, C.SCALE2))
        pairs = [(0, 1), (0, 2), (1, 0), (2, 0)]
        want = [dict(C.ref_pair(F, Wd, sets, a, b), id=sets[a], frame=b) for a, b in pairs]
        assert np.array_equal(out["counts"], np.stack([w["count"] for w in want]))
        lists, alias, upd = F.apply_fusion(Wd["lists"], want)
        assert out["observations"].lists() == [list(map(tuple, x)) for x in lists] and out["alias"].tolist() == alias
        assert [tuple(u) for u in out["updates"].tolist()] == upd
        # the eight duplicates of frame 0 merge into their originals, which gain frame 0; points seen in 0 gain the neighbours
        M0 = Wd["n_land"]
        assert alias[M0:] == list(range(8)) and all(len(lists[m]) == 3 for m in range(8)) and all(lists[m] == [] for m in range(M0, M0 + 8))
        touched = out["touched"]
        assert set(range(8)) <= set(touched.tolist()) and len(touched) > 20 and len(out["points"]) == 1 and out["points"].n == len(touched)
        same_refresh(out["refresh"], F.refresh(Wd["pts"]["xyz"], lists, [f["desc"] for f in fr_d], [f["level"] for f in fr_d], Wd["centres"],
                                               C.SCALE, None, touched))
    finally:
        for x in (ps, fr, ob, out and out["observations"], out and out["points"]):
            if x:
                x.free()


# ---- what tells Fuse from SearchByProjection ---------------------------------------------------------------------------------

def test_nearest_descriptor_outside_chi2_loses_to_the_farther_one(fz, gpu_ctx):
    pts = C.flat_points([[100.0, 100.0]], [C.ones(0)])
    fr = C.flat_frame([[102.5, 100.0], [101.0, 100.0]], [0, 0], [C.ones(2), C.ones(10)])
    res, _ = flat(fz, gpu_ctx, pts, [fr], [[]], [(0, 0)], chi2=5.99)         # e2 = 6.25 > 5.99: row 0 is no candidate
    assert (res[0]["row"][0], res[0]["dist"][0], res[0]["status"][0]) == (1, 10, 0)
    res, _ = flat(fz, gpu_ctx, pts, [fr], [[]], [(0, 0)], chi2=6.25)         # at equality it is kept, and nearer
    assert (res[0]["row"][0], res[0]["dist"][0]) == (0, 2)
    lv = C.flat_frame([[102.5, 100.0], [101.0, 100.0]], [1, 0], [C.ones(2), C.ones(10)])     # on level 1 the bound is 5.99 * 1.44
    res, _ = flat(fz, gpu_ctx, pts, [lv], [[]], [(0, 0)], chi2=5.99, level_offsets=(0, 1))
    assert res[0]["row"][0] == 0


def test_a_row_holding_a_map_point_is_the_one_found(fz, gpu_ctx):
    """search_by_projection hides a taken row; Fuse finds it and names its holder."""
    from slamhip import FrameGrids, PointSets, search_by_projection
    pts = C.flat_points([[50.0, 60.0], [200.0, 60.0]], [C.ones(0), C.ones(8)], ids=[3, 4])
    fr = C.flat_frame([[50.5, 60.0], [200.0, 60.5]], [0, 0], [C.ones(3), C.ones(9)], point=[7, -1])
    res, cnt = flat(fz, gpu_ctx, pts, [fr], [[] for _ in range(8)], [(0, 0)])
    assert res[0]["row"].tolist() == [0, 1] and res[0]["other"].tolist() == [7, -1] and cnt[0].tolist() == [1, 1, 0]
    ps = PointSets(pts["xyz"], pts["desc"], level=pts["level"], ctx=gpu_ctx)
    g = FrameGrids.from_arrays(fr["desc"], fr["xy"], fr["level"], C.SIZE, taken=fr["point"] >= 0, ctx=gpu_ctx)
    try:
        m, _ = search_by_projection(ps, g, [(0, 0)], C.I34[None], np.zeros((1, 3)), bounds=INF_BOUNDS, scale=(C.SCALE, C.SCALE2), th=3.0, ctx=gpu_ctx)
    finally:
        ps.free()
        g.free()
    assert m[0].tolist() == [-1, 1]


def test_status_5_only_for_the_pair_whose_frame_is_in_the_list(fz, gpu_ctx):
    pts = C.flat_points([[50.0, 60.0], [80.0, 60.0]], [C.ones(0), C.ones(0)], ids=[0, -1])
    fr = C.flat_frame([[50.5, 60.0], [80.0, 60.5]], [0, 0], [C.ones(3), C.ones(4)])
    lists = [[(1, 0), (2, 5)]]                           # point 0 is seen in frames 1 and 2; a point without an id is never skipped
    res, cnt = flat(fz, gpu_ctx, pts, [fr, fr, fr, fr], lists, [(0, 0), (0, 1), (0, 2), (0, 3)])
    assert [r["status"].tolist() for r in res] == [[0, 0], [5, 0], [5, 0], [0, 0]]
    assert res[1]["row"][0] == -1 and np.isnan(res[1]["u"][0]) and res[1]["lp"][0] == -1


def test_a_contested_row_goes_to_the_smallest_distance_then_point(fz, gpu_ctx):
    pts = C.flat_points([[50.0, 60.0], [51.0, 60.0], [50.0, 61.0]], [C.ones(6), C.ones(2), C.ones(2)], ids=[40, 41, 42])
    fr = C.flat_frame([[50.5, 60.5]], [0], [C.ones(0)], point=[9])
    res, cnt = flat(fz, gpu_ctx, pts, [fr], [[] for _ in range(43)], [(0, 0)])
    assert res[0]["status"].tolist() == [8, 0, 8] and res[0]["other"].tolist() == [41, 9, 41]
    assert res[0]["row"].tolist() == [0, 0, 0] and res[0]["dist"].tolist() == [6, 2, 2] and cnt[0].tolist() == [0, 1, 2]


def test_level_offsets(fz, gpu_ctx):
    pts = C.flat_points([[50.0, 60.0]], [C.ones(0)])
    fr = C.flat_frame([[50.5, 60.0]], [2], [C.ones(1)])
    assert flat(fz, gpu_ctx, pts, [fr], [[]], [(0, 0)])[0][0]["status"].tolist() == [6]                       # (-1, 0) about level 0
    assert flat(fz, gpu_ctx, pts, [fr], [[]], [(0, 0)], level_offsets=(0, 1))[0][0]["status"].tolist() == [6]
    assert flat(fz, gpu_ctx, pts, [fr], [[]], [(0, 0)], level_offsets=(0, 2))[0][0]["status"].tolist() == [0]
    assert flat(fz, gpu_ctx, pts, [fr], [[]], [(0, 0)], level_offsets=(2, 2))[0][0]["row"].tolist() == [0]


def test_th_low_at_50_and_51(fz, gpu_ctx):
    pts = C.flat_points([[50.0, 60.0], [90.0, 60.0]], [C.ones(0), C.ones(0)])
    fr = C.flat_frame([[50.5, 60.0], [90.5, 60.0]], [0, 0], [C.ones(50), C.ones(51)])
    res, cnt = flat(fz, gpu_ctx, pts, [fr], [[], []], [(0, 0)])
    assert res[0]["status"].tolist() == [0, 7] and res[0]["row"].tolist() == [0, 1] and res[0]["dist"].tolist() == [50, 51]
    assert res[0]["other"].tolist() == [-1, -1] and cnt[0].tolist() == [1, 0, 0]
    res, cnt = flat(fz, gpu_ctx, pts, [fr], [[], []], [(0, 0)], th_low=51)
    assert res[0]["status"].tolist() == [0, 0] and cnt[0].tolist() == [2, 0, 0]


def test_fuse_arrays_is_the_candidate_rule(fz, gpu_ctx):
    rng = np.random.default_rng(8)
    q, t = rng.integers(0, 256, (65, 32), dtype=np.uint8), rng.integers(0, 256, (130, 32), dtype=np.uint8)
    uv = rng.uniform(0, 100, (65, 2))
    txy = rng.uniform(0, 100, (130, 2)).astype(np.float32)
    lv = rng.integers(0, 8, 130)
    row, dist = fz.fuse_arrays(q, t, uv, txy, lv, 5.0, (100, 100), scale=(C.SCALE, C.SCALE2), chi2=20.0, ctx=gpu_ctx)
    pts = C.flat_points(uv, q, ids=np.full(65, -1))
    want = F.search(pts, C.flat_frame(txy, lv, t), 0, [], C.I34, np.zeros(3), 5.0, UNIT, INF_BOUNDS, C.SCALE, C.SCALE2, th_low=256, chi2=20.0,
                    offsets=(0, 16))
    assert np.array_equal(row, want["row"]) and np.array_equal(dist, want["dist"]) and (row >= 0).sum() > 20 and (row < 0).sum() >= 5


# ---- the refresh ------------------------------------------------------------------------------------------------------------------

LENGTHS = (0, 1, 2, 3, 4, 31, 32, 33, 64, 255, 256)


@pytest.fixture(scope="module")
def many():
    """About 300 map points with lists of every length of LENGTHS over 256 frames of 4 rows, descriptors in clusters so that
    medians tie."""
    rng = np.random.default_rng(13)
    B = 256
    seeds = rng.integers(0, 256, (6, 32), dtype=np.uint8)
    desc = [C.flip_bits(rng, seeds[rng.integers(0, 6, 4)], 5) for _ in range(B)]
    level = [rng.integers(0, 8, 4) for _ in range(B)]
    centres = rng.normal(0, 1, (B, 3))
    lens = [LENGTHS[i % len(LENGTHS)] for i in range(297)]
    lists = [[(int(f), int(rng.integers(0, 4))) for f in np.sort(rng.choice(B, n, replace=False))] for n in lens]
    xyz = rng.normal(0, 1, (297, 3)) + np.array([0, 0, 8.0])
    xyz[5] = centres[lists[5][2][0]]                     # a view of length zero (N = 31)
    xyz[16] = np.nan
    ref = np.array([rng.integers(0, max(n, 1)) for n in lens])
    return dict(desc=desc, level=level, centres=centres, lists=lists, xyz=xyz, ref=ref, lens=lens)


def frames_of(ctx, desc, level):
    from slamhip import FrameGrids
    off = np.concatenate([[0], np.cumsum([len(x) for x in level])]).astype(np.int64)
    n = int(off[-1])
    xy = np.random.default_rng(1).uniform(0, 600, (n, 2)).astype(np.float32)       # (the grid order differs from the row order)
    return FrameGrids.from_arrays(np.concatenate(desc), xy, np.concatenate(level), C.SIZE, off, ctx=ctx)


def same_refresh(got, want):
    assert np.array_equal(got["best"], want["best"]) and np.array_equal(got["descriptors"], want["descriptors"])
    for k in ("normal", "dmin2", "dmax2"):
        assert np.array_equal(bits(got[k]), bits(want[k])), k


def test_refresh_mixed_list_lengths_in_one_call(fz, gpu_ctx, many):
    fr = frames_of(gpu_ctx, many["desc"], many["level"])
    ob = fz.MapObservations.from_lists(many["lists"], gpu_ctx)
    try:
        got = fz.refresh_map_points(many["xyz"], ob, fr, many["centres"], many["ref"], (C.SCALE, C.SCALE2), ctx=gpu_ctx)
        want = F.refresh(many["xyz"], many["lists"], many["desc"], many["level"], many["centres"], C.SCALE, many["ref"])
        same_refresh(got, want)
        again = fz.refresh_map_points(many["xyz"], ob, fr, many["centres"], many["ref"], (C.SCALE, C.SCALE2), ctx=gpu_ctx)
        same_refresh(again, got)
        lens = np.array(many["lens"])
        assert (got["best"][lens == 0] == -1).all() and not got["descriptors"][lens == 0].any() and np.isnan(got["normal"][lens == 0]).all()
        assert (got["best"][lens > 0] >= 0).all() and (got["best"] < np.maximum(lens, 1)).all()
        for m in (5, 16):                                # a zero length, a NaN position: the descriptor is still chosen
            assert np.isnan(got["normal"][m]).all() and np.isnan(got["dmin2"][m]) and np.isnan(got["dmax2"][m]) and got["best"][m] >= 0
        ok = (lens > 0) & ~np.isin(np.arange(297), (5, 16))
        assert np.abs(np.linalg.norm(got["normal"][ok], axis=1) - 1).max() < 1e-12 and (got["dmin2"][ok] < got["dmax2"][ok]).all()
        sel = np.array([296, 10, 9, 0, 43, 10])          # a selection, out of order and with a repeat; no reference indices
        part = fz.refresh_map_points(many["xyz"], ob, fr, many["centres"], None, (C.SCALE, C.SCALE2), select=sel, ctx=gpu_ctx)
        same_refresh(part, F.refresh(many["xyz"], many["lists"], many["desc"], many["level"], many["centres"], C.SCALE, None, sel))
        none = fz.refresh_map_points(many["xyz"], ob, fr, many["centres"], select=[], ctx=gpu_ctx)
        assert len(none["best"]) == 0
    finally:
        fr.free()
        ob.free()


def test_a_list_of_257_is_rejected_and_nothing_runs(fz, gpu_ctx, many):
    from slamhip._lib import SLAM_ERR_INVALID, addr
    with pytest.raises(ValueError):
        fz.MapObservations.from_lists([[(b, 0) for b in range(257)]])
    off, foff, s = np.array([0, 2, 259], np.int64), np.array([0, 4], np.int64), np.ones(8)
    rc = gpu_ctx.lib.slam_fuse_refresh(gpu_ctx.handle, None, addr(off), None, 2, None, 2, None, None, None, addr(foff), 1, None, None, addr(s), 8,
                                       None, None, None, None)
    assert rc == SLAM_ERR_INVALID
    off = np.array([0, 3, 2], np.int64)                  # descending
    rc = gpu_ctx.lib.slam_fuse_refresh(gpu_ctx.handle, None, addr(off), None, 2, None, 2, None, None, None, addr(foff), 1, None, None, addr(s), 8,
                                       None, None, None, None)
    assert rc == SLAM_ERR_INVALID
    fr = frames_of(gpu_ctx, many["desc"][:2], many["level"][:2])             # the context is usable afterwards
    ob = fz.MapObservations.from_lists([[(0, 1), (1, 2)]], gpu_ctx)
    try:
        got = fz.refresh_map_points([[0.0, 0.0, 5.0]], ob, fr, many["centres"][:2], ctx=gpu_ctx)
        same_refresh(got, F.refresh([[0.0, 0.0, 5.0]], [[(0, 1), (1, 2)]], many["desc"], many["level"], many["centres"], C.SCALE))
        with pytest.raises(ValueError):                  # an observation outside the frames
            bad = fz.MapObservations.from_lists([[(0, 4)]], gpu_ctx)
            fz.refresh_map_points([[0.0, 0.0, 5.0]], bad, fr, many["centres"][:2], ctx=gpu_ctx)
    finally:
        fr.free()
        ob.free()


def test_invalid_search_arguments_launch_nothing(fz, gpu_ctx, W):
    from slamhip import FrameGrids, PointSets
    from slamhip._lib import SLAM_ERR_INVALID, FuseParams, addr
    from slamhip.proj_match import _params
    s = C.subset(W["pts"], np.arange(10))
    f = W["frames"][1]
    ps = PointSets(s["xyz"], s["desc"], dmin2=s["range"][:, 0], dmax2=s["range"][:, 1], normal=s["normal"], ctx=gpu_ctx)
    fr = FrameGrids.from_arrays(f["desc"], f["xy"], f["level"], C.SIZE, ctx=gpu_ctx)
    ob = fz.MapObservations.from_lists(W["lists"], gpu_ctx)
    m = [gpu_ctx.upload(np.ascontiguousarray(s["id"], np.int32)), gpu_ctx.upload(np.ascontiguousarray(f["point"], np.int32))]
    out = [gpu_ctx.malloc(64) for _ in range(5)]
    try:
        prm, keep = _params(C.CAMERA, C.BOUNDS, (C.SCALE, C.SCALE2), 0, 0.0, 0.25, True, -1, 0)
        sp, sf, dev = ps._struct(gpu_ctx), fr._struct(gpu_ctx), ob._resident(gpu_ctx)
        pair, A, O, th = np.array([[0, 0]], np.int32), np.ascontiguousarray(W["poses"][1:2]), np.ascontiguousarray(W["centres"][1:2]), np.array([3.0])

        def call(fp, pair=pair, th=th, off=ob.offsets, row=out[0].ptr):
            return gpu_ctx.lib.slam_fuse_search(gpu_ctx.handle, ctypes.byref(sp), m[0].ptr, ctypes.byref(sf), m[1].ptr, addr(off), dev["offsets"].ptr,
                                                dev["obs"].ptr, len(off) - 1, addr(pair), addr(A), addr(O), addr(th), 1, ctypes.byref(prm),
                                                ctypes.byref(fp), row, out[1].ptr, out[2].ptr, out[3].ptr, out[4].ptr, None, None, None)

        good = FuseParams(0.64, 1.44, 5.99, 50, 0)
        for bad in (FuseParams(np.nan, 1.44, 5.99, 50, 0), FuseParams(0.64, 0.0, 5.99, 50, 0), FuseParams(-1.0, 1.0, 5.99, 50, 0),
                    FuseParams(0.64, 1.44, np.nan, 50, 0), FuseParams(0.64, 1.44, 5.99, 257, 0)):
            assert call(bad) == SLAM_ERR_INVALID
        assert call(good, pair=np.array([[0, 1]], np.int32)) == SLAM_ERR_INVALID       # a pair outside the sets
        assert call(good, th=np.array([0.0])) == SLAM_ERR_INVALID
        bad_off = ob.offsets.copy()
        bad_off[3] = bad_off[2] - 1
        assert call(good, off=bad_off) == SLAM_ERR_INVALID                              # descending offsets
        assert call(good, row=None) == SLAM_ERR_INVALID
        assert call(good) == 0
        gpu_ctx.sync()
        want = F.search(s, f, 0, W["lists"], W["poses"][1], W["centres"][1], 3.0, C.CAMERA, C.BOUNDS, C.SCALE, C.SCALE2)
        assert np.array_equal(out[2].download(np.int32, (10,)), want["status"]) and np.array_equal(out[4].download(np.int32, (3,)), want["count"])
        del keep
    finally:
        for x in (ps, fr, ob, *m, *out):
            x.free()


# ---- two observations: the triangulation's own normal and range ------------------------------------------------------------

@pytest.fixture(scope="module")
def created(built, gpu_ctx):
    """Two keyframes of 200 rows seeing 150 common points, a third frame, and the points create_new_map_points makes."""
    import tri_match_cases as TC
    from slamhip import FeatureVectors, tri_match as tm
    s1, s2, s3, truth = TC.make_scene(3, 150, 200)
    off = np.array([0, 200, 400], np.int64)
    fv = FeatureVectors.from_nodes(np.concatenate([s1["desc"], s2["desc"]]), np.concatenate([s1["nodes"], s2["nodes"]]).astype(np.int64), off,
                                   ctx=gpu_ctx)
    v = tm.KeyframeViews(np.concatenate([s1["xy"], s2["xy"]]), np.concatenate([s1["level"], s2["level"]]).astype(np.int64), None, gpu_ctx)
    try:
        pts, _, _ = tm.create_new_map_points(fv, fv, [(0, 1)], v, v, TC.POSES[0][None], TC.POSES[1][None], TC.CAMERA, (TC.SCALE, TC.SIGMA2),
                                             ctx=gpu_ctx)
    finally:
        fv.free()
        v.free()
    d = pts[0]
    rows1 = np.flatnonzero(d["status"] == 0)
    return dict(s=(s1, s2, s3), truth=truth, d=d, rows1=rows1, rows2=d["matches12"][rows1], TC=TC)


def test_two_observation_refresh_equals_the_triangulation(fz, gpu_ctx, created):
    from slamhip.proj_match import camera_centres
    TC, (s1, s2, s3), d, rows1, rows2 = created["TC"], created["s"], created["d"], created["rows1"], created["rows2"]
    assert len(rows1) > 100
    fr = frames_of(gpu_ctx, [s1["desc"], s2["desc"]], [s1["level"], s2["level"]])
    ob = fz.MapObservations.from_lists([[(0, int(a)), (1, int(b))] for a, b in zip(rows1, rows2)], gpu_ctx)
    try:
        got = fz.refresh_map_points(d["X"][rows1], ob, fr, camera_centres(np.stack(TC.POSES[:2])), scale=(TC.SCALE, TC.SIGMA2), ctx=gpu_ctx)
    finally:
        fr.free()
        ob.free()
    for k in ("normal", "dmin2", "dmax2"):
        assert np.array_equal(bits(got[k]), bits(d[k][rows1])), k
    assert (got["best"] == 0).all() and np.array_equal(got["descriptors"], s1["desc"][rows1])     # medians 0 and 0: the first


def test_new_points_fused_merged_refreshed_and_found_by_projection(fz, gpu_ctx, created):
    """create_new_map_points -> fuse_points into the third keyframe -> apply_fusion -> refresh_map_points -> search_by_projection:
    every created point is fused at its landmark's row, and the projection search finds every fused point at that row - but for
    exactly the points the numpy gates of 4l put out of range (they have no margin) under the refreshed ranges."""
    import proj_match_ref as PR
    from slamhip import FrameGrids, PointSets, search_by_projection
    from slamhip.proj_match import camera_centres
    TC, (s1, s2, s3), d, rows1, rows2, truth = created["TC"], created["s"], created["d"], created["rows1"], created["rows2"], created["truth"]
    K = len(rows1)
    sides = [s1, s2, s3]
    scale = (TC.SCALE, TC.SIGMA2)
    lists = [[(0, int(a)), (1, int(b))] for a, b in zip(rows1, rows2)]
    holder = [np.full(200, -1, np.int32) for _ in range(3)]
    holder[0][rows1] = np.arange(K)
    holder[1][rows2] = np.arange(K)
    off = np.array([0, 200, 400, 600], np.int64)
    fr = FrameGrids.from_arrays(np.concatenate([s["desc"] for s in sides]), np.concatenate([s["xy"] for s in sides]),
                                np.concatenate([s["level"] for s in sides]).astype(np.int64), TC.SIZE, off, ctx=gpu_ctx)
    ps = PointSets(d["X"][rows1], s1["desc"][rows1], dmin2=d["dmin2"][rows1], dmax2=d["dmax2"][rows1], normal=d["normal"][rows1], ctx=gpu_ctx)
    ob = fz.MapObservations.from_lists(lists, gpu_ctx)
    new = ps2 = None
    try:
        res, cnt = fz.fuse_points(ps, np.arange(K), fr, np.concatenate(holder), ob, [(0, 2), (0, 0)], np.stack([TC.POSES[2], TC.POSES[0]]),
                                  camera=TC.CAMERA, scale=scale, th=4.0, ctx=gpu_ctx)
        assert (res[1]["status"] == 5).all() and cnt[1].tolist() == [0, 0, 0]   # keyframe 1 sees them all already
        fused = np.flatnonzero(res[0]["status"] == 0)
        point_of_row1 = np.full(200, -1)
        point_of_row1[truth["rows1"]] = np.arange(150)
        land = point_of_row1[rows1[fused]]
        right = (land >= 0) & (res[0]["row"][fused] == truth["rows3"][np.maximum(land, 0)])
        print("created %d, fused %d into the third keyframe, %d at the landmark's row" % (K, len(fused), right.sum()))
        assert len(fused) == K and right.all() and cnt[0].tolist() == [K, 0, 0]
        new, alias, upd = fz.apply_fusion(ob, res)
        assert np.array_equal(alias, np.arange(K)) and new.nobs[fused].tolist() == [3] * len(fused) and new.nnz == 2 * K + len(fused)
        assert np.array_equal(upd, np.stack([np.full(len(fused), 2), res[0]["row"][fused], fused], 1)[np.argsort(res[0]["row"][fused])])
        ref = fz.refresh_map_points(d["X"][rows1], new, fr, camera_centres(np.stack(TC.POSES)), scale=scale, select=fused, ctx=gpu_ctx)
        same_refresh(ref, F.refresh(d["X"][rows1], new.lists(), [s["desc"] for s in sides], [s["level"] for s in sides],
                                    camera_centres(np.stack(TC.POSES)), TC.SCALE, None, fused))
        assert np.array_equal(bits(ref["dmax2"]), bits(d["dmax2"][rows1][fused]))             # the reference keyframe is still the first
        ps2 = PointSets(d["X"][rows1][fused], ref["descriptors"], dmin2=ref["dmin2"], dmax2=ref["dmax2"], normal=ref["normal"], ctx=gpu_ctx)
        m13, _, tabs = search_by_projection(ps2, fr, [(0, 2)], TC.POSES[2][None], camera=TC.CAMERA, scale=scale, th=4.0, ratio=np.inf,
                                            return_tables=True, ctx=gpu_ctx)
        O3 = camera_centres(TC.POSES[2][None])[0]
        st, u, v, lp, _ = PR.gates(d["X"][rows1][fused], TC.POSES[2], O3, 4.0, TC.CAMERA, (0.0, float(TC.SIZE[0]), 0.0, float(TC.SIZE[1])), TC.SCALE,
                                   TC.SIGMA2, np.stack([ref["dmin2"], ref["dmax2"]], 1), ref["normal"])
        assert np.array_equal(tabs[0]["status"], st) and np.array_equal(tabs[0]["lp"], lp)
        assert np.array_equal(bits(tabs[0]["u"]), bits(u)) and np.array_equal(bits(tabs[0]["v"]), bits(v))
        searched = st == 0
        print("searched %d of the %d fused points by projection, %d out of range" % (searched.sum(), len(fused), (st == 3).sum()))
        assert set(st.tolist()) == {0, 3} and searched.sum() > (st == 3).sum() > 0
        assert np.array_equal(m13[0], np.where(searched, res[0]["row"][fused], -1))            # every one of them, at its row
        again, cnt2 = fz.fuse_points(ps, np.arange(K), fr, np.concatenate(holder), new, [(0, 2)], TC.POSES[2][None], camera=TC.CAMERA,
                                     scale=scale, th=4.0, ctx=gpu_ctx)
        assert (again[0]["status"] == 5).all() and cnt2[0].tolist() == [0, 0, 0]              # the new table knows the third keyframe
    finally:
        for x in (fr, ps, ob, new, ps2):
            if x is not None:
                x.free()
