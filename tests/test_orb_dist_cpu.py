"""CPU: the numpy statement of the quadtree keypoint distribution (tests/orb_dist_ref.py) against answers derived
by hand on dot images (tests/orb_dist_cases.py), its invariants on real and procedural images, and the host-side pieces of the
product that need no device: OrbParams validation, the workspace query, the header entries.

The zero-gain case stands on a 165 x 165 level, not on the 145 x 65 one of the other dot cases: two dots two pixels apart are
parted as soon as their node is at most two pixels wide, a node that is cut k times without parting them is wider than two, and
with the halves cut at ceil(width / 2) that takes a root wider than 2^(k+1); six such rounds need more than 128 scoreable pixels.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import orb_cases as C
import orb_dist_cases as D
import orb_dist_ref as dref
import orb_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = {c.name: c for c in D.cases()}


def run(case, trace=None):
    """[(x, y)] of one level of the statement, its R, and the candidate list it started from."""
    img = case.img
    scores = ref.fast_scores(img, case.t_min)
    R, ys, xs = ref.candidates(img, case.t_min)
    keep = dref.select(R, ys, xs, scores, img.shape[0], img.shape[1], case.quota, case.t_ini, trace)
    return list(zip(xs[keep].tolist(), ys[keep].tolist())), R[keep].tolist(), (R, ys, xs)


# ---------------------------------------------------------------------------------------------------------- hand-derived
@pytest.mark.parametrize("name", list(CASES))
def test_hand_made_case(name):
    case = CASES[name]
    got, R, _ = run(case)
    assert got == case.want
    if case.harris is not None:
        Rh, ys, xs = ref.candidates(case.img, case.t_ini)
        keep = ref.select(Rh, ys, xs, case.quota)
        assert list(zip(xs[keep].tolist(), ys[keep].tolist())) == case.harris


def test_dots_have_their_closed_forms():
    got, R, (Rall, ys, xs) = run(CASES["spread"])
    by_xy = dict(zip(zip(xs.tolist(), ys.tolist()), Rall.tolist()))
    assert by_xy == {(x, y): C.dot_R(c) for x, y, c in D.SPREAD}
    assert R == [C.dot_R(60), C.dot_R(30), C.dot_R(30), C.dot_R(30)]
    scores = ref.fast_scores(D.dots(D.SEAM_RIGHT), 7)
    assert int(scores[20, 40]) == C.dot_score(30) == 29 and int(scores[20, 48]) == C.dot_score(12) == 11


def test_spread_is_one_dot_per_quadrant():
    got, _, _ = run(CASES["spread"])
    assert sorted(next(i for i, (x0, y0, x1, y1) in enumerate(D.QUADRANTS0) if x0 <= x < x1 and y0 <= y < y1) for x, y in got) == [0, 1, 2, 3]
    in_q0 = [p for p in CASES["spread"].harris if p[0] < 35 and p[1] < 33]
    assert len(in_q0) == 3                                               # the rule by R alone: the cluster's three and one other


def test_only_the_first_quadrant_in_the_order_is_split():
    trace = []
    run(CASES["cut5"], trace)
    assert trace == [[D.ROOT0], [D.QUADRANTS0[0]]]                       # four nodes of two dots each: (y0, x0) decides
    trace = []
    run(CASES["cut6"], trace)
    assert trace == [[D.ROOT0], [D.QUADRANTS0[0], D.QUADRANTS0[1]]]      # y0 before x0: the upper right one, not the lower left


def test_rounds_that_gain_nothing():
    trace = []
    got, _, _ = run(CASES["zero_gain"], trace)
    assert got == [(16, 16), (18, 16)]
    assert [r[0][2] - r[0][0] for r in trace] == [133, 67, 34, 17, 9, 5, 3] and all(len(r) == 1 for r in trace)
    assert len(trace) - 1 >= 6                                           # six rounds leave one node, the seventh parts the dots


def test_roots():
    assert dref.roots(97, 150) == [(16, 16, 75, 81), (75, 16, 134, 81)] and dref.n_roots(97, 150) == 2
    assert dref.n_roots(145, 65) == 1 and dref.roots(145, 65) == [(16, 16, 49, 129)]
    assert dref.n_roots(65, 145) == 3 and [r[0] for r in dref.roots(65, 145)] == [16, 53, 91]
    for name in ("two_roots_1", "two_roots_2"):
        trace = []
        run(CASES[name], trace)
        assert trace == []                                               # as many non-empty roots as the quota: no split
    trace = []
    run(CASES["tall"], trace)
    assert trace == [[(16, 16, 49, 129)]]
    assert dref.distribute(np.asarray([20]), np.asarray([20]), 80, 32, 5) == {}


def test_adaptive_cells():
    for name, weak in (("same_cell", (40, 30)), ("seam_left", (47, 20)), ("seam_right", (48, 20))):
        case = CASES[name]
        _, _, (R, ys, xs) = run(case)
        assert weak in list(zip(xs.tolist(), ys.tolist()))               # a candidate at t_min in every case
        live = dref.live_mask(ref.fast_scores(case.img, case.t_min), ys, xs, case.t_ini)
        assert int(live.sum()) == len(case.want)
    _, _, (R, ys, xs) = run(CASES["weak_never"])
    assert list(zip(xs.tolist(), ys.tolist())) == [(40, 20)]


# ------------------------------------------------------------------------------------------------------------- invariants
def _level0(img, quota, t_ini, t_min):
    scores = ref.fast_scores(img, t_min)
    R, ys, xs = ref.candidates(img, t_min)
    live = int(dref.live_mask(scores, ys, xs, t_ini).sum()) if len(R) else 0
    keep = dref.select(R, ys, xs, scores, img.shape[0], img.shape[1], quota, t_ini)
    return xs[keep], ys[keep], live


def _harris0(img, quota, t_ini):
    R, ys, xs = ref.candidates(img, t_ini)
    keep = ref.select(R, ys, xs, quota)
    return xs[keep], ys[keep], len(R)


def _desk():
    return np.load(os.path.join(HERE, "golden", "orb_desk_320x240.npz"))["image"]


IMAGES = {"desk": _desk, "scene": lambda: ref.scene(120, 160, 8, shapes=70), "noise": lambda: ref.noise(96, 112, 9), "half_noise": D.half_noise}


@pytest.mark.parametrize("name", list(IMAGES))
def test_counts_and_occupied_cells(name):
    img = IMAGES[name]()
    n_all = len(ref.candidates(img, 7)[0])
    for quota in (1, 2, 5, 50, 200, n_all + 10):
        hx, hy, n_ini = _harris0(img, quota, 20)
        assert len(hx) == min(quota, n_ini)
        for t_min in (20, 7):
            x, y, live = _level0(img, quota, 20, t_min)
            assert len(x) == min(quota, live) and len(set(zip(x.tolist(), y.tolist()))) == len(x)
            assert live >= n_ini if t_min == 7 else live == n_ini
            assert dref.occupied_cells(x, y) >= dref.occupied_cells(hx, hy), (name, quota, t_min)


def test_the_quadtree_occupies_more_cells_where_it_matters():
    desk = _desk()
    hx, hy, _ = _harris0(desk, 50, 20)
    x, y, _ = _level0(desk, 50, 20, 20)
    x7, y7, _ = _level0(desk, 50, 20, 7)
    print("desk, quota 50: cells", dref.occupied_cells(hx, hy), dref.occupied_cells(x, y), dref.occupied_cells(x7, y7))
    assert dref.occupied_cells(x, y) > dref.occupied_cells(hx, hy)
    half = D.half_noise()
    hx, hy, _ = _harris0(half, 200, 20)
    x7, y7, _ = _level0(half, 200, 20, 7)
    print("half noise, quota 200: cells", dref.occupied_cells(hx, hy), dref.occupied_cells(x7, y7))
    assert dref.occupied_cells(x7, y7) > dref.occupied_cells(hx, hy)


def test_equal_thresholds_and_a_large_quota_give_the_harris_rows():
    img = ref.scene(83, 97, 11, shapes=80)
    lh, lw = ref.level_sizes(83, 97, 4)
    table = ref.steered_table(np.zeros((256, 4), np.int8) + np.asarray([3, 0, -3, 0], np.int8))
    quota = np.asarray([500] * 4, np.int32)
    a = ref.extract(img, lh, lw, quota, 20, table)
    b = dref.extract(img, lh, lw, quota, 20, 20, table)
    for k in ("x", "y", "level", "bin", "response", "descriptors"):
        assert np.array_equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------- the product, no device
def test_params_validation(built):
    from slamhip import orb

    P = orb.OrbParams(240, 320, distribution="quadtree")
    assert P.distribution == "quadtree" and P.t == P.t_min == 20
    assert orb.OrbParams(240, 320).distribution == "harris" and orb.OrbParams(240, 320).t_min == 20
    assert orb.OrbParams(240, 320, distribution="quadtree", fast_threshold_min=7).t_min == 7
    for kw in (dict(distribution="octree"), dict(distribution=None), dict(distribution="quadtree", fast_threshold_min=0),
               dict(distribution="quadtree", fast_threshold_min=21), dict(distribution="quadtree", fast_threshold_min=7.0),
               dict(distribution="quadtree", fast_threshold_min=True), dict(fast_threshold_min=7)):
        with pytest.raises(ValueError):
            orb.OrbParams(240, 320, **kw)
    for bad in (0, 21, 7.0):
        with pytest.raises(ValueError):
            orb.OrbFeatureDetector.quadtree(500, fast_threshold_min=bad)
    det = orb.OrbFeatureDetector.quadtree(300, fast_threshold_min=7)
    assert isinstance(det, orb.OrbFeatureDetector) and (det.n_features, det.distribution, det.fast_threshold_min) == (300, "quadtree", 7)
    plain = orb.OrbFeatureDetector()
    assert (plain.n_features, plain.distribution, plain.fast_threshold_min) == (500, "harris", None)


def test_workspace_query_needs_no_device(built):
    from slamhip import orb

    H, W = 65, 145
    Ph = orb.OrbParams(H, W, n_features=100, n_levels=3)
    Pq = orb.OrbParams(H, W, n_features=100, n_levels=3, distribution="quadtree")
    nh, lh = Ph.workspace(2)
    nq, lq = Pq.workspace(2)
    assert nq > nh
    for k in ("image_base", "counts", "selection"):
        assert lq[k] == lh[k]
    for k in ("image", "blur", "score", "candidates", "pitch", "capacity"):
        assert np.array_equal(lq[k], lh[k]), k                           # today's offsets inside an image block
    assert lq["image_stride"] > lh["image_stride"] and lq["image_stride"] % 256 == 0
    live = np.minimum(Pq.lh, Pq.lw) >= 33
    assert live.tolist() == [True, True, True]
    roots = [dref.n_roots(int(h), int(w)) for h, w in zip(Pq.lh, Pq.lw)]
    assert lq["node_capacity"].tolist() == [r + int(q) + 2 for r, q in zip(roots, Pq.quota)]
    end = int(lh["candidates"][-1]) + 16 * int(lh["capacity"][-1])       # the new buffers lie behind today's, in order, disjoint
    for l in range(3):
        assert lq["node_index"][l] >= end and lq["node_index"][l] % 16 == 0
        assert lq["nodes"][l] >= lq["node_index"][l] + 4 * lq["capacity"][l] and lq["nodes"][l] % 16 == 0
        assert lq["node_best"][l] == lq["nodes"][l] + 64 * lq["node_capacity"][l]
        end = int(lq["node_best"][l] + 16 * lq["node_capacity"][l])
    assert end <= lq["image_stride"] and nq == lq["image_base"] + 2 * lq["image_stride"]
    dead = orb.OrbParams(36, 36, n_features=10, n_levels=3, distribution="quadtree").workspace(1)[1]
    assert dead["node_capacity"].tolist()[1:] == [0, 0] and dead["node_capacity"][0] > 0


def test_workspace_query_argument_errors(built):
    import slamhip
    from slamhip._lib import SLAM_ERR_INVALID, addr

    lib = slamhip.load()
    lw, lh, quota = np.asarray([145, 121], np.int32), np.asarray([65, 54], np.int32), np.asarray([10, 5], np.int32)
    n = ctypes.c_uint64(0)
    assert lib.slam_orb_dist_workspace(1, 65, 145, 2, addr(lw), addr(lh), addr(quota), ctypes.byref(n), None) == 0 and n.value > 0
    assert lib.slam_orb_dist_workspace(0, 65, 145, 2, addr(lw), addr(lh), addr(quota), ctypes.byref(n), None) == 0
    bad = np.asarray([10, -1], np.int32)
    for args in ((1, 65, 145, 2, addr(lw), addr(lh), None), (1, 65, 145, 2, addr(lw), addr(lh), addr(bad)), (1, 65, 145, 17, addr(lw), addr(lh), addr(quota)),
                 (1, 65, 144, 2, addr(lw), addr(lh), addr(quota)), (-1, 65, 145, 2, addr(lw), addr(lh), addr(quota)), (1, 65, 145, 2, None, addr(lh), addr(quota))):
        assert lib.slam_orb_dist_workspace(*args, ctypes.byref(n), None) == SLAM_ERR_INVALID
    assert lib.slam_orb_dist_workspace(1, 65, 145, 2, addr(lw), addr(lh), addr(quota), None, None) == SLAM_ERR_INVALID


def test_header_entries_against_the_signature_table(built):
    import slamhip
    from slamhip import _lib

    header = open(os.path.join(os.path.dirname(HERE), "include", "slamhip.h")).read()
    lib = slamhip.load()
    for name in ("slam_orb_dist_workspace", "slam_orb_extract_dist_u8"):
        m = re.search(r"SLAM_API int " + name + r"\(([^;]*)\);", header)
        assert m, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == m.group(1).count(",") + 1 and getattr(lib, name).argtypes == argtypes
        comment = header[:m.start()].rsplit("/*", 1)[1]
        assert "feature_detectors.py:18-26" in comment and "frontend.py:245" in comment
    assert not re.search(r"slam_orb_extract_dist_u8_host", header) and "slam_orb_extract_dist_u8_host" not in _lib.SIGNATURES
    args = re.search(r"SLAM_API int slam_orb_extract_dist_u8\(([^;]*)\);", header).group(1)
    assert re.search(r"int fast_threshold,\s*int fast_threshold_min", args)
