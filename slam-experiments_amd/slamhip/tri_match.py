"""The epipolar node search and new-map-point creation (``slam_tri_match_*``): ORB-SLAM's
``ORBmatcher::SearchForTriangulation`` - the features of two keyframes that have no map point yet, matched inside one
vocabulary node under the epipolar constraint of the two known poses - and the per-match half of
``LocalMapping::CreateNewMapPoints``: parallax, triangulation, depths, reprojection errors and scale consistency, with the new
point's viewing normal and scale-invariance range.  The result is laid out as ``PointSets`` takes it, so that "keyframe in ->
neighbours -> new points -> ``search_by_projection`` -> BA" is one chain of device calls.

The reference makes its points from a whole-image match and a bare triangulation.  PARITY UNPINNED: the gates are f64 in a
stated operation order, the distance to the epipolar line is tested without its division, the DLT's null vector comes from
Jacobi sweeps instead of an SVD, and the one-to-one step and the rotation check are those of §4k.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Tuple

import numpy as np

from ._args import N_BINS, PAIRS_MAX, _Buffers, _bins_arg, _down, _down_split, _int_rows, _pairs_arg, _poses_arg, _split
from ._lib import TriParams, TriViews, addr, check, load
from .bow_match import FeatureVectors, _groups, _scan_order
from .device import Context, default_context
from .matching import as_descriptors
from .proj_match import camera_centres, scale_tables

ROWS_MAX, LEVELS_MAX = 8192, 16
TH_LOW, CHI2, EPIPOLE_R2 = 50, 3.84, 100.0          # ORBmatcher::TH_LOW, CheckDistEpipolarLine's 3.84, the 100 of 100 * scaleFactor
COS_MAX, CHI2_PX, RATIO = 0.9998, 5.991, 1.5        # CreateNewMapPoints: cosParallaxRays, the reprojection chi2, ratioFactor's 1.5


def limits() -> dict:
    """The library's limits (``slam_tri_match_limits``); needs no GPU."""
    lim = (ctypes.c_int32 * 8)()
    check(load().slam_tri_match_limits(lim))
    assert (lim[0], lim[1], lim[3], lim[4]) == (ROWS_MAX, PAIRS_MAX, LEVELS_MAX, N_BINS), "the library's limits are not this module's"
    return {"rows_per_image": lim[0], "pairs_per_call": lim[1], "scan_lanes": lim[2], "levels": lim[3], "bins": lim[4],
            "search_pair_bytes": lim[5], "triangulate_pair_bytes": lim[6], "params_bytes": lim[7]}


def plan_describe(P: int, n: int) -> dict:
    """The launch plan for ``P`` pairs of ``n`` rows per image, WITHOUT a device (``slam_tri_match_plan_describe``)."""
    plan = (ctypes.c_int64 * 6)()
    check(load().slam_tri_match_plan_describe(int(P), int(n), plan))
    names = ("scan_blocks", "finish_blocks", "triangulate_blocks", "search_workspace_bytes", "triangulate_workspace_bytes",
             "finish_lds_bytes")
    return dict(zip(names, plan))


def _camera(camera) -> Tuple[float, float, float, float]:
    cam = tuple(float(c) for c in camera)
    if len(cam) != 4:
        raise ValueError("camera is (fx, fy, cx, cy)")
    return cam


def _pose(T) -> np.ndarray:
    T = np.asarray(T, np.float64)
    if T.shape not in ((3, 4), (4, 4)):
        raise ValueError(f"a pose is [3,4] or [4,4], got {T.shape}")
    return T[:3]


def fundamental_from_poses(T1, T2, camera) -> np.ndarray:
    """``LocalMapping::ComputeF12``: F12 f64 [3,3] with ``x1^T F12 x2 = 0`` for the pixels x1, x2 (homogeneous) of one point
    in keyframes 1 and 2, from their world -> camera poses: ``R12 = R1 R2^T``, ``t12 = t1 - R12 t2``,
    ``F12 = K^-T [t12]x R12 K^-1``.  numpy on the host."""
    T1, T2 = _pose(T1), _pose(T2)
    fx, fy, cx, cy = _camera(camera)
    R12 = T1[:, :3] @ T2[:, :3].T
    t12 = T1[:, 3] - R12 @ T2[:, 3]
    tx = np.array([[0.0, -t12[2], t12[1]], [t12[2], 0.0, -t12[0]], [-t12[1], t12[0], 0.0]])
    Ki = np.array([[1.0 / fx, 0.0, -cx / fx], [0.0, 1.0 / fy, -cy / fy], [0.0, 0.0, 1.0]])
    return np.ascontiguousarray(Ki.T @ tx @ R12 @ Ki)


def epipole_in_second(T1, T2, camera) -> np.ndarray:
    """The pixel f64 [2] of camera 1's centre in image 2 (``CreateNewMapPoints``' ex, ey); NaN when the centre is not in
    front of camera 2 - a NaN switches the search's epipole gate off."""
    T1, T2 = _pose(T1), _pose(T2)
    fx, fy, cx, cy = _camera(camera)
    c = T2[:, :3] @ camera_centres(T1[None])[0] + T2[:, 3]
    if not c[2] > 0:
        return np.full(2, np.nan)
    return np.array([fx * c[0] / c[2] + cx, fy * c[1] / c[2] + cy])


class KeyframeViews:
    """What the rows of a set of keyframes carry besides their descriptors, resident on the device in ROW order over the whole
    set (the offsets are the ``FeatureVectors``'): ``xy`` f32 [n,2] level-0 pixels, ``level`` int [n] in [0, 16), and
    ``taken`` [n] or None - non-zero = the row has a map point already (``set_taken`` replaces it as points are created;
    the grouped ``FeatureVectors`` stay as they are)."""

    def __init__(self, xy, level, taken=None, ctx: Optional[Context] = None):
        xy = np.asarray(xy, np.float32)
        if xy.ndim != 2 or xy.shape[1] != 2:
            if xy.size:
                raise ValueError(f"xy must have shape [n, 2], got {xy.shape}")
            xy = np.zeros((0, 2), np.float32)
        self.n = len(xy)
        lv = np.ascontiguousarray(_int_rows(level, self.n, "level", 0, LEVELS_MAX), np.int32)
        self.ctx = ctx or default_context()
        pad = lambda a: a if a.size else np.zeros(16, a.dtype)  # noqa: E731
        self.device: Optional[dict] = {"xy": None, "level": None, "taken": None}
        try:
            self.device["xy"] = self.ctx.upload(pad(np.ascontiguousarray(xy)))
            self.device["level"] = self.ctx.upload(pad(lv))
            self.set_taken(taken)
        except BaseException:
            self.free()
            raise

    def set_taken(self, taken) -> None:
        if self.device is None:
            raise ValueError("these views have been freed")
        tk = None if taken is None else np.ascontiguousarray(_int_rows(taken, self.n, "taken", 0, 256) != 0, np.uint8)
        if self.device["taken"] is not None:
            self.device["taken"].free()
            self.device["taken"] = None
        if tk is not None:
            self.device["taken"] = self.ctx.upload(tk if tk.size else np.zeros(16, np.uint8))

    def free(self) -> None:
        if self.device is not None:
            for b in self.device.values():
                if b is not None:
                    b.free()
            self.device = None

    def _struct(self, ctx: Context, n: int) -> TriViews:
        if self.device is None:
            raise ValueError("these views have been freed")
        if self.ctx is not ctx:
            raise ValueError("the views belong to another context")
        if self.n != n:
            raise ValueError(f"the views hold {self.n} rows, the feature vectors {n}")
        d = self.device
        return TriViews(d["xy"].ptr, d["level"].ptr, d["taken"].ptr if d["taken"] is not None else None)


def _tables(scale):
    s, s2 = (np.ascontiguousarray(t, np.float64).reshape(-1) for t in (scale or scale_tables()))
    if not 1 <= len(s) <= LEVELS_MAX or len(s2) != len(s):
        raise ValueError(f"scale is the pair of tables of scale_tables, 1 to {LEVELS_MAX} levels each")
    return s, s2


def _params(camera, scale, th_low=TH_LOW, chi2=CHI2, epipole_r2=EPIPOLE_R2, cos_max=COS_MAX, chi2_px=CHI2_PX, ratio_factor=None):
    s, s2 = _tables(scale)
    if isinstance(th_low, bool) or int(th_low) != th_low or not 0 <= th_low <= 256:
        raise ValueError("th_low must be an integer in [0, 256]")
    rf = RATIO * (s[1] if len(s) > 1 else 1.0) if ratio_factor is None else float(ratio_factor)
    vals = [float(chi2), float(epipole_r2), float(cos_max), float(chi2_px), float(rf)]
    if any(v != v for v in vals):
        raise ValueError("chi2, epipole_r2, cos_max, chi2_px and ratio_factor must be numbers")
    prm = TriParams(*_camera(camera), *vals, addr(s), addr(s2), len(s), int(th_low))
    return prm, (s, s2)                                  # (the tables must outlive the call)


def _pair_f64(a, P: int, shape: tuple, name: str) -> np.ndarray:
    a = np.asarray(a, np.float64)
    if P == 0:
        return np.zeros((0,) + shape)
    if a.shape == shape:
        a = a[None]
    if a.shape != (P,) + shape:
        raise ValueError(f"{name} must have shape {(P,) + shape}, got {a.shape}")
    return np.ascontiguousarray(a)


def _check_sets(fv1, fv2, views1, views2):
    if not isinstance(fv1, FeatureVectors) or not isinstance(fv2, FeatureVectors):
        raise ValueError("the two sides are FeatureVectors (see bow_feature_vectors, FeatureVectors.from_nodes)")
    if not isinstance(views1, KeyframeViews) or not isinstance(views2, KeyframeViews):
        raise ValueError("views1 and views2 are KeyframeViews")


def _search(ctx, m, fv1, fv2, views1, views2, p, F, epi, prm, b1, b2, scan_order, total, tables: bool):
    g1 = _groups(fv1, fv1._resident(ctx, m), m.up(b1) if b1 is not None else None)
    g2 = _groups(fv2, fv2._resident(ctx, m), m.up(b2) if b2 is not None else None)
    v1, v2 = views1._struct(ctx, fv1.n), views2._struct(ctx, fv2.n)
    d_m, d_c = m.new(4 * total), m.new(4 * len(p))
    d_i, d_d = (m.new(8 * total), m.new(8 * total)) if tables else (None, None)
    check(ctx.lib.slam_tri_match_search(ctx.handle, ctypes.byref(g1), ctypes.byref(g2), ctypes.byref(v1), ctypes.byref(v2), addr(p), len(p),
                                        addr(F), addr(epi), ctypes.byref(prm), scan_order, d_m.ptr, d_c.ptr, d_i.ptr if d_i else None,
                                        d_d.ptr if d_d else None))
    return d_m, d_c, d_i, d_d, (v1, v2)


def _triangulate(ctx, m, fv1, fv2, v1, v2, p, d_m, T1, T2, prm, total):
    O1, O2 = camera_centres(T1), camera_centres(T2)
    out = [m.new(sz * total) for sz in (24, 24, 16, 4)] + [m.new(4 * len(p))]
    check(ctx.lib.slam_tri_match_triangulate(ctx.handle, addr(fv1.offsets), len(fv1), addr(fv2.offsets), len(fv2), ctypes.byref(v1),
                                             ctypes.byref(v2), addr(p), len(p), d_m.ptr, addr(T1), addr(T2), addr(O1), addr(O2),
                                             ctypes.byref(prm), *(b.ptr for b in out)))
    return out


def _sizes(fv1, p):
    sizes = np.diff(fv1.offsets)[p[:, 0]]
    return sizes, int(sizes.sum())


def _bins_pair(bins1, bins2, fv1, fv2):
    b1, b2 = _bins_arg(bins1, fv1.n, "bins1"), _bins_arg(bins2, fv2.n, "bins2")
    if (b1 is None) != (b2 is None):
        raise ValueError("bins1 and bins2 come together or not at all")
    return b1, b2


def search_for_triangulation(fv1: FeatureVectors, fv2: FeatureVectors, pairs, views1: KeyframeViews, views2: KeyframeViews, F, epipoles,
                             scale=None, bins1=None, bins2=None, th_low: int = TH_LOW, chi2: float = CHI2,
                             epipole_r2: float = EPIPOLE_R2, return_tables: bool = False, ctx: Optional[Context] = None,
                             scan_order: int = 0):
    """``ORBmatcher::SearchForTriangulation`` for P keyframe pairs in one copy, one memset and two launches.
    ``pairs`` int [P,2] holds (image of ``fv1``, image of ``fv2``); ``F`` f64 [P,3,3] is ``fundamental_from_poses`` of each pair
    and ``epipoles`` f64 [P,2] ``epipole_in_second`` (NaN: no epipole gate); ``scale``: the tables of ``scale_tables`` (None: 8
    levels at 1.2), whose second table is sigma^2 per level.

    Row j of side 2 is a candidate for row i of side 1 iff both lie in one node (>= 0), neither is ``taken``, their distance
    is at most ``th_low``, j is not within ``sqrt(epipole_r2 * scale[level_j])`` of the epipole and lies within
    ``sqrt(chi2 * sigma2[level_j])`` pixels of the epipolar line of i.  The nearest candidate is proposed - there is no ratio
    test - and the one-to-one step and rotation check of ``search_by_bow`` follow.

    Returns (matches12: list of int32 [n1] holding the side-2 row or -1, counts int32 [P]) and with ``return_tables`` also the
    list of the top-2 tables (idx, dist) int32 [n1, 2] of the candidates."""
    _check_sets(fv1, fv2, views1, views2)
    p = _pairs_arg(pairs, len(fv1), len(fv2))
    P = len(p)
    b1, b2 = _bins_pair(bins1, bins2, fv1, fv2)
    prm, keep = _params((1.0, 1.0, 0.0, 0.0), scale, th_low, chi2, epipole_r2)
    scan_order = _scan_order(scan_order)
    Fm, epi = _pair_f64(F, P, (3, 3), "F"), _pair_f64(epipoles, P, (2,), "epipoles")
    if P == 0:
        return ([], np.zeros(0, np.int32), []) if return_tables else ([], np.zeros(0, np.int32))
    sizes, total = _sizes(fv1, p)
    ctx = ctx or fv1.ctx
    m = _Buffers(ctx)
    try:
        d_m, d_c, d_i, d_d, _ = _search(ctx, m, fv1, fv2, views1, views2, p, Fm, epi, prm, b1, b2, scan_order, total, return_tables)
        counts = d_c.download(np.int32, (P,))
        matches = _down_split(d_m, np.int32, (), total, sizes)
        if not return_tables:
            return matches, counts
        return matches, counts, list(zip(_down_split(d_i, np.int32, (2,), total, sizes), _down_split(d_d, np.int32, (2,), total, sizes)))
    finally:
        m.free()
        del keep


def _points(out, P: int, total: int, sizes) -> List[dict]:
    X, nr, rg, st = (_down(b, dt, sh, total) for b, (dt, sh) in zip(out, ((np.float64, (3,)), (np.float64, (3,)), (np.float64, (2,)),
                                                                         (np.int32, ()))))
    cols = dict(status=_split(st, sizes), X=_split(X, sizes), normal=_split(nr, sizes), dmin2=_split(np.ascontiguousarray(rg[:, 0]), sizes),
                dmax2=_split(np.ascontiguousarray(rg[:, 1]), sizes))
    return [{k: cols[k][i] for k in cols} for i in range(P)]


def triangulate_matches(fv1: FeatureVectors, fv2: FeatureVectors, pairs, views1: KeyframeViews, views2: KeyframeViews, matches12, poses1,
                        poses2, camera, scale=None, cos_max: float = COS_MAX, chi2_px: float = CHI2_PX, ratio_factor=None,
                        ctx: Optional[Context] = None):
    """The per-match half of ``LocalMapping::CreateNewMapPoints`` in one launch for P pairs: ``matches12`` is the list of
    ``search_for_triangulation`` (or any int [n1] arrays of side-2 rows, -1 = none); ``poses1`` / ``poses2`` f64 [P,3,4] (or
    [P,4,4]) the world -> camera poses of the pair's two keyframes; ``camera`` = (fx, fy, cx, cy).  Returns (points: per pair
    a dict ``status`` int32 [n1] (0 created, 1 no match, 2 parallax, 3 at infinity, 4 / 5 behind camera 1 / 2, 6 / 7
    reprojection error in image 1 / 2, 8 scale inconsistent), ``X`` f64 [n1,3], ``normal`` f64 [n1,3], ``dmin2``, ``dmax2``
    f64 [n1] - NaN wherever status != 0, so the arrays go into ``PointSets`` as they are - and created int32 [P])."""
    _check_sets(fv1, fv2, views1, views2)
    p = _pairs_arg(pairs, len(fv1), len(fv2))
    P = len(p)
    T1, T2 = _poses_arg(poses1, P), _poses_arg(poses2, P)
    prm, keep = _params(camera, scale, cos_max=cos_max, chi2_px=chi2_px, ratio_factor=ratio_factor)
    if P == 0:
        return [], np.zeros(0, np.int32)
    sizes, total = _sizes(fv1, p)
    if len(matches12) != P or any(np.asarray(a).shape != (s,) for a, s in zip(matches12, sizes)):
        raise ValueError("matches12 holds one int array [n1] per pair")
    flat = np.concatenate([np.asarray(a, np.int32).reshape(-1) for a in matches12]) if total else np.zeros(0, np.int32)
    ctx = ctx or fv1.ctx
    m = _Buffers(ctx)
    try:
        out = _triangulate(ctx, m, fv1, fv2, views1._struct(ctx, fv1.n), views2._struct(ctx, fv2.n), p, m.up(np.ascontiguousarray(flat)),
                           T1, T2, prm, total)
        return _points(out, P, total, sizes), out[4].download(np.int32, (P,))
    finally:
        m.free()
        del keep


def create_new_map_points(fv1: FeatureVectors, fv2: FeatureVectors, pairs, views1: KeyframeViews, views2: KeyframeViews, poses1, poses2,
                          camera, scale=None, bins1=None, bins2=None, th_low: int = TH_LOW, chi2: float = CHI2,
                          epipole_r2: float = EPIPOLE_R2, cos_max: float = COS_MAX, chi2_px: float = CHI2_PX, ratio_factor=None,
                          ctx: Optional[Context] = None):
    """``LocalMapping::CreateNewMapPoints`` for P keyframe pairs: the fundamental matrices and epipoles from the poses on the
    host, then ``search_for_triangulation`` and ``triangulate_matches`` as one chain of launches - the matches never leave the
    device in between.  Returns (points, matched int32 [P], created int32 [P]): per pair a dict with ``matches12`` int32 [n1]
    and ``status``, ``X``, ``normal``, ``dmin2``, ``dmax2`` as ``triangulate_matches`` returns them."""
    _check_sets(fv1, fv2, views1, views2)
    p = _pairs_arg(pairs, len(fv1), len(fv2))
    P = len(p)
    T1, T2 = _poses_arg(poses1, P), _poses_arg(poses2, P)
    b1, b2 = _bins_pair(bins1, bins2, fv1, fv2)
    prm, keep = _params(camera, scale, th_low, chi2, epipole_r2, cos_max, chi2_px, ratio_factor)
    if P == 0:
        return [], np.zeros(0, np.int32), np.zeros(0, np.int32)
    F = np.ascontiguousarray(np.stack([fundamental_from_poses(a, b, camera) for a, b in zip(T1, T2)]))
    epi = np.ascontiguousarray(np.stack([epipole_in_second(a, b, camera) for a, b in zip(T1, T2)]))
    sizes, total = _sizes(fv1, p)
    ctx = ctx or fv1.ctx
    m = _Buffers(ctx)
    try:
        d_m, d_c, _, _, (v1, v2) = _search(ctx, m, fv1, fv2, views1, views2, p, F, epi, prm, b1, b2, 0, total, False)
        out = _triangulate(ctx, m, fv1, fv2, v1, v2, p, d_m, T1, T2, prm, total)
        pts = _points(out, P, total, sizes)
        for d, m12 in zip(pts, _down_split(d_m, np.int32, (), total, sizes)):
            d["matches12"] = m12
        return pts, d_c.download(np.int32, (P,)), out[4].download(np.int32, (P,))
    finally:
        m.free()
        del keep


def epi_match_arrays(query, train, query_nodes, train_nodes, query_xy, train_xy, train_level, F, epipole=(np.nan, np.nan), scale=None,
                     k: int = 2, th_low: int = 256, chi2: float = CHI2, epipole_r2: float = EPIPOLE_R2, query_taken=None, train_taken=None,
                     ctx: Optional[Context] = None, scan_order: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """``knnMatch(query, train, k, mask=W)`` for the epipolar node mask W of one pair - the mirror of ``node_match_arrays``:
    train row j is a candidate for query row i iff ``search_for_triangulation`` would compare them.  Returns (idx, dist)
    int32 [N, k], k in {1, 2}, ordered by (distance, train index); missing neighbours (-1, INT32_MAX)."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or int(k) not in (1, 2):
        raise ValueError(f"k must be 1 or 2, got {k!r}")
    q, t = as_descriptors(query), as_descriptors(train)
    if max(len(q), len(t)) > ROWS_MAX:
        raise ValueError(f"at most {ROWS_MAX} rows per image")
    ctx = ctx or default_context()
    made = []
    try:
        made.append(FeatureVectors.from_nodes(q, query_nodes, ctx=ctx))
        made.append(FeatureVectors.from_nodes(t, train_nodes, ctx=ctx))
        made.append(KeyframeViews(query_xy, np.zeros(len(q), np.int32), query_taken, ctx))
        made.append(KeyframeViews(train_xy, train_level, train_taken, ctx))
        _, _, tab = search_for_triangulation(made[0], made[1], [(0, 0)], made[2], made[3], np.asarray(F, np.float64).reshape(1, 3, 3),
                                             np.asarray(epipole, np.float64).reshape(1, 2), scale, th_low=th_low, chi2=chi2,
                                             epipole_r2=epipole_r2, return_tables=True, ctx=ctx, scan_order=scan_order)
    finally:
        for x in made:
            x.free()
    return np.ascontiguousarray(tab[0][0][:, :int(k)]), np.ascontiguousarray(tab[0][1][:, :int(k)])
