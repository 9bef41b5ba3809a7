"""Map points matched into frames by projection (``slam_proj_match_*``): ORB-SLAM's
``ORBmatcher::SearchByProjection`` - the step that turns a first pose into the several hundred correspondences a refinement
needs (``TrackWithMotionModel``, ``TrackLocalMap``, the second half of ``Relocalization``, ``ComputeSim3``) - and
``SearchBySim3``, batched over (point set, frame, pose) pairs.

The reference tracks by a whole-image brute-force match instead (``frontend.py:156-187``).  PARITY UNPINNED: the gates are
f64 in a stated operation order, the predicted level is a count of comparisons instead of a logarithm, the search radius
does not depend on the viewing angle, and the one-to-one step and the rotation check are those of §4k.  There is no CPU
fallback.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np

from ._args import (N_BINS, PAIRS_MAX, _Buffers, _bins_arg, _device_rows, _down_split, _f64_rows, _int_rows, _offsets, _pairs_arg, _poses_arg,
                    _rows_arg)
from ._lib import ProjFrames, ProjParams, ProjPoints, addr, check, load
from .bow_match import match_index_pairs  # noqa: F401  (part of this module's interface)
from .device import Context, DeviceBuffer, default_context
from .matching import as_descriptors

ROWS_MAX, LEVELS_MAX = 8192, 16
TH_HIGH, RATIO, COS2_LIMIT, CELL = 100, 0.9, 0.25, 16     # ORBmatcher::TH_HIGH, mfNNratio of the tracking calls, cos^2 60 deg


def limits() -> dict:
    """The library's limits (``slam_proj_match_limits``); needs no GPU."""
    lim = (ctypes.c_int32 * 6)()
    check(load().slam_proj_match_limits(lim))
    assert (lim[0], lim[1], lim[3], lim[4]) == (ROWS_MAX, PAIRS_MAX, LEVELS_MAX, N_BINS), "the library's limits are not this module's"
    return {"rows_per_image": lim[0], "pairs_per_call": lim[1], "scan_lanes": lim[2], "levels": lim[3], "bins": lim[4], "pair_bytes": lim[5]}


def plan_describe(B: int, P: int, n: int) -> dict:
    """The launch plan for ``B`` frames and ``P`` pairs of ``n`` rows each, WITHOUT a device."""
    plan = (ctypes.c_int64 * 8)()
    check(load().slam_proj_match_plan_describe(int(B), int(P), int(n), plan))
    names = ("cell_blocks", "sort_blocks", "gather_blocks", "scan_blocks", "finish_blocks", "workspace_bytes", "finish_lds_bytes",
             "grid_workspace_bytes")
    return dict(zip(names, plan))


def scale_tables(n_levels: int = 8, scale: float = 1.2) -> Tuple[np.ndarray, np.ndarray]:
    """(scale[l], scale2[l]) f64 [n_levels] as ORB-SLAM's extractor makes them: s_0 = 1, s_l = s_{l-1} * scale, and their
    squares.  Made on the host: the device only ever compares with them."""
    if isinstance(n_levels, bool) or int(n_levels) != n_levels or not 1 <= n_levels <= LEVELS_MAX:
        raise ValueError(f"n_levels must be an integer in [1, {LEVELS_MAX}]")
    s = np.ones(int(n_levels), np.float64)
    for l in range(1, int(n_levels)):
        s[l] = s[l - 1] * np.float64(scale)
    return s, s * s


def _set_offsets(offsets, n: int, what: str) -> np.ndarray:
    off = _offsets([0, n] if offsets is None else offsets, n)
    if len(off) > 1 and np.diff(off).max() > ROWS_MAX:
        raise ValueError(f"at most {ROWS_MAX} {what}")
    return off


class FrameGrids:
    """B frames with their features grouped into square cells (``Frame::AssignFeaturesToGrid``; the counterpart of
    ``FeatureVectors``): frame b owns the positions ``[offsets[b], offsets[b+1])``; inside a frame the rows are sorted by
    (cell, row), the cell of a row being ``clamp(floor(y / cell)) * columns + clamp(floor(x / cell))`` over ``[0, W) x [0, H)``.
    ``order`` int32 [n] is the row (local to its frame) at each position, ``cells`` int32 [n] the cell of each ROW; both are
    read from the device when asked for.  Built once per frame, reused by every search, resident until ``free``."""

    _NAMES = ("desc", "cells_sorted", "order", "inverse", "xy", "meta", "cells", "level", "bins")

    def __init__(self, ctx: Context, offsets: np.ndarray, size: Tuple[int, int], cell: int, device: dict):
        self.ctx, self.offsets, self.size, self.cell = ctx, offsets, (int(size[0]), int(size[1])), int(cell)
        self.device: Optional[dict] = device

    def __len__(self) -> int:
        return len(self.offsets) - 1

    @property
    def n(self) -> int:
        return int(self.offsets[-1])

    @property
    def grid(self) -> Tuple[int, int]:
        """(columns, rows) of the cell grid."""
        return -(-self.size[0] // self.cell), -(-self.size[1] // self.cell)

    def _read(self, name: str, dtype, shape) -> np.ndarray:
        if self.device is None:
            raise ValueError("these frame grids have been freed")
        return self.device[name].download(dtype, shape) if self.n else np.zeros(shape, dtype)

    @property
    def order(self) -> np.ndarray:
        return self._read("order", np.int32, (self.n,))

    @property
    def cells(self) -> np.ndarray:
        return self._read("cells", np.int32, (self.n,))

    @property
    def cells_sorted(self) -> np.ndarray:
        return self._read("cells_sorted", np.int32, (self.n,))

    @property
    def descriptors_sorted(self) -> np.ndarray:
        return self._read("desc", np.uint8, (self.n, 32))

    @property
    def xy_sorted(self) -> np.ndarray:
        return self._read("xy", np.float32, (self.n, 2))

    def free(self) -> None:
        if self.device is not None:
            for b in self.device.values():
                if b is not None:
                    b.free()
            self.device = None

    def _struct(self, ctx: Context) -> ProjFrames:
        if self.device is None:
            raise ValueError("these frame grids have been freed")
        if self.ctx is not ctx:
            raise ValueError("the frame grids belong to another context")
        d = self.device
        return ProjFrames(d["desc"].ptr, d["cells_sorted"].ptr, d["order"].ptr, d["xy"].ptr, d["meta"].ptr, d["level"].ptr,
                          d["bins"].ptr if d["bins"] is not None else None, addr(self.offsets), len(self), self.size[0], self.size[1],
                          self.cell, 0)

    @classmethod
    def from_arrays(cls, descriptors, xy, level, size: Tuple[int, int], offsets=None, bins=None, taken=None, cell: int = CELL,
                    ctx: Optional[Context] = None) -> "FrameGrids":
        """``descriptors``: u8 [n,32] or ``(DeviceBuffer, n)``; ``xy`` f32 [n,2] level-0 pixels; ``level`` int [n] in [0, 16);
        ``size`` = (W, H); ``offsets`` int [B+1] (None: one frame); ``bins`` int [n] in [0, 32) or None; ``taken`` [n], non-zero
        = out of every search, or None; ``cell``: the side of a cell in pixels (results do not depend on it)."""
        rows, n = _rows_arg(descriptors)
        off = _set_offsets(offsets, n, "rows per frame")
        W, H = int(size[0]), int(size[1])
        if W <= 0 or H <= 0:
            raise ValueError(f"size must be positive, got {size}")
        if isinstance(cell, bool) or int(cell) != cell or cell <= 0:
            raise ValueError(f"cell must be a positive integer, got {cell!r}")
        if -(-W // int(cell)) * -(-H // int(cell)) > 1 << 30:
            raise ValueError("more than 2^30 cells")
        xy = np.asarray(xy, np.float32)
        xy = np.ascontiguousarray(xy.reshape(n, 2)) if xy.size == 2 * n else xy
        if xy.shape != (n, 2):
            raise ValueError(f"xy must have shape [{n}, 2], got {xy.shape}")
        lv = np.ascontiguousarray(_int_rows(level, n, "level", 0, LEVELS_MAX), np.int32)
        bn = _bins_arg(bins, n, "bins")
        tk = None if taken is None else np.ascontiguousarray(_int_rows(taken, n, "taken", 0, 256) != 0, np.uint8)
        ctx = ctx or default_context()
        m = _Buffers(ctx)
        dev = dict.fromkeys(cls._NAMES)
        try:
            for name, sz in (("desc", 32), ("cells_sorted", 4), ("order", 4), ("inverse", 4), ("xy", 8), ("meta", 4), ("cells", 4)):
                dev[name] = ctx.malloc(max(sz * n, 16))
            dev["level"] = ctx.upload(lv if n else np.zeros(4, np.int32))
            dev["bins"] = ctx.upload(bn if n else np.zeros(16, np.uint8)) if bn is not None else None
            if n:
                d_rows, d_xy = _device_rows(ctx, m, rows), m.up(xy)
                d_taken = m.up(tk) if tk is not None else None
                check(ctx.lib.slam_proj_match_grid(ctx.handle, d_rows.ptr, d_xy.ptr, dev["level"].ptr, d_taken.ptr if d_taken else None, addr(off),
                                                   len(off) - 1, W, H, int(cell), dev["cells"].ptr, dev["desc"].ptr, dev["cells_sorted"].ptr,
                                                   dev["order"].ptr, dev["inverse"].ptr, dev["xy"].ptr, dev["meta"].ptr))
                ctx.sync()                               # the inputs may be the caller's temporaries
        except BaseException:
            for b in dev.values():
                if b is not None:
                    b.free()
            raise
        finally:
            m.free()
        return cls(ctx, off, (W, H), int(cell), dev)

    @classmethod
    def from_orb(cls, result, taken=None, cell: int = CELL, ctx: Optional[Context] = None, xy=None) -> "FrameGrids":
        """The frames of an ``OrbResult``: pixels, levels and bins as it holds them.  A result kept on the device
        (``keep_on_device=True``) whose rows are contiguous - one image, or every image full - is grouped from its resident
        descriptor block; otherwise the descriptors are uploaded.  ``xy`` (one array [n,2] or a list of one per image)
        overrides the pixels the grid is built from: the undistorted keypoints (``OrbResult.undistorted``), kept as float32
        like ORB-SLAM's ``mvKeysUn``.  Pixels outside the image fall into the border cells; a row whose override is not
        finite (a keypoint without an undistorted image) is taken out of every search."""
        counts = np.asarray(result.counts, np.int64)
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        n = int(off[-1])
        cat = lambda parts, shape, dt: np.concatenate([np.asarray(p, dt).reshape(shape) for p in parts]) if len(parts) else np.zeros(shape, dt)  # noqa: E731
        desc = cat(result.descriptors, (-1, 32), np.uint8)
        if getattr(result, "_block", None) is not None and n and (len(counts) == 1 or (counts == result.params.n_max).all()):
            desc = (result._block.view(0, n * 32), n)
        if xy is None:
            pix = cat(result.xy, (-1, 2), np.float32)
        else:
            pix = cat(xy, (-1, 2), np.float32) if isinstance(xy, (list, tuple)) else np.asarray(xy, np.float32).reshape(-1, 2)
            if pix.shape != (n, 2):
                raise ValueError(f"xy must hold {n} pixels, got shape {pix.shape}")
            lost = ~np.isfinite(pix).all(axis=1)
            if lost.any():
                pix = np.where(lost[:, None], np.float32(0), pix)
                tk = np.zeros(n, np.uint8) if taken is None else (_int_rows(taken, n, "taken", 0, 256) != 0).astype(np.uint8)
                taken = tk | lost.astype(np.uint8)
        return cls.from_arrays(desc, pix, cat(result.level, (-1,), np.int64), (result.params.W, result.params.H),
                               off, cat(result.bin, (-1,), np.int64), taken, cell, ctx)


class PointSets:
    """Sets of map points resident on the device: set a owns the points ``[offsets[a], offsets[a+1])`` (at most 8192 each).
    ``xyz`` f64 [n,3] world positions, ``descriptors`` u8 [n,32] (``MapPoint::GetDescriptor``); optional: ``dmin2`` and
    ``dmax2`` f64 [n], the SQUARES of the scale-invariance distances, ``normal`` f64 [n,3] unit viewing normals, ``level``
    int [n] the pyramid level each point was last seen at, ``bins`` int [n] orientation bins in [0, 32)."""

    def __init__(self, xyz, descriptors, offsets=None, dmin2=None, dmax2=None, normal=None, level=None, bins=None,
                 ctx: Optional[Context] = None):
        rows, n = _rows_arg(descriptors)
        self.offsets = _set_offsets(offsets, n, "points per set")
        x = _f64_rows(xyz, n, 3, "xyz")
        if (dmin2 is None) != (dmax2 is None):
            raise ValueError("dmin2 and dmax2 come together or not at all")
        rng = None if dmin2 is None else np.ascontiguousarray(np.stack([_f64_rows(dmin2, n, 1, "dmin2")[:, 0], _f64_rows(dmax2, n, 1, "dmax2")[:, 0]], 1))
        nr = None if normal is None else _f64_rows(normal, n, 3, "normal")
        lv = None if level is None else np.ascontiguousarray(_int_rows(level, n, "level", 0, LEVELS_MAX), np.int32)
        bn = _bins_arg(bins, n, "bins")
        self.ctx = ctx or default_context()
        self.has_range, self.has_level = rng is not None, lv is not None
        pad = lambda a: a if a.size else np.zeros(16, a.dtype)  # noqa: E731
        self.device: Optional[dict] = {}
        try:
            self.device["desc"] = rows if isinstance(rows, DeviceBuffer) else self.ctx.upload(pad(rows))
            self._own_desc = not isinstance(rows, DeviceBuffer)
            if isinstance(rows, DeviceBuffer) and rows.ctx is not self.ctx:
                raise ValueError("the device rows belong to another context")
            for name, a in (("xyz", x), ("range", rng), ("normal", nr), ("level", lv), ("bins", bn)):
                self.device[name] = self.ctx.upload(pad(a)) if a is not None else None
        except BaseException:
            self.free()
            raise

    def __len__(self) -> int:
        return len(self.offsets) - 1

    @property
    def n(self) -> int:
        return int(self.offsets[-1])

    def free(self) -> None:
        if self.device is not None:
            for name, b in self.device.items():
                if b is not None and (name != "desc" or self._own_desc):
                    b.free()
            self.device = None

    def _struct(self, ctx: Context) -> ProjPoints:
        if self.device is None:
            raise ValueError("these point sets have been freed")
        if self.ctx is not ctx:
            raise ValueError("the point sets belong to another context")
        p = lambda k: self.device[k].ptr if self.device[k] is not None else None  # noqa: E731
        return ProjPoints(p("xyz"), p("desc"), p("range"), p("normal"), p("level"), p("bins"), addr(self.offsets), len(self))


def camera_centres(poses) -> np.ndarray:
    """The camera centres ``-M^-1 t`` of poses ``[M | t]`` f64 [P,3,4] (M = R, or sR for a Sim(3))."""
    A = np.asarray(poses, np.float64).reshape(-1, 3, 4)
    return np.ascontiguousarray(np.stack([-np.linalg.solve(a[:, :3], a[:, 3]) for a in A])) if len(A) else np.zeros((0, 3))


def _params(camera, bounds, scale, th_high, ratio, cos2_limit, level_rule: bool, lo: int, hi: int):
    cam = [float(c) for c in camera]
    bnd = [float(b) for b in bounds]
    if len(cam) != 4 or len(bnd) != 4:
        raise ValueError("camera is (fx, fy, cx, cy) and bounds (min_x, max_x, min_y, max_y)")
    s, s2 = (np.ascontiguousarray(t, np.float64).reshape(-1) for t in scale)
    if not 1 <= len(s) <= LEVELS_MAX or len(s2) != len(s):
        raise ValueError(f"scale is the pair of tables of scale_tables, 1 to {LEVELS_MAX} levels each")
    if isinstance(th_high, bool) or int(th_high) != th_high or not -(1 << 31) <= th_high < 1 << 31:
        raise ValueError("th_high must be an integer")
    ratio = float(ratio)
    if ratio != ratio:
        raise ValueError("ratio is not a number")
    if lo > hi:
        raise ValueError(f"the level offsets ({lo}, {hi}) descend")
    prm = ProjParams(*cam, *bnd, float(cos2_limit), ratio, addr(s), addr(s2), len(s), int(th_high), int(bool(level_rule)), int(lo), int(hi), 0)
    return prm, (s, s2)                                  # (the tables must outlive the call)


def _th_arg(th, P: int) -> np.ndarray:
    t = np.ascontiguousarray(np.broadcast_to(np.asarray(th, np.float64), (P,)))
    if P and not (t > 0).all():
        raise ValueError("th must be positive")
    return t


def _pair_args(P: int, poses, centres, th):
    A = _poses_arg(poses, P)
    Ow = camera_centres(A) if centres is None else _f64_rows(centres, P, 3, "centres")
    return A, Ow, _th_arg(th, P)


def _default_bounds(frames: FrameGrids):
    return (0.0, float(frames.size[0]), 0.0, float(frames.size[1]))


def _level_rule(points: PointSets, level_rule, level_offsets):
    rule = (points.has_range or points.has_level) if level_rule is None else bool(level_rule)
    lo, hi = ((-1, 0) if points.has_range else (-1, 1)) if level_offsets is None else (int(level_offsets[0]), int(level_offsets[1]))
    return rule, lo, hi


def search_by_projection(points: PointSets, frames: FrameGrids, pairs, poses, centres=None, camera=(1.0, 1.0, 0.0, 0.0), bounds=None,
                         scale=None, th=1.0, th_high: int = TH_HIGH, ratio: float = RATIO, cos2_limit: float = COS2_LIMIT,
                         level_offsets=None, level_rule=None, return_tables: bool = False, ctx: Optional[Context] = None):
    """``ORBmatcher::SearchByProjection`` for P pairs in a pair-table copy, one memset and two launches.
    ``pairs`` int [P,2] holds (set of ``points``, frame of ``frames``); ``poses`` f64 [P,3,4] (or [P,4,4]) world -> camera of
    the pair's frame, a rigid pose or ``[sR | t]``; ``centres`` f64 [P,3] the camera centres (None: ``-M^-1 t``); ``camera`` =
    (fx, fy, cx, cy); ``bounds`` = (min_x, max_x, min_y, max_y) (None: the frames' image); ``scale``: the tables of
    ``scale_tables`` (None: 8 levels at 1.2); ``th``: the radius factor, one number or one per pair.

    Per point: the gates (in front, inside the bounds, inside its distance range when the points carry ranges, within 60
    degrees of its normal when they carry normals), the predicted level (from the range; else the level it was last seen at;
    else 0) and the radius ``th * scale[level]``; the two nearest frame rows strictly inside the window that are not taken
    and - ``level_rule``, on by default when the points carry ranges or levels - lie ``level_offsets`` around the predicted
    level (default (-1, 0) with ranges, (-1, +1) with levels); ORB-SLAM's selection (``d0 <= th_high``; the ratio only
    between two neighbours on one level - NOT the rule of ``search_by_bow``); the one-to-one step and, when both sides
    carry bins, the rotation check of ``search_by_bow``.

    Returns (matches12: list of int32 [P_a] holding the frame row or -1, counts int32 [P]) and with ``return_tables`` a list
    of dicts ``status, u, v, lp, idx, dist`` per pair."""
    if not isinstance(points, PointSets) or not isinstance(frames, FrameGrids):
        raise ValueError("search_by_projection takes PointSets and FrameGrids")
    p = _pairs_arg(pairs, len(points), len(frames))
    P = len(p)
    A, Ow, t = _pair_args(P, poses, centres, th)
    rule, lo, hi = _level_rule(points, level_rule, level_offsets)
    prm, keep = _params(camera, _default_bounds(frames) if bounds is None else bounds, scale or scale_tables(), th_high, ratio, cos2_limit,
                        rule, lo, hi)
    if P == 0:
        return ([], np.zeros(0, np.int32), []) if return_tables else ([], np.zeros(0, np.int32))
    sizes = np.diff(points.offsets)[p[:, 0]]
    total = int(sizes.sum())
    ctx = ctx or points.ctx
    sp, sf = points._struct(ctx), frames._struct(ctx)
    m = _Buffers(ctx)
    try:
        d_m, d_c = m.new(4 * total), m.new(4 * P)
        tabs = [m.new(sz * total) for sz in (4, 8, 8, 4, 8, 8)] if return_tables else [None] * 6
        check(ctx.lib.slam_proj_match_search(ctx.handle, ctypes.byref(sp), ctypes.byref(sf), addr(p), addr(A), addr(Ow), addr(t), P,
                                             ctypes.byref(prm), d_m.ptr, d_c.ptr, *(b.ptr if b else None for b in tabs)))
        counts = d_c.download(np.int32, (P,))
        matches = _down_split(d_m, np.int32, (), total, sizes)
        if not return_tables:
            return matches, counts
        return matches, counts, _tables(tabs, total, sizes, True)
    finally:
        m.free()
        del keep


def _tables(tabs, total: int, sizes, search: bool) -> List[dict]:
    spec = (("status", np.int32, ()), ("u", np.float64, ()), ("v", np.float64, ()), ("lp", np.int32, ()), ("idx", np.int32, (2,)),
            ("dist", np.int32, (2,)))[:6 if search else 4]
    cols = {name: _down_split(b, dt, sh, total, sizes) for (name, dt, sh), b in zip(spec, tabs)}
    return [{name: cols[name][i] for name in cols} for i in range(len(sizes))]


def project_points(points: PointSets, sets, poses, centres=None, camera=(1.0, 1.0, 0.0, 0.0), bounds=(-np.inf, np.inf, -np.inf, np.inf),
                   scale=None, th=1.0, cos2_limit: float = COS2_LIMIT, ctx: Optional[Context] = None) -> List[dict]:
    """The gates alone (``Frame::isInFrustum``): for pair p the points of set ``sets[p]`` under ``poses[p]`` -> a list of
    dicts ``status`` (0 searched, 1 behind, 2 out of bounds, 3 out of range, 4 off the normal), ``u``, ``v`` (NaN where never
    computed) and ``lp`` (the predicted level, -1 where the point is not searched)."""
    if not isinstance(points, PointSets):
        raise ValueError("project_points takes PointSets")
    s = np.asarray(sets)
    if s.size and (s.dtype.kind not in "iu" or s.ndim != 1 or s.min() < 0 or s.max() >= len(points)):
        raise ValueError("sets must be indices of point sets")
    if len(s) > PAIRS_MAX:
        raise ValueError(f"at most {PAIRS_MAX} pairs per call")
    s = np.ascontiguousarray(s.reshape(-1), np.int32)
    P = len(s)
    A, Ow, t = _pair_args(P, poses, centres, th)
    prm, keep = _params(camera, bounds, scale or scale_tables(), 0, 0.0, cos2_limit, False, 0, 0)
    if P == 0:
        return []
    sizes = np.diff(points.offsets)[s]
    total = int(sizes.sum())
    ctx = ctx or points.ctx
    sp = points._struct(ctx)
    m = _Buffers(ctx)
    try:
        tabs = [m.new(sz * total) for sz in (4, 8, 8, 4)]
        check(ctx.lib.slam_proj_match_project(ctx.handle, ctypes.byref(sp), addr(s), addr(A), addr(Ow), addr(t), P, ctypes.byref(prm),
                                              *(b.ptr for b in tabs)))
        return _tables(tabs, total, sizes, False)
    finally:
        m.free()
        del keep


def proj_match_arrays(query, train, query_xy, train_xy, radius: float, size: Tuple[int, int], k: int = 2, taken=None, cell: int = CELL,
                      ctx: Optional[Context] = None) -> Tuple[np.ndarray, np.ndarray]:
    """``knnMatch(query, train, k, mask=W)`` for the window mask W: train row j is a candidate for query row i iff
    ``|x_j - u_i| < radius and |y_j - v_i| < radius`` (strict) and it is not taken.  ``query_xy`` f64 [N,2] are the projected
    pixels (they pass through the gates unchanged: identity pose, unit camera, depth 1).  Returns (idx, dist) int32 [N, k],
    k in {1, 2}, ordered by (distance, train index); missing neighbours (-1, INT32_MAX).  One pair of at most 8192 rows a
    side; with a window that covers the image this is ``knn_match_arrays``."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or int(k) not in (1, 2):
        raise ValueError(f"k must be 1 or 2, got {k!r}")
    q, t = as_descriptors(query), as_descriptors(train)
    if max(len(q), len(t)) > ROWS_MAX:
        raise ValueError(f"at most {ROWS_MAX} rows per image")
    uv = _f64_rows(query_xy, len(q), 2, "query_xy")
    ctx = ctx or default_context()
    fr = FrameGrids.from_arrays(t, train_xy, np.zeros(len(t), np.int32), size, taken=taken, cell=cell, ctx=ctx)
    try:
        ps = PointSets(np.c_[uv, np.ones(len(q))], q, ctx=ctx)
        try:
            _, _, tab = search_by_projection(ps, fr, [(0, 0)], np.eye(4)[None], np.zeros((1, 3)), bounds=(-np.inf, np.inf, -np.inf, np.inf),
                                             scale=scale_tables(1, 1.0), th=radius, return_tables=True, ctx=ctx)
        finally:
            ps.free()
    finally:
        fr.free()
    return np.ascontiguousarray(tab[0]["idx"][:, :int(k)]), np.ascontiguousarray(tab[0]["dist"][:, :int(k)])


def _compose(S: np.ndarray, T: np.ndarray) -> np.ndarray:
    """[3,4] of x -> S (T x)."""
    return np.c_[S[:, :3] @ T[:, :3], S[:, :3] @ T[:, 3] + S[:, 3]]


def _invert(S: np.ndarray) -> np.ndarray:
    Mi = np.linalg.inv(S[:, :3])
    return np.c_[Mi, -Mi @ S[:, 3]]


def search_by_sim3(points1: PointSets, frames1: FrameGrids, rows1: Sequence, points2: PointSets, frames2: FrameGrids, rows2: Sequence, pairs,
                   poses1, poses2, S12, camera, scale=None, th: float = 7.5, th_high: int = TH_HIGH, ratio: float = np.inf,
                   ctx: Optional[Context] = None) -> List[Tuple[np.ndarray, np.ndarray]]:
    """ORB-SLAM's ``ORBmatcher::SearchBySim3`` for P keyframe pairs.  Pair p = (a, b): keyframe a with its map points
    ``points1`` set a, frame a of ``frames1`` and ``rows1[a]`` (int [P_a]: the feature row of frame a each point was seen at);
    keyframe b likewise on side 2.  ``poses1[p]`` / ``poses2[p]``: world -> camera of the two keyframes; ``S12[p]`` f64 [3,4]
    = ``[s R | t]`` taking camera-2 coordinates into camera 1.  The points of a are searched in frame b under
    ``S12^-1 poses1`` and the points of b in frame a under ``S12 poses2`` (two calls of ``search_by_projection``; no ratio
    test by default, as in ORB-SLAM); on the host the matches both directions agree on are kept.  Returns per pair
    ``(i1, i2)``: int32 indices into the two point sets, i1 ascending - one pair of ``estimate_sim3_batch``."""
    p = _pairs_arg(pairs, len(points1), len(points2))
    P = len(p)
    if len(frames1) != len(points1) or len(frames2) != len(points2) or len(rows1) != len(points1) or len(rows2) != len(points2):
        raise ValueError("every keyframe has one point set, one frame and one rows array")
    T1, T2 = _poses_arg(poses1, P), _poses_arg(poses2, P)
    S = _poses_arg(S12, P)
    if P == 0:
        return []
    A12 = np.stack([_compose(_invert(S[i]), T1[i]) for i in range(P)])      # world -> camera 2 for the points of keyframe 1
    A21 = np.stack([_compose(S[i], T2[i]) for i in range(P)])
    kw = dict(camera=camera, scale=scale, th=th, th_high=th_high, ratio=ratio, ctx=ctx)
    m12, _ = search_by_projection(points1, frames2, p, A12, **kw)
    m21, _ = search_by_projection(points2, frames1, p[:, ::-1].copy(), A21, **kw)
    out = []
    for i, (a, b) in enumerate(p):
        r1, r2 = np.asarray(rows1[a], np.int64).reshape(-1), np.asarray(rows2[b], np.int64).reshape(-1)
        if len(r1) != len(m12[i]) or len(r2) != len(m21[i]):
            raise ValueError("rows1 / rows2 must name one feature row per point")
        point_of_row2 = np.full(int(np.diff(frames2.offsets)[b]) + 1, -1, np.int64)
        point_of_row2[r2] = np.arange(len(r2))
        i1 = np.flatnonzero(m12[i] >= 0)
        k = point_of_row2[m12[i][i1]]
        ok = (k >= 0) & (m21[i][np.maximum(k, 0)] == r1[i1]) if len(i1) and len(r2) else np.zeros(len(i1), bool)
        out.append((i1[ok].astype(np.int32), k[ok].astype(np.int32)))
    return out
