"""Map-point fusion and the refresh of fused points (``slam_fuse_*``): ORB-SLAM's ``ORBmatcher::Fuse`` as
``LocalMapping::SearchInNeighbors`` and ``LoopClosing::SearchAndFuse`` call it, batched over (point set, frame, pose) pairs, the
merge of the links it returns (``apply_fusion``, numpy on the host), and ``MapPoint::ComputeDistinctiveDescriptors`` with
``MapPoint::UpdateNormalAndDepth`` for the points it touched.

The reference has no fusion step.  PARITY UNPINNED: integers and f64 in a stated operation order; a deterministic one-to-one
step and deterministic merge rules in place of ORB-SLAM's iteration order, a unit normal instead of the mean of the views, the
chi-square gate as a product instead of a division, and at most 256 observations per point.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np

from ._args import _Buffers, _down_split, _f64_rows, _int_rows, _pairs_arg
from ._lib import FuseParams, addr, check, load
from .device import Context, default_context
from .matching import as_descriptors
from .proj_match import (CELL, COS2_LIMIT, LEVELS_MAX, PAIRS_MAX, ROWS_MAX, FrameGrids, PointSets, _default_bounds, _pair_args,  # noqa: F401
                         _params, scale_tables)

OBS_MAX = 256                                   # SLAM_FUSE_OBS_MAX
POINTS_MAX = 1 << 24
TH, TH_LOW, CHI2 = 3.0, 50, 5.99                # SearchInNeighbors' radius factor, ORBmatcher::TH_LOW, Fuse's chi-square bound
MARGINS = (0.64, 1.44)                          # 0.8^2, 1.2^2: the range gate's margins, squared
STATUS = ("linked", "behind", "out of bounds", "out of range", "off the normal", "observed", "no candidate", "too far", "lost the row")


def limits() -> dict:
    """The library's limits (``slam_fuse_limits``); needs no GPU."""
    lim = (ctypes.c_int32 * 8)()
    check(load().slam_fuse_limits(lim))
    assert (lim[0], lim[1], lim[3], lim[4]) == (ROWS_MAX, PAIRS_MAX, LEVELS_MAX, OBS_MAX), "the library's limits are not this module's"
    return {"rows_per_image": lim[0], "pairs_per_call": lim[1], "scan_lanes": lim[2], "levels": lim[3], "observations": lim[4],
            "pair_bytes": lim[5], "job_bytes": lim[6], "refresh_threads": lim[7]}


class MapObservations:
    """The observations of M map points in compressed rows: ``offsets`` int64 [M+1] and ``obs`` int32 [nnz,2] = (frame, row
    inside that frame); inside a point's list the frames ascend strictly (a point is seen once per frame), and a list holds at
    most 256 entries.  Both arrays stay readable on the host; the device copy is made at the first call that needs it and
    stays resident until ``free``."""

    def __init__(self, offsets: np.ndarray, obs: np.ndarray, ctx: Optional[Context] = None):
        self.offsets, self.obs, self.ctx = offsets, obs, ctx
        self.device: Optional[dict] = None

    def __len__(self) -> int:
        return len(self.offsets) - 1

    @property
    def nnz(self) -> int:
        return int(self.offsets[-1])

    @property
    def nobs(self) -> np.ndarray:
        """int64 [M]: the length of each list."""
        return np.diff(self.offsets)

    def list(self, m: int) -> np.ndarray:
        return self.obs[self.offsets[m]:self.offsets[m + 1]]

    def lists(self) -> List[List[Tuple[int, int]]]:
        return [[(int(f), int(r)) for f, r in self.list(m)] for m in range(len(self))]

    @classmethod
    def from_arrays(cls, offsets, obs, ctx: Optional[Context] = None) -> "MapObservations":
        off = np.asarray(offsets)
        if off.dtype.kind not in "iu" or off.ndim != 1 or len(off) < 1:
            raise ValueError("offsets must be integers of shape [M + 1]")
        off = np.ascontiguousarray(off, np.int64)
        if len(off) - 1 > POINTS_MAX:
            raise ValueError(f"at most {POINTS_MAX} map points")
        o = np.asarray(obs)
        if o.size == 0:
            o = np.zeros((0, 2), np.int32)
        if o.dtype.kind not in "iu" or o.ndim != 2 or o.shape[1] != 2:
            raise ValueError(f"obs must be integers of shape [nnz, 2], got {o.dtype} {o.shape}")
        if off[0] != 0 or off[-1] != len(o) or (np.diff(off) < 0).any():
            raise ValueError(f"offsets must ascend from 0 to {len(o)}")
        if len(off) > 1 and np.diff(off).max() > OBS_MAX:
            raise ValueError(f"at most {OBS_MAX} observations per map point")
        if len(o) and (o.min() < 0 or o.max() >= 1 << 31):
            raise ValueError("frames and rows must lie in [0, 2^31)")
        o = np.ascontiguousarray(o, np.int32)
        if len(o) > 1:
            inside = np.ones(len(o) - 1, bool)
            inside[off[1:-1][(off[1:-1] > 0) & (off[1:-1] < len(o))] - 1] = False     # (the step from one list into the next)
            if (inside & (np.diff(o[:, 0].astype(np.int64)) <= 0)).any():
                raise ValueError("the frames of an observation list must ascend strictly")
        return cls(off, o, ctx)

    @classmethod
    def from_lists(cls, lists: Sequence, ctx: Optional[Context] = None) -> "MapObservations":
        """``lists[m]``: the (frame, row) pairs of map point m, frames strictly ascending."""
        off = np.zeros(len(lists) + 1, np.int64)
        off[1:] = np.cumsum([len(x) for x in lists])
        flat = [np.asarray(x).reshape(-1, 2) for x in lists if len(x)]
        return cls.from_arrays(off, np.concatenate(flat) if flat else np.zeros((0, 2), np.int32), ctx)

    def _resident(self, ctx: Context) -> dict:
        if self.ctx is None:
            self.ctx = ctx
        if self.ctx is not ctx:
            raise ValueError("the observations belong to another context")
        if self.device is None:
            pad = lambda a: a if a.size else np.zeros(2, a.dtype)  # noqa: E731
            dev = {"offsets": ctx.upload(self.offsets), "obs": None}
            try:
                dev["obs"] = ctx.upload(pad(self.obs))
            except BaseException:
                dev["offsets"].free()
                raise
            self.device = dev
        return self.device

    def free(self) -> None:
        if self.device is not None:
            for b in self.device.values():
                if b is not None:
                    b.free()
            self.device = None


def _ids_arg(a, n: int, name: str, M: int) -> np.ndarray:
    return np.ascontiguousarray(_int_rows(a, n, name, -1, M, "iu", f"be -1 or a map point in [0, {M})"), np.int32)


def _fuse_params(th_low, margins, chi2) -> FuseParams:
    if isinstance(th_low, bool) or int(th_low) != th_low or not 0 <= th_low <= 256:
        raise ValueError("th_low must be an integer in [0, 256]")
    lo2, hi2 = float(margins[0]), float(margins[1])
    if not (lo2 > 0.0 and hi2 > 0.0):
        raise ValueError("the margins must be positive numbers")
    chi2 = float(chi2)
    if chi2 != chi2:
        raise ValueError("chi2 is not a number")
    return FuseParams(lo2, hi2, chi2, int(th_low), 0)


def fuse_points(points: PointSets, ids, frames: FrameGrids, frame_points, obs: MapObservations, pairs, poses, centres=None,
                camera=(1.0, 1.0, 0.0, 0.0), bounds=None, scale=None, th=TH, th_low: int = TH_LOW, margins=MARGINS, chi2: float = CHI2,
                cos2_limit: float = COS2_LIMIT, level_offsets=(-1, 0), return_tables: bool = False, ctx: Optional[Context] = None):
    """``ORBmatcher::Fuse`` for P pairs in one copy, one memset and two launches.  ``points`` with ``ids`` int
    [points.n] (the map point of each point, -1: none); ``frames`` built WITHOUT taken marks, with ``frame_points`` int
    [frames.n] in ROW order (the map point each row holds, -1: none); ``obs`` the observation table of the map; ``pairs``,
    ``poses``, ``centres``, ``camera``, ``bounds``, ``scale`` and ``th`` as ``search_by_projection`` takes them (a Sim(3) pose
    ``[sR | t]`` included).  ``margins`` are the SQUARED factors of the range gate, (1, 1) the gate of ``search_by_projection``.

    Per point the first status that applies: 5 observed in the pair's frame already; 1 - 4 the gates; 6 no frame row strictly
    inside the window, on a level in ``level_offsets`` around the predicted one, within ``chi2 * sigma2[level]`` of the
    projection; 7 the nearest such row is farther than ``th_low``; 8 another point took the row with a smaller (distance,
    point); 0 linked.  Returns (results, counts int32 [P,3]): per pair a dict ``row`` (-1 unless status 0, 7, 8), ``dist``,
    ``status``, ``other`` (status 0: ``frame_points`` of the row, -1 = the point gains an observation; status 8: the id of the
    winner), ``id`` (the pair's slice of ``ids``) and ``frame``; with ``return_tables`` also ``u``, ``v``, ``lp``.  counts =
    (added, merged, lost)."""
    if not isinstance(points, PointSets) or not isinstance(frames, FrameGrids) or not isinstance(obs, MapObservations):
        raise ValueError("fuse_points takes PointSets, FrameGrids and MapObservations")
    p = _pairs_arg(pairs, len(points), len(frames))
    P = len(p)
    A, Ow, t = _pair_args(P, poses, centres, th)
    lo, hi = int(level_offsets[0]), int(level_offsets[1])
    prm, keep = _params(camera, _default_bounds(frames) if bounds is None else bounds, scale or scale_tables(), 0, 0.0, cos2_limit, True, lo, hi)
    fp = _fuse_params(th_low, margins, chi2)
    id1 = _ids_arg(ids, points.n, "ids", len(obs))
    pt2 = _ids_arg(frame_points, frames.n, "frame_points", len(obs))
    if P == 0:
        return [], np.zeros((0, 3), np.int32)
    sizes = np.diff(points.offsets)[p[:, 0]]
    total = int(sizes.sum())
    ctx = ctx or points.ctx
    sp, sf = points._struct(ctx), frames._struct(ctx)
    ob = obs._resident(ctx)
    m = _Buffers(ctx)
    try:
        d_id, d_pt = m.up(id1), m.up(pt2)
        out = [m.new(4 * total) for _ in range(4)]
        d_c = m.new(12 * P)
        tabs = [m.new(sz * total) for sz in (8, 8, 4)] if return_tables else [None] * 3
        check(ctx.lib.slam_fuse_search(ctx.handle, ctypes.byref(sp), d_id.ptr, ctypes.byref(sf), d_pt.ptr, addr(obs.offsets), ob["offsets"].ptr,
                                       ob["obs"].ptr, len(obs), addr(p), addr(A), addr(Ow), addr(t), P, ctypes.byref(prm), ctypes.byref(fp),
                                       *(b.ptr for b in out), d_c.ptr, *(b.ptr if b else None for b in tabs)))
        counts = d_c.download(np.int32, (P, 3))
        down = lambda b, dt: _down_split(b, dt, (), total, sizes)  # noqa: E731
        cols = dict(zip(("row", "dist", "status", "other"), (down(b, np.int32) for b in out)))
        if return_tables:
            cols.update(u=down(tabs[0], np.float64), v=down(tabs[1], np.float64), lp=down(tabs[2], np.int32))
        res = []
        for i, (a, b) in enumerate(p):
            d = {k: cols[k][i] for k in cols}
            d["id"] = id1[points.offsets[a]:points.offsets[a + 1]].copy()
            d["frame"] = int(b)
            res.append(d)
        return res, counts
    finally:
        m.free()
        del keep


def fuse_by_sim3(points: PointSets, ids, frames: FrameGrids, frame_points, obs: MapObservations, pairs, sims, centres=None, th=4.0, **kw):
    """``LoopClosing::SearchAndFuse``: ``fuse_points`` with the similarity ``sims[p]`` = ``[sR | t]`` f64 [P,3,4] taking world
    coordinates into the camera of the pair's frame (the gates take it as they take a rigid pose; the centres default to
    ``-(sR)^-1 t``) and ORB-SLAM's radius factor 4."""
    return fuse_points(points, ids, frames, frame_points, obs, pairs, sims, centres, th=th, **kw)


def refresh_map_points(xyz, obs: MapObservations, frames: FrameGrids, centres, ref=None, scale=None, select=None,
                       ctx: Optional[Context] = None) -> dict:
    """``MapPoint::ComputeDistinctiveDescriptors`` and ``UpdateNormalAndDepth`` for the map points ``select`` (int [K]; None:
    all M) of ``obs`` in up to three launches.  ``xyz`` f64 [M,3]; ``frames``: the frames the observations name; ``centres``
    f64 [B,3] the camera centres; ``ref`` int [M]: the index inside its list of each point's reference observation (None: 0).

    Returns a dict, in ``select`` order: ``best`` int32 [K] - the observation with the smallest (median distance to the
    others, index), the median being the element of rank (N - 1) // 2 of its row of the N x N Hamming table - with its
    ``descriptors`` u8 [K,32]; ``normal`` f64 [K,3], the unit vector of the sum of the unit views in list order; ``dmin2``,
    ``dmax2`` f64 [K] from the reference observation.  An empty list: -1, zero bytes, NaN."""
    if not isinstance(obs, MapObservations) or not isinstance(frames, FrameGrids):
        raise ValueError("refresh_map_points takes MapObservations and FrameGrids")
    M, B = len(obs), len(frames)
    X = _f64_rows(xyz, M, 3, "xyz")
    C = _f64_rows(centres, B, 3, "centres")
    s = np.ascontiguousarray((scale or scale_tables())[0], np.float64).reshape(-1)
    if not 1 <= len(s) <= LEVELS_MAX:
        raise ValueError(f"scale is the pair of tables of scale_tables, 1 to {LEVELS_MAX} levels each")
    rf = None if ref is None else _ids_arg(ref, M, "ref", OBS_MAX)
    if rf is not None and M and (rf < 0).any():
        raise ValueError("ref must not be negative")
    sel = None
    if select is not None:
        sel = np.asarray(select)
        if sel.size == 0:
            sel = np.zeros(0, np.int32)
        if sel.dtype.kind not in "iu" or sel.ndim != 1 or (len(sel) and (sel.min() < 0 or sel.max() >= M)) or len(sel) > POINTS_MAX:
            raise ValueError(f"select must be map points in [0, {M})")
        sel = np.ascontiguousarray(sel, np.int32)
    if obs.nnz and (obs.obs[:, 0].max() >= B or (obs.obs[:, 1] >= np.diff(frames.offsets)[obs.obs[:, 0]]).any()):
        raise ValueError("an observation names a frame or a row outside the frames")
    K = M if sel is None else len(sel)
    if K == 0:
        return dict(best=np.zeros(0, np.int32), descriptors=np.zeros((0, 32), np.uint8), normal=np.zeros((0, 3)), dmin2=np.zeros(0),
                    dmax2=np.zeros(0))
    ctx = ctx or frames.ctx
    sf = frames._struct(ctx)
    ob = obs._resident(ctx)
    m = _Buffers(ctx)
    try:
        d_x, d_c = m.up(X), m.up(C)
        d_r = m.up(rf) if rf is not None else None
        out = [m.new(sz * K) for sz in (4, 32, 24, 16)]
        check(ctx.lib.slam_fuse_refresh(ctx.handle, d_x.ptr, addr(obs.offsets), ob["obs"].ptr, M, addr(sel) if sel is not None else None, K,
                                        sf.d_desc, frames.device["inverse"].ptr, sf.d_level, addr(frames.offsets), B, d_c.ptr,
                                        d_r.ptr if d_r else None, addr(s), len(s), *(b.ptr for b in out)))
        rg = out[3].download(np.float64, (K, 2))
        return dict(best=out[0].download(np.int32, (K,)), descriptors=out[1].download(np.uint8, (K, 32)),
                    normal=out[2].download(np.float64, (K, 3)), dmin2=np.ascontiguousarray(rg[:, 0]), dmax2=np.ascontiguousarray(rg[:, 1]))
    finally:
        m.free()


def _find(parent: list, a: int) -> int:
    while parent[a] != a:
        parent[a] = parent[parent[a]]
        a = parent[a]
    return a


def apply_fusion(obs: MapObservations, results) -> Tuple[MapObservations, np.ndarray, np.ndarray]:
    """The links of ``fuse_points`` applied to the observation table; numpy on the host, the same answer for every order of
    ``results``.  Classes: the union of m ~ q over every status-0 link with ``other`` = q >= 0, every status-8 link (m and the
    winner q), and over the points that gain an observation on one and the same (frame, row).  The survivor of a class has the
    most observations, ties to the smallest id.  Its new list is the union of its members' lists and of their "add" links;
    where that names two rows in one frame the survivor's own row is kept, else the smallest.  Every other member's list is
    empty.  Links of points without an id (-1) are dropped.

    Returns (the new ``MapObservations``, ``alias`` int32 [M] - the survivor of each point's class - and ``updates`` int32
    [K,3] = (frame, row, id) sorted: the frame rows whose map point changes, id = -1 for a row that lost its point)."""
    if not isinstance(obs, MapObservations):
        raise ValueError("apply_fusion takes MapObservations")
    M = len(obs)
    nobs = obs.nobs
    parent = list(range(M))

    def union(a: int, b: int) -> None:
        a, b = _find(parent, a), _find(parent, b)
        if a != b:
            parent[max(a, b)] = min(a, b)

    adds, first = [], {}
    for r in results:
        ids, st, ot, rw = (np.asarray(r[k]).reshape(-1) for k in ("id", "status", "other", "row"))
        f = int(r["frame"])
        if ids.size and ids.max() >= M:
            raise ValueError("a result names a map point outside the table")
        for i in np.flatnonzero(((st == 0) | (st == 8)) & (ids >= 0)):
            m, q = int(ids[i]), int(ot[i])
            if st[i] == 0 and q < 0:
                adds.append((m, f, int(rw[i])))
                union(m, first.setdefault((f, int(rw[i])), m))
            elif 0 <= q < M:
                union(m, q)
    classes = {}
    for m in range(M):
        classes.setdefault(_find(parent, m), []).append(m)
    alias = np.arange(M, dtype=np.int32)
    for ms in classes.values():
        alias[ms] = min(ms, key=lambda m: (-int(nobs[m]), m))
    gained = {}
    for m, f, r in adds:
        gained.setdefault(int(alias[m]), []).append((f, r))
    lists = [obs.list(m) for m in range(M)]
    before, after = {}, {}
    for ms in classes.values():
        s = int(alias[ms[0]])
        if len(ms) == 1 and s not in gained:
            continue
        own = {int(f): int(r) for f, r in obs.list(s)}
        kept = dict(own)
        for f, r in sorted([(int(f), int(r)) for m in ms if m != s for f, r in obs.list(m)] + gained.get(s, [])):
            if f not in own:
                kept[f] = min(kept.get(f, r), r)
        for f, r in gained.get(s, []):
            before[(f, r)] = -1
        for m in ms:
            for f, r in obs.list(m):
                before[(int(f), int(r))] = m
            lists[m] = np.zeros((0, 2), np.int32)
        lists[s] = np.array(sorted(kept.items()), np.int32).reshape(-1, 2)
        for f, r in kept.items():
            after[(f, r)] = s
    upd = sorted((f, r, after.get((f, r), -1)) for (f, r), was in before.items() if after.get((f, r), -1) != was)
    return MapObservations.from_lists(lists, obs.ctx), alias, np.array(upd, np.int32).reshape(-1, 3)


def fuse_arrays(query, train, query_xy, train_xy, train_level, radius: float, size: Tuple[int, int], scale=None, chi2: float = CHI2,
                th_low: int = 256, level_offsets=(0, LEVELS_MAX), train_points=None, cell: int = CELL,
                ctx: Optional[Context] = None) -> Tuple[np.ndarray, np.ndarray]:
    """The candidate rule of ``fuse_points`` for one pair as a masked nearest-neighbour search - the mirror of
    ``proj_match_arrays``: train row j is a candidate for query row i iff it lies strictly inside the window of ``radius``
    about ``query_xy[i]`` (f64 [N,2]; they pass through the gates unchanged: identity pose, unit camera, depth 1), on a level
    in ``level_offsets`` (the predicted level is 0) and within ``chi2 * sigma2[level_j]`` of it.  Returns (row, dist) int32
    [N]: the nearest candidate by (distance, row) BEFORE the one-to-one step, (-1, INT32_MAX) where there is none."""
    q, t = as_descriptors(query), as_descriptors(train)
    if max(len(q), len(t)) > ROWS_MAX:
        raise ValueError(f"at most {ROWS_MAX} rows per image")
    uv = _f64_rows(query_xy, len(q), 2, "query_xy")
    ctx = ctx or default_context()
    fr = FrameGrids.from_arrays(t, train_xy, train_level, size, cell=cell, ctx=ctx)
    ps = ob = None
    try:
        ps = PointSets(np.c_[uv, np.ones(len(q))], q, ctx=ctx)
        ob = MapObservations.from_lists([], ctx)
        res, _ = fuse_points(ps, np.full(len(q), -1), fr, np.full(len(t), -1) if train_points is None else train_points, ob, [(0, 0)],
                             np.eye(4)[None], np.zeros((1, 3)), bounds=(-np.inf, np.inf, -np.inf, np.inf), scale=scale or scale_tables(),
                             th=radius, th_low=th_low, chi2=chi2, level_offsets=level_offsets, ctx=ctx)
    finally:
        for x in (ps, ob, fr):
            if x is not None:
                x.free()
    return res[0]["row"], res[0]["dist"]
