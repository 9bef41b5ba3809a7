"""Local-map selection and keyframe culling (``slam_lmap_*``): ``Tracking::UpdateLocalKeyFrames`` (the vote on
the device, the expansion over a ``CovisibilityGraph`` on the host), ``UpdateLocalPoints``, ``LocalMapping::KeyFrameCulling``
and ``MapPointCulling`` over the tables a ``fuse_points`` call leaves resident: the observations of every point, the point of
every frame row and the pyramid level of every row.

The reference keeps a sliding window by distance and no observation counts.  PARITY UNPINNED: integers only, every output a
function of the input alone; index order where ORB-SLAM follows container and pointer order.  There is no CPU fallback: the
``*_host`` functions are the numpy statements the device is held to, bit for bit.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np

from ._args import _Buffers
from ._lib import addr, check, load
from .covis import CovisibilityGraph
from .device import Context, default_context
from .fuse import OBS_MAX, POINTS_MAX, MapObservations
from .proj_match import FrameGrids

LIMIT_NAMES = ("threads", "vote_lds_small", "vote_lds_frames", "group16", "group64", "group256", "scan_tile_words", "scalar_bytes")
WORKSPACE_NAMES = ("frame_points", "vote", "points", "cull")
FRAMES_MAX = 1 << 24
QUERIES_MAX = 65535
VOTE_FORMS = {"auto": 0, "lds16": 1, "lds": 2, "global": 3}


def limits() -> dict:
    """The library's constants (``slam_lmap_limits``); needs no device.  ``vote_lds_small`` / ``vote_lds_frames``: the number
    of frames up to which the vote keeps its counters in 16 KiB / in all the LDS of a CU (above: global memory); ``group*``:
    the lanes a row of the culling kernel gets, by the length of its point's list."""
    lim = (ctypes.c_int32 * 8)()
    check(load().slam_lmap_limits(lim))
    assert lim[5] == OBS_MAX, "the library's limits are not this module's"
    return dict(zip(LIMIT_NAMES, lim))


def workspace_bytes(B: int, F: int, M: int, C: int = 0) -> dict:
    """Bytes of the four workspaces (``slam_lmap_workspace``); needs no device."""
    n = (ctypes.c_uint64 * 4)()
    check(load().slam_lmap_workspace(int(B), int(F), int(M), int(C), n))
    return dict(zip(WORKSPACE_NAMES, (int(v) for v in n)))


def _new(ctx: Context, held: Optional[_Buffers], nbytes: int, role: str):
    """Every device block this module allocates comes from here, and is freed with ``held`` where one is given.  ``role`` -
    "ws" for a workspace, "out" for an output - is not read here: it is there for the GPU tests, which replace this function
    to fill workspaces and outputs with different bytes before a call and to hand the same blocks out a second time."""
    b = ctx.malloc(max(int(nbytes), 16))
    if held is not None:
        held.bufs.append(b)
    return b


# ---- arguments ----------------------------------------------------------------------------------------------------------------------
def _mask(mask, n: int, name: str) -> Optional[np.ndarray]:
    if mask is None:
        return None
    a = np.asarray(mask)
    if a.dtype.kind not in "biu" or a.shape != (n,):
        raise ValueError(f"{name} must be a mask of shape [{n}], got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a != 0, np.uint8)


def _frame_offsets(offsets) -> np.ndarray:
    off = np.asarray(offsets)
    if off.dtype.kind not in "iu" or off.ndim != 1 or len(off) < 2:
        raise ValueError("frame_offsets must be integers of shape [F + 1], F >= 1")
    off = np.ascontiguousarray(off, np.int64)
    if off[0] != 0 or (np.diff(off) < 0).any() or off[-1] >= 1 << 31 or len(off) - 1 > FRAMES_MAX:
        raise ValueError("frame_offsets must ascend from 0 and end below 2^31")
    return off


def _lists(x, offsets, name: str) -> Tuple[np.ndarray, np.ndarray]:
    """B lists of integers as (flat int32, offsets int64 [B+1]): a flat array with ``offsets``, a sequence of sequences, or one
    list (B = 1)."""
    if offsets is None:
        many = isinstance(x, (list, tuple)) and (len(x) == 0 or not np.isscalar(x[0]))
        parts = [np.asarray(p).reshape(-1) for p in (x if many else [x])]
        if any(p.size and p.dtype.kind not in "iu" for p in parts):
            raise ValueError(f"{name} must be integer lists")
        offsets = np.zeros(len(parts) + 1, np.int64)
        offsets[1:] = np.cumsum([len(p) for p in parts])
        x = np.concatenate([p.astype(np.int64) for p in parts]) if parts else np.zeros(0, np.int64)
    a = np.asarray(x)
    if a.size == 0:
        a = np.zeros(0, np.int64)
    off = np.asarray(offsets)
    if a.dtype.kind not in "iu" or a.ndim != 1 or off.dtype.kind not in "iu" or off.ndim != 1 or len(off) < 1:
        raise ValueError(f"{name} must be integer lists, with integer offsets of shape [B + 1]")
    off = np.ascontiguousarray(off, np.int64)
    if off[0] != 0 or off[-1] != len(a) or (np.diff(off) < 0).any():
        raise ValueError(f"the offsets of {name} must ascend from 0 to {len(a)}")
    if len(off) - 1 > QUERIES_MAX:
        raise ValueError(f"at most {QUERIES_MAX} queries per call")
    if len(a) and (a.min() < -(1 << 31) or a.max() >= 1 << 31):
        raise ValueError(f"{name} must fit 32 bits")
    return np.ascontiguousarray(a, np.int32), off


def _th_obs(th_obs) -> int:
    if isinstance(th_obs, bool) or int(th_obs) != th_obs or not 0 <= th_obs <= OBS_MAX:
        raise ValueError(f"th_obs must be an integer in [0, {OBS_MAX}]")
    return int(th_obs)


def _candidates(candidates, F: int) -> Optional[np.ndarray]:
    if candidates is None:
        return None
    c = np.asarray(candidates)
    if c.size == 0:
        c = np.zeros(0, np.int64)
    if c.dtype.kind not in "iu" or c.ndim != 1 or (len(c) and (c.min() < 0 or c.max() >= F)) or len(c) > FRAMES_MAX:
        raise ValueError(f"candidates must be frames in [0, {F})")
    return np.ascontiguousarray(c, np.int32)


def _ranges(starts: np.ndarray, lengths: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """The integers of the ranges [starts[i], starts[i] + lengths[i]) one after the other, and the range each lies in."""
    lengths = np.asarray(lengths, np.int64)
    total = int(lengths.sum())
    first = np.cumsum(lengths) - lengths
    owner = np.repeat(np.arange(len(lengths), dtype=np.int64), lengths)
    return np.repeat(np.asarray(starts, np.int64) - first, lengths) + np.arange(total, dtype=np.int64), owner


# ---- the numpy statements -------------------------------------------------------------------------------------------------------------
def frame_points_host(obs: MapObservations, frame_offsets) -> Tuple[np.ndarray, int, int]:
    """``slam_lmap_frame_points`` in numpy -> (frame_points int32 [n], slots out of range, claims of a row that had a point);
    a row claimed twice holds the greatest claimant."""
    fo = _frame_offsets(frame_offsets)
    F, n = len(fo) - 1, int(fo[-1])
    f, r = obs.obs[:, 0].astype(np.int64), obs.obs[:, 1].astype(np.int64)
    m = np.repeat(np.arange(len(obs), dtype=np.int64), obs.nobs)
    ok = (f >= 0) & (f < F)
    ok[ok] &= (r[ok] >= 0) & (r[ok] < np.diff(fo)[f[ok]])
    at = fo[f[ok]] + r[ok]
    fp = np.full(n, -1, np.int32)
    np.maximum.at(fp, at, m[ok].astype(np.int32))
    return fp, int((~ok).sum()), int(len(at) - len(np.unique(at)))


def votes_host(obs: MapObservations, F: int, query_points, offsets=None, frame_removed=None, point_bad=None) -> dict:
    """``slam_lmap_vote`` in numpy: the dict of ``local_keyframe_votes``."""
    q, off = _lists(query_points, offsets, "query_points")
    M, B = len(obs), len(off) - 1
    rem, bad = _mask(frame_removed, F, "frame_removed"), _mask(point_bad, M, "point_bad")
    votes = np.zeros((B, F), np.int32)
    skipped = 0
    for b in range(B):
        m = q[off[b]:off[b + 1]].astype(np.int64)
        m = m[m != -1]
        inside = (m >= 0) & (m < M)
        skipped += int((~inside).sum())
        m = m[inside]
        if bad is not None:
            m = m[bad[m] == 0]
        slots = _ranges(obs.offsets[m], obs.offsets[m + 1] - obs.offsets[m])[0]
        f = obs.obs[slots, 0].astype(np.int64)
        inside = (f >= 0) & (f < F)
        skipped += int((~inside).sum())
        f = f[inside]
        if rem is not None:
            f = f[rem[f] == 0]
        votes[b] = np.bincount(f, minlength=F)[:F]
    best = np.stack([votes.argmax(1), votes.max(1)], 1).astype(np.int32) if F else np.zeros((B, 2), np.int32)
    best[best[:, 1] == 0] = (-1, 0)
    return dict(votes=votes, best=best, nvoted=(votes > 0).sum(1).astype(np.int32), skipped=skipped)


def local_points_host(frame_points, frame_offsets, M: int, local_keyframes, query_points, lkf_offsets=None, offsets=None, frame_removed=None,
                      point_bad=None) -> List[np.ndarray]:
    """``slam_lmap_points_mark`` / ``_fill`` in numpy: per query the points (ascending, each once) of the rows of its local
    keyframes, without bad points and without the query's own."""
    fo = _frame_offsets(frame_offsets)
    F = len(fo) - 1
    fp = np.asarray(frame_points, np.int64)
    lk, lo = _lists(local_keyframes, lkf_offsets, "local_keyframes")
    q, off = _lists(query_points, offsets, "query_points")
    if len(lo) != len(off):
        raise ValueError("one list of local keyframes per query")
    rem, bad = _mask(frame_removed, F, "frame_removed"), _mask(point_bad, M, "point_bad")
    out = []
    for b in range(len(off) - 1):
        seen = np.zeros(M, bool)
        for f in lk[lo[b]:lo[b + 1]]:
            if 0 <= f < F and not (rem is not None and rem[f]):
                m = fp[fo[f]:fo[f + 1]]
                m = m[(m >= 0) & (m < M)]
                seen[m] = True
        if bad is not None:
            seen[bad != 0] = False
        own = q[off[b]:off[b + 1]].astype(np.int64)
        seen[own[(own >= 0) & (own < M)]] = False
        out.append(np.flatnonzero(seen).astype(np.int32))
    return out


def keyframe_redundancy_host(obs: MapObservations, frame_points, level, frame_offsets, candidates=None, th_obs: int = 3, frame_removed=None,
                             point_bad=None) -> Tuple[np.ndarray, np.ndarray]:
    """``slam_lmap_cull_count`` in numpy -> (counts int32 [C,2] = (n_points, n_redundant), flags u8 per candidate row)."""
    fo = _frame_offsets(frame_offsets)
    F, M = len(fo) - 1, len(obs)
    th = _th_obs(th_obs)
    fp, lv = np.asarray(frame_points, np.int64), np.asarray(level, np.int64)
    rem, bad = _mask(frame_removed, F, "frame_removed"), _mask(point_bad, M, "point_bad")
    cand = _candidates(candidates, F)
    cand = np.arange(F, dtype=np.int32) if cand is None else cand
    of, orow = obs.obs[:, 0].astype(np.int64), obs.obs[:, 1].astype(np.int64)
    olevel = lv[fo[of] + orow] if len(of) else np.zeros(0, np.int64)
    gone = np.zeros(F, bool) if rem is None else rem != 0
    rows, ci = _ranges(fo[cand], fo[cand.astype(np.int64) + 1] - fo[cand])      # the candidate rows, the candidates in order
    c = cand.astype(np.int64)[ci]
    m = fp[rows]
    ok = (m >= 0) & ~gone[c]
    if bad is not None:
        ok[ok] &= bad[m[ok]] == 0
    slots, seg = _ranges(obs.offsets[m[ok]], obs.nobs[m[ok]])                       # the observers of every such row
    alive = ~gone[of[slots]]
    near = alive & (of[slots] != c[ok][seg]) & (olevel[slots] <= lv[rows[ok]][seg] + 1)
    n_rows = int(ok.sum())
    N, q = np.bincount(seg[alive], minlength=n_rows), np.bincount(seg[near], minlength=n_rows)
    flags = np.zeros(len(rows), np.uint8)
    flags[ok] = np.where((N > th) & (q >= th), 2, 1)
    counts = np.stack([np.bincount(ci[flags > 0], minlength=len(cand)), np.bincount(ci[flags == 2], minlength=len(cand))], 1).astype(np.int32)
    return counts.reshape(-1, 2), flags


# ---- the resident tables --------------------------------------------------------------------------------------------------------------
class MapTables:
    """What the local-map steps read, resident on the device: the observation table ``obs`` (its own device copy), and for
    the n rows of the F frames ``frame_offsets``: ``d_frame_points`` int32 [n] (the inverse of ``obs``, built on the device),
    ``d_level`` int32 [n], and the byte masks ``d_frame_removed`` [F] and ``d_point_bad`` [M].  ``frame_removed`` and
    ``point_bad`` are the host's copies of the masks; ``cull_keyframes`` updates both sides."""

    def __init__(self, ctx: Context, obs: MapObservations, frame_offsets: np.ndarray):
        self.ctx, self.obs, self.frame_offsets = ctx, obs, frame_offsets
        self.F, self.M, self.n_rows = len(frame_offsets) - 1, len(obs), int(frame_offsets[-1])
        self.max_list = int(obs.nobs.max()) if len(obs) else 0
        self.frame_removed = np.zeros(self.F, np.uint8)
        self.point_bad = np.zeros(self.M, np.uint8)
        self.d_frame_offsets = self.d_frame_points = self.d_level = self.d_frame_removed = self.d_point_bad = None
        self._own_level = True
        self.cull_launches = 0

    @classmethod
    def from_observations(cls, obs: MapObservations, frames, level=None, frame_removed=None, point_bad=None,
                          ctx: Optional[Context] = None) -> "MapTables":
        """``frames``: a ``FrameGrids`` (its offsets and its resident levels are used; it must outlive the tables) or
        ``frame_offsets`` int [F+1] with ``level`` int [n] in row order.  The inverse table is built on the device; a slot of
        ``obs`` that names no frame row, or a row that two points claim, is a ``ValueError`` with nothing left allocated."""
        if not isinstance(obs, MapObservations):
            raise ValueError("MapTables takes MapObservations")
        if len(obs) < 1:
            raise ValueError("the map has no points")
        grids = frames if isinstance(frames, FrameGrids) else None
        fo = _frame_offsets(grids.offsets if grids is not None else frames)
        n = int(fo[-1])
        lv = None
        if grids is None:
            lv = np.asarray(level if level is not None else np.zeros(0, np.int64))
            if lv.dtype.kind not in "iu" or lv.shape != (n,) or (n and (lv.min() < 0 or lv.max() >= 1 << 15)):
                raise ValueError(f"level must be integers in [0, 2^15) of shape [{n}]")
            lv = np.ascontiguousarray(lv, np.int32)
        elif grids.device is None:
            raise ValueError("these frame grids have been freed")
        ctx = ctx or obs.ctx or (grids.ctx if grids is not None else None) or default_context()
        if grids is not None and grids.ctx is not ctx:
            raise ValueError("the frame grids belong to another context")
        t = cls(ctx, obs, fo)
        rem, bad = _mask(frame_removed, t.F, "frame_removed"), _mask(point_bad, t.M, "point_bad")
        dev = obs._resident(ctx)
        ws = None
        try:
            pad = lambda a: a if a.size else np.zeros(4, a.dtype)  # noqa: E731
            t.d_frame_offsets = ctx.upload(fo)
            t.d_frame_points = _new(ctx, None, 4 * n, "out")
            if grids is not None:
                t.d_level, t._own_level = grids.device["level"], False
            else:
                t.d_level = ctx.upload(pad(lv))
            t.d_frame_removed = ctx.upload(t.frame_removed)
            t.d_point_bad = ctx.upload(t.point_bad)
            ws = _new(ctx, None, workspace_bytes(0, t.F, t.M)["frame_points"], "ws")
            s = (ctypes.c_int64 * 2)()
            check(ctx.lib.slam_lmap_frame_points(ctx.handle, t.M, obs.nnz, dev["offsets"].ptr, dev["obs"].ptr, t.F, t.d_frame_offsets.ptr, n,
                                                 t.d_frame_points.ptr, ws.ptr, s))
            if s[0]:
                raise ValueError(f"{s[0]} observations name a frame or a row outside the frames")
            if s[1]:
                raise ValueError(f"{s[1]} claims of a frame row that another map point holds")
            if rem is not None:
                t.set_frame_removed(rem)
            if bad is not None:
                t.set_point_bad(bad)
            return t
        except BaseException:
            t.free()
            raise
        finally:
            if ws is not None:
                ws.free()

    def set_frame_removed(self, mask) -> None:
        self.frame_removed = _mask(mask, self.F, "frame_removed").copy()
        self.d_frame_removed.upload(self.frame_removed)

    def set_point_bad(self, mask) -> None:
        self.point_bad = _mask(mask, self.M, "point_bad").copy()
        self.d_point_bad.upload(self.point_bad)

    def remove_frame(self, f: int) -> None:
        """Marks one frame removed on both sides (one byte crosses)."""
        f = int(f)
        if not 0 <= f < self.F:
            raise ValueError(f"frame {f} is not in [0, {self.F})")
        self.frame_removed[f] = 1
        self.d_frame_removed.view(f, 1).upload(self.frame_removed[f:f + 1])

    def frame_points(self) -> np.ndarray:
        """int32 [n]: the map point of every frame row, -1 = none (downloaded)."""
        return self.d_frame_points.download(np.int32, (self.n_rows,)) if self.n_rows else np.zeros(0, np.int32)

    def level(self) -> np.ndarray:
        return self.d_level.download(np.int32, (self.n_rows,)) if self.n_rows else np.zeros(0, np.int32)

    def _live(self) -> dict:
        if self.d_frame_points is None:
            raise ValueError("these map tables have been freed")
        return self.obs._resident(self.ctx)

    def free(self) -> None:
        """Frees what the tables made; the observations and a ``FrameGrids`` they were built from stay their owners'."""
        for name in ("d_frame_offsets", "d_frame_points", "d_level", "d_frame_removed", "d_point_bad"):
            b = getattr(self, name)
            if b is not None and (name != "d_level" or self._own_level):
                b.free()
            setattr(self, name, None)


def _tables(tables) -> MapTables:
    if not isinstance(tables, MapTables):
        raise ValueError("the local-map steps take MapTables")
    return tables


# ---- the device calls -----------------------------------------------------------------------------------------------------------------
def local_keyframe_votes(tables: MapTables, query_points, offsets=None, form: str = "auto") -> dict:
    """``UpdateLocalKeyFrames``' vote for B query frames in one launch (two in the global-memory form): ``query_points`` the
    map points each frame tracks (a flat array with ``offsets``, a sequence of lists, or one list; -1 and bad points are
    skipped, other entries outside the map are skipped and counted).  Returns a dict: ``votes`` int32 [B,F] - for every
    occurrence of a point, +1 for every frame that observes it and is not removed; ``best`` int32 [B,2] = (the frame with the
    most votes, the lowest on ties; its votes), (-1, 0) without votes; ``nvoted`` int32 [B]; ``skipped``.  ``form``: "auto",
    or "lds16" / "lds" / "global" to force where the counters live (the same bytes).

    How lists are read, here and in ``local_points``: with ``offsets``, ``query_points`` is flat and ``offsets`` int [B+1]
    cuts it.  Without, a Python list or tuple whose first element is not a scalar is B lists (``[]`` is B = 0, ``[[]]`` one
    empty query); anything else - a list of scalars, a numpy array, ``np.array([])`` included - is ONE query.  Pass
    ``[array]`` or ``offsets`` where the kind of the argument is not known in advance."""
    t = _tables(tables)
    q, off = _lists(query_points, offsets, "query_points")
    if form not in VOTE_FORMS:
        raise ValueError(f"form must be one of {sorted(VOTE_FORMS)}")
    B = len(off) - 1
    if B == 0:
        return dict(votes=np.zeros((0, t.F), np.int32), best=np.zeros((0, 2), np.int32), nvoted=np.zeros(0, np.int32), skipped=0)
    if B * t.F >= 1 << 31:
        raise ValueError("B x F votes: more than 2^31 - 1")
    dev, ctx = t._live(), t.ctx
    m = _Buffers(ctx)
    try:
        d_q = m.up(q)
        ws = _new(ctx, m, workspace_bytes(B, t.F, t.M)["vote"], "ws")
        d_v, d_b, d_n = (_new(ctx, m, sz, "out") for sz in (4 * B * t.F, 8 * B, 4 * B))
        skipped = ctypes.c_int64(0)
        check(ctx.lib.slam_lmap_vote(ctx.handle, B, d_q.ptr, addr(off), t.M, t.obs.nnz, dev["offsets"].ptr, dev["obs"].ptr, t.d_point_bad.ptr,
                                     t.F, t.d_frame_removed.ptr, VOTE_FORMS[form], ws.ptr, d_v.ptr, d_b.ptr, d_n.ptr, ctypes.byref(skipped)))
        return dict(votes=d_v.download(np.int32, (B, t.F)), best=d_b.download(np.int32, (B, 2)), nvoted=d_n.download(np.int32, (B,)),
                    skipped=int(skipped.value))
    finally:
        m.free()


def local_keyframes(votes, graph: CovisibilityGraph, limit: int = 80, best: int = 10, query: int = 0, frame_removed=None) -> Tuple[np.ndarray, int]:
    """The second half of ``UpdateLocalKeyFrames``, on the host over a ``CovisibilityGraph``: ``votes`` the dict of
    ``local_keyframe_votes`` (its row ``query``) or an int array [F].  K1 = the voted frames, ascending; then for each of them
    in that order, while the list holds at most ``limit`` entries: the first of ``graph.best(k, best)`` not yet in, the first
    child not yet in (the k' with ``spanning_tree()[k'] == k``, ascending) and the parent if not yet in (frames of
    ``frame_removed`` are passed over).  Returns (the list int32, the reference keyframe: the most voted, the lowest on ties,
    -1 without votes)."""
    if not isinstance(graph, CovisibilityGraph):
        raise ValueError("local_keyframes takes a CovisibilityGraph")
    row = np.asarray(votes["votes"][query] if isinstance(votes, dict) else votes)
    if row.dtype.kind not in "iu" or row.shape != (graph.K,):
        raise ValueError(f"votes must be integers of shape [{graph.K}]")
    if limit < 0 or best < 0:
        raise ValueError("limit and best must not be negative")
    rem = _mask(frame_removed, graph.K, "frame_removed")
    gone = (lambda k: False) if rem is None else (lambda k: bool(rem[k]))
    out = [int(k) for k in np.flatnonzero(row > 0)]
    ref = int(row.argmax()) if out else -1
    inside = set(out)
    parent = graph.spanning_tree()
    order = np.argsort(parent, kind="stable")
    first = np.searchsorted(parent[order], np.arange(graph.K + 1))

    def add(ks) -> None:
        for k in ks:
            k = int(k)
            if k not in inside and not gone(k):
                inside.add(k)
                out.append(k)
                return

    for k in list(out):
        if len(out) > limit:
            break
        add(graph.best(k, best))
        add(order[first[k]:first[k + 1]])
        if parent[k] >= 0:
            add([parent[k]])
    return np.array(out, np.int32), ref


def local_points(tables: MapTables, local_keyframes, query_points, lkf_offsets=None, offsets=None) -> List[np.ndarray]:
    """``UpdateLocalPoints`` for B queries in two phases (mark and count, then fill): per query the map points, ascending and
    each once, of the rows of its ``local_keyframes`` - without bad points, without the rows of removed frames and without the
    points the query tracks already (``query_points``).  Both arguments as ``local_keyframe_votes`` takes its lists."""
    t = _tables(tables)
    lk, lo = _lists(local_keyframes, lkf_offsets, "local_keyframes")
    q, off = _lists(query_points, offsets, "query_points")
    if len(lo) != len(off):
        raise ValueError("one list of local keyframes per query")
    B = len(off) - 1
    if B == 0:
        return []
    W = (t.M + 31) // 32
    if B * W >= 1 << 31:
        raise ValueError("a bitmap of more than 2^31 - 1 words")
    t._live()
    ctx = t.ctx
    m = _Buffers(ctx)
    try:
        d_lk, d_q = m.up(lk), m.up(q)
        ws, bitmap = _new(ctx, m, workspace_bytes(B, t.F, t.M)["points"], "ws"), _new(ctx, m, 4 * B * W, "out")
        counts = np.zeros(B, np.int64)
        check(ctx.lib.slam_lmap_points_mark(ctx.handle, B, d_lk.ptr, addr(lo), d_q.ptr, addr(off), t.M, t.d_point_bad.ptr, t.F,
                                            t.d_frame_offsets.ptr, t.n_rows, t.d_frame_points.ptr, t.d_frame_removed.ptr, bitmap.ptr, ws.ptr,
                                            addr(counts)))
        out_off = np.zeros(B + 1, np.int64)
        out_off[1:] = np.cumsum(counts)
        total = int(out_off[-1])
        d_out = _new(ctx, m, 4 * total, "out")
        check(ctx.lib.slam_lmap_points_fill(ctx.handle, B, t.M, bitmap.ptr, ws.ptr, addr(out_off), d_out.ptr))
        flat = d_out.download(np.int32, (total,)) if total else np.zeros(0, np.int32)
        return [flat[out_off[b]:out_off[b + 1]].copy() for b in range(B)]
    finally:
        m.free()


def keyframe_redundancy(tables: MapTables, candidates=None, th_obs: int = 3, return_flags: bool = False):
    """``KeyFrameCulling``'s count for the frames ``candidates`` (None: all F) in up to three launches: counts int32 [C,2] =
    (n_points, n_redundant).  A row of candidate c with a point that is not bad counts as a point; it is redundant when the
    point has more than ``th_obs`` observers that are not removed and at least ``th_obs`` of them, c aside, see it at a level
    of at most the row's + 1.  A removed candidate gives (0, 0).  ``return_flags``: also u8 per candidate row, the candidates
    in order: 0 no point, 1 counted, 2 redundant."""
    t = _tables(tables)
    cand, th = _candidates(candidates, t.F), _th_obs(th_obs)
    C = t.F if cand is None else len(cand)
    rows = np.diff(t.frame_offsets)
    total = int(rows.sum() if cand is None else rows[cand].sum())
    if C == 0:
        return (np.zeros((0, 2), np.int32), np.zeros(0, np.uint8)) if return_flags else np.zeros((0, 2), np.int32)
    dev, ctx = t._live(), t.ctx
    m = _Buffers(ctx)
    try:
        ws, d_c = _new(ctx, m, workspace_bytes(0, t.F, t.M, C)["cull"], "ws"), _new(ctx, m, 8 * C, "out")
        d_f = _new(ctx, m, total, "out") if return_flags else None
        check(ctx.lib.slam_lmap_cull_count(ctx.handle, C, addr(cand) if cand is not None else None, t.M, t.obs.nnz, dev["offsets"].ptr,
                                           dev["obs"].ptr, t.d_point_bad.ptr, t.F, addr(t.frame_offsets), t.d_frame_offsets.ptr,
                                           t.d_frame_points.ptr, t.d_level.ptr, t.d_frame_removed.ptr, th, t.max_list, ws.ptr, d_c.ptr,
                                           d_f.ptr if d_f is not None else None))
        t.cull_launches += 1
        counts = d_c.download(np.int32, (C, 2))
        if not return_flags:
            return counts
        return counts, (d_f.download(np.uint8, (total,)) if total else np.zeros(0, np.uint8))
    finally:
        m.free()


def _ratio(ratio) -> Tuple[int, int]:
    a, b = ratio
    if isinstance(a, bool) or isinstance(b, bool) or int(a) != a or int(b) != b or a < 0 or b <= 0:
        raise ValueError("ratio must be a pair of integers (a, b), a >= 0 and b > 0: redundant when b n_redundant > a n_points")
    return int(a), int(b)


def redundant_verdict(counts, ratio=(9, 10)) -> np.ndarray:
    """bool [C]: ``ratio[1] * n_redundant > ratio[0] * n_points`` - ORB-SLAM's "more than 90 %" in integers."""
    a, b = _ratio(ratio)
    c = np.asarray(counts, np.int64).reshape(-1, 2)
    return b * c[:, 1] > a * c[:, 0]


def cull_keyframes(tables: MapTables, candidates, ratio=(9, 10), th_obs: int = 3, sequential: bool = True, protect=(0,)) -> np.ndarray:
    """``LocalMapping::KeyFrameCulling``: the candidates (None: all frames) whose redundant points outnumber ``ratio`` of
    their points are marked in ``tables.frame_removed`` on both sides and returned (int32, in candidate order).  Frames of
    ``protect`` (None: none) are never removed.  ``sequential``: the first redundant candidate in the given order is removed and the count
    runs again on the candidates after it - each keyframe judged against the map as the earlier removals left it; removals + 1
    launches of ``keyframe_redundancy`` (``tables.cull_launches`` counts them).  Without it every candidate gets the verdict
    of the map as it stands, in one."""
    t = _tables(tables)
    _ratio(ratio)
    cand = _candidates(candidates, t.F)
    cand = np.arange(t.F, dtype=np.int32) if cand is None else cand
    keep = np.zeros(t.F, bool)
    p = _candidates(list(protect) if protect is not None else [], t.F)
    keep[p] = True
    removed: List[int] = []
    while len(cand):
        verdict = redundant_verdict(keyframe_redundancy(t, cand, th_obs), ratio) & ~keep[cand] & (t.frame_removed[cand] == 0)
        hit = np.flatnonzero(verdict)
        if not sequential:
            for i in hit:
                if not t.frame_removed[cand[i]]:                # (a candidate may be listed twice)
                    t.remove_frame(int(cand[i]))
                    removed.append(int(cand[i]))
            break
        if not len(hit):
            break
        t.remove_frame(int(cand[hit[0]]))
        removed.append(int(cand[hit[0]]))
        cand = cand[hit[0] + 1:]
    return np.array(removed, np.int32)


# ---- host only ------------------------------------------------------------------------------------------------------------------------
def cull_map_points(found, visible, first_keyframe, n_obs, current_keyframe: int, th_obs: int = 2) -> np.ndarray:
    """``LocalMapping::MapPointCulling`` for the recently added points, numpy on the host (a few hundred elements do not pay
    for a launch).  u8 per point, the first that applies: 1 (bad) if ``4 found < visible`` - a found ratio below a quarter;
    2 (bad) if ``current_keyframe - first_keyframe >= 2`` and ``n_obs <= th_obs``; 3 (kept, leaves the recent list) if
    ``current_keyframe - first_keyframe >= 3``; else 0 (stays on the list)."""
    arrs = [np.asarray(a) for a in (found, visible, first_keyframe, n_obs)]
    arrs = [np.zeros(0, np.int64) if a.size == 0 else a for a in arrs]
    if any(a.dtype.kind not in "iu" or a.ndim != 1 or a.shape != arrs[0].shape for a in arrs):
        raise ValueError("found, visible, first_keyframe and n_obs must be integer arrays of one shape [n]")
    fd, vs, first, nob = (a.astype(np.int64) for a in arrs)
    age = int(current_keyframe) - first
    out = np.zeros(len(fd), np.uint8)
    out[age >= 3] = 3
    out[(age >= 2) & (nob <= int(th_obs))] = 2
    out[4 * fd < vs] = 1
    return out


def remove_frames(obs: MapObservations, removed) -> MapObservations:
    """A new ``MapObservations`` without the entries of the frames ``removed`` (a mask over the frames or a list of frame
    indices); host, beside ``apply_fusion``."""
    if not isinstance(obs, MapObservations):
        raise ValueError("remove_frames takes MapObservations")
    r = np.asarray(removed)
    if r.size == 0:
        r = np.zeros(0, np.int64)
    if r.dtype.kind == "b":
        r = np.flatnonzero(r)
    if r.dtype.kind not in "iu" or r.ndim != 1 or (len(r) and r.min() < 0):
        raise ValueError("removed must be a mask over the frames or a list of frame indices")
    keep = ~np.isin(obs.obs[:, 0], r)
    point = np.repeat(np.arange(len(obs)), obs.nobs)
    off = np.zeros(len(obs) + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(point[keep], minlength=len(obs)))
    return MapObservations.from_arrays(off, obs.obs[keep], obs.ctx)
