"""Stereo matching on the GPU (``slam_stereo_match``): ORB-SLAM's ``Frame::ComputeStereoMatches`` on what the ORB
extractor left on the device - keypoints, descriptors and both pyramids - so nothing crosses PCIe between "two rectified frames
in" and "keypoints with ``u_right`` and depth out".  The reference opens one camera and has no counterpart.

The images must be rectified (``slamhip.camera``: ``OrbExtractor.upload_raw``) and of one shape.  Every row carries a status:
0 matched, 1 no candidate, 2 descriptor distance >= ``th_orb``, 3 window, 4 slide border, 5 disparity out of range, 6 rejected
by the median; ``u_right`` and ``depth`` are NaN unless it is 0.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import numpy as np

from ._args import _Buffers
from ._lib import addr, check
from .device import Context, default_context

MAX_PAIRS = 4096                    # SLAM_STEREO_MAX_PAIRS
MAX_ROWS = 8192                     # SLAM_STEREO_MAX_ROWS
MAX_LEVELS = 16                     # SLAM_STEREO_MAX_LEVELS
MAX_SIDE = 8192                     # SLAM_STEREO_MAX_SIDE
HALF_MAX = 15                       # SLAM_STEREO_HALF_MAX
TH_ORB = 75                         # ORB-SLAM's (TH_HIGH + TH_LOW) / 2
MATCHED, NO_CANDIDATE, ORB_DISTANCE, WINDOW, SLIDE_BORDER, DISPARITY, MEDIAN = range(7)
NO_DIST = 256
TH_DEPTH_FACTOR = 40.0              # ORB-SLAM's ThDepth: close points lie within 40 baselines


def scale_table(scale: float, n_levels: int) -> np.ndarray:
    """``h_scale`` f32 [L] exactly as ``OrbResult`` makes it."""
    return np.float32(scale) ** np.arange(n_levels, dtype=np.float32)


def _check_params(bf, fx, min_d, max_d, th_orb, w, Ls):
    if max_d is None:
        if fx is None:
            raise ValueError("give max_d, or fx (the default of max_d)")
        max_d = fx
    try:
        bf, min_d, max_d = float(bf), float(min_d), float(max_d)
    except (TypeError, ValueError) as exc:
        raise ValueError("bf, min_d and max_d must be numbers") from exc
    if not (np.isfinite(bf) and bf > 0):
        raise ValueError("bf must be positive and finite")
    if not np.isfinite(min_d):
        raise ValueError("min_d must be finite")
    if not max_d > min_d:
        raise ValueError("max_d must be above min_d")
    for name, v, lo, hi in (("th_orb", th_orb, 0, 256), ("w", w, 1, HALF_MAX), ("Ls", Ls, 1, HALF_MAX)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError(f"{name} must be an integer in [{lo}, {hi}]")
    return bf, min_d, max_d, int(th_orb), int(w), int(Ls)


def _check_pairs(pairs, B_left: int, B_right: int) -> np.ndarray:
    p = np.asarray(pairs)
    if p.size == 0:
        p = np.zeros((0, 2), np.int32)
    if p.dtype.kind not in "iu" or p.ndim != 2 or p.shape[1] != 2:
        raise ValueError(f"pairs must be integers of shape [P, 2], got {p.dtype} {p.shape}")
    if len(p) > MAX_PAIRS:
        raise ValueError(f"at most {MAX_PAIRS} pairs per call")
    if len(p) and (p.min() < 0 or p[:, 0].max() >= B_left or p[:, 1].max() >= B_right):
        raise ValueError(f"a pair is outside its blocks of {B_left} and {B_right} images")
    return np.ascontiguousarray(p, np.int32)


class StereoResult:
    """Per pair ``p`` (arrays trimmed to the count of the left image): ``right[p]`` int32 (the right row taken, -1: none),
    ``u_right[p]`` and ``depth[p]`` f64 (NaN unless ``status[p]`` is 0), ``orb_dist[p]`` int32 (256: no candidate), ``sad[p]``
    int32 (-1 for status 1, 2, 3), ``status[p]`` u8; ``counts`` int32 [P,2] = (rows of status 0, rows accepted before the
    median).  The left rows travel with it: ``xy[p]`` f32 [n,2] level-0 pixels, ``level[p]``, ``bin[p]``, ``descriptors[p]``."""

    def __init__(self, pairs, scale, bf, out: dict, counts, left_count, left_kp, left_desc):
        self.pairs, self.scale, self.bf, self.counts = pairs, np.asarray(scale, np.float32), float(bf), counts
        self.right, self.u_right, self.depth, self.orb_dist, self.sad, self.status = ([] for _ in range(6))
        self.xy, self.level, self.bin, self.descriptors = ([] for _ in range(4))
        for p, (a, _) in enumerate(pairs):
            n = int(left_count[a])
            for name in ("right", "u_right", "depth", "orb_dist", "sad", "status"):
                getattr(self, name).append(out[name][p, :n].copy())
            k = left_kp[a, :n]
            lv = np.clip(k[:, 2], 0, len(self.scale) - 1)
            self.xy.append(k[:, :2].astype(np.float32) * self.scale[lv][:, None])
            self.level.append(k[:, 2].copy())
            self.bin.append(k[:, 3].copy())
            self.descriptors.append(np.ascontiguousarray(left_desc[a, :n]))

    def __len__(self):
        return len(self.pairs)

    def points(self, b: int, K, pose=None, th_depth: Optional[float] = None):
        """(X f64 [n,3], close bool [n]) of pair ``b``: the camera-frame point ``((uL - cx) z / fx, (vL - cy) z / fy, z)`` with
        ``z = depth`` of every status-0 row, NaN elsewhere; with ``pose`` ([3,4] or [4,4] world -> camera) the world point
        ``R^T (X - t)``.  ``close = depth < th_depth`` (default: 40 baselines = 40 bf / fx, ORB-SLAM's ThDepth)."""
        fx, fy, cx, cy = (float(v) for v in K)
        z = self.depth[b]
        uv = self.xy[b].astype(np.float64)
        X = np.stack([(uv[:, 0] - cx) * z / fx, (uv[:, 1] - cy) * z / fy, z], 1) if len(z) else np.zeros((0, 3))
        if pose is not None:
            T = np.asarray(pose, np.float64).reshape(-1, 4)[:3]
            X = (X - T[:, 3]) @ T[:, :3]
        th = TH_DEPTH_FACTOR * self.bf / fx if th_depth is None else float(th_depth)
        with np.errstate(invalid="ignore"):
            close = z < th
        return X, close

    def point_set(self, b: int, K, pose=None, ctx: Optional[Context] = None):
        """(``PointSets`` of the status-0 rows of pair ``b``, their row indices int32): world (or camera-frame) positions, the
        left descriptors, levels and bins, the viewing normal from the camera centre and the scale-invariance range
        ``dmax = dist scale[l]``, ``dmin = dmax / scale[L - 1]`` of DESIGN.md 4m."""
        from .proj_match import PointSets

        X, _ = self.points(b, K, pose)
        rows = np.flatnonzero(self.status[b] == MATCHED).astype(np.int32)
        X = np.ascontiguousarray(X[rows])
        centre = np.zeros(3)
        if pose is not None:
            T = np.asarray(pose, np.float64).reshape(-1, 4)[:3]
            centre = -T[:, :3].T @ T[:, 3]
        ray = X - centre
        dist = np.sqrt((ray * ray).sum(1))
        s = self.scale.astype(np.float64)
        dmax = dist * s[self.level[b][rows]]
        dmin = dmax / s[-1]
        with np.errstate(invalid="ignore", divide="ignore"):
            normal = ray / dist[:, None]
        return PointSets(X, self.descriptors[b][rows], dmin2=dmin * dmin, dmax2=dmax * dmax, normal=normal, level=self.level[b][rows],
                         bins=self.bin[b][rows], ctx=ctx), rows


def stereo_match_device(ctx: Context, pairs: np.ndarray, left: dict, right: dict, n_max: int, layout: dict, scale: np.ndarray, bf, min_d, max_d,
                        th_orb, w, Ls, reject) -> dict:
    """``slam_stereo_match`` on resident blocks.  ``left`` / ``right``: dict(B, count, kp, desc, ws) of ``DeviceBuffer``s;
    ``layout``: dict(image_base, image_stride, image [L], pitch [L], w [L], h [L]).  Returns the outputs as host arrays
    [P, n_max] and ``counts`` [P, 2]."""
    P, L = len(pairs), len(scale)
    need = ctypes.c_uint64(0)
    check(ctx.lib.slam_stereo_workspace(P, n_max, ctypes.byref(need)))
    off = np.ascontiguousarray(layout["image"], np.uint64)
    pitch, lw, lh = (np.ascontiguousarray(layout[k], np.int32) for k in ("pitch", "w", "h"))
    sc = np.ascontiguousarray(scale, np.float32)
    slots = P * n_max
    m = _Buffers(ctx)
    try:
        ws = m.new(need.value)
        o = dict(right=m.new(4 * slots), u_right=m.new(8 * slots), depth=m.new(8 * slots), orb_dist=m.new(4 * slots), sad=m.new(4 * slots),
                 status=m.new(slots), counts=m.new(8 * P))
        check(ctx.lib.slam_stereo_match(ctx.handle, P, addr(pairs) if P else None, left["B"], left["count"].ptr, left["kp"].ptr, left["desc"].ptr,
                                        left["ws"].ptr, right["B"], right["count"].ptr, right["kp"].ptr, right["desc"].ptr, right["ws"].ptr, n_max,
                                        L, int(layout["image_base"]), int(layout["image_stride"]), addr(off), addr(pitch), addr(lw), addr(lh),
                                        addr(sc), bf, min_d, max_d, th_orb, w, Ls, int(bool(reject)), ws.ptr, need.value, o["right"].ptr,
                                        o["u_right"].ptr, o["depth"].ptr, o["orb_dist"].ptr, o["sad"].ptr, o["status"].ptr, o["counts"].ptr))
        if slots == 0:
            out = dict(right=np.zeros((P, n_max), np.int32), u_right=np.zeros((P, n_max)), depth=np.zeros((P, n_max)),
                       orb_dist=np.zeros((P, n_max), np.int32), sad=np.zeros((P, n_max), np.int32), status=np.zeros((P, n_max), np.uint8))
            out["counts"] = np.zeros((P, 2), np.int32)
            return out
        out = {k: o[k].download(t, (P, n_max)) for k, t in (("right", np.int32), ("u_right", np.float64), ("depth", np.float64),
                                                            ("orb_dist", np.int32), ("sad", np.int32), ("status", np.uint8))}
        out["counts"] = o["counts"].download(np.int32, (P, 2))
        return out
    finally:
        m.free()


def _extractor_block(ex) -> dict:
    if not ex.bufs or "desc" not in ex.bufs:
        raise ValueError("the extractor was freed, or its descriptors were released")
    return dict(B=ex.B, count=ex.bufs["count"], kp=ex.bufs["kp"], desc=ex.bufs["desc"], ws=ex.bufs["ws"])


def stereo_match(left, right=None, pairs=None, *, bf, fx=None, min_d: float = 0.0, max_d: Optional[float] = None, th_orb: int = TH_ORB, w: int = 5,
                 Ls: int = 5, reject: bool = True) -> StereoResult:
    """``Frame::ComputeStereoMatches`` on ``OrbExtractor``s after ``run()``.  Either one extractor and ``pairs`` int [P,2] =
    (left image, right image) inside it, or two extractors of one shape, paired image by image (``pairs`` may then select).
    ``bf`` = focal length x baseline; ``max_d`` defaults to ``fx``."""
    bf, min_d, max_d, th_orb, w, Ls = _check_params(bf, fx, min_d, max_d, th_orb, w, Ls)
    two = right is not None
    rx = right if two else left
    if two:
        a, b = left.P, right.P
        if left.ctx is not right.ctx:
            raise ValueError("the two extractors belong to different contexts")
        if (a.H, a.W, a.L, a.scale, a.n_max) != (b.H, b.W, b.L, b.scale, b.n_max) or left.B != right.B \
                or not np.array_equal(left.layout["pitch"], right.layout["pitch"]) or not np.array_equal(left.layout["image"], right.layout["image"]) \
                or (left.layout["image_base"], left.layout["image_stride"]) != (right.layout["image_base"], right.layout["image_stride"]):
            raise ValueError("pairs of extractors that differ in shape are not supported")
        if pairs is None:
            pairs = np.stack([np.arange(left.B), np.arange(left.B)], 1)
    elif pairs is None:
        raise ValueError("one extractor needs pairs")
    pairs = _check_pairs(pairs, left.B, rx.B)
    prm = left.P
    if prm.n_max > MAX_ROWS:
        raise ValueError(f"at most {MAX_ROWS} rows per image")
    scale = scale_table(prm.scale, prm.L)
    lay = dict(image_base=left.layout["image_base"], image_stride=left.layout["image_stride"], image=left.layout["image"],
               pitch=left.layout["pitch"], w=prm.lw, h=prm.lh)
    ctx = left.ctx
    out = stereo_match_device(ctx, pairs, _extractor_block(left), _extractor_block(rx), prm.n_max, lay, scale, bf, min_d, max_d, th_orb, w, Ls,
                              reject)
    count, kp, _, desc = left.download()
    return StereoResult(pairs, scale, bf, out, out["counts"], np.clip(count, 0, prm.n_max), kp, desc)


def _host_block(m: _Buffers, kps: Sequence, descs: Sequence, planes: Sequence, n_max: int, lay: dict):
    B = len(kps)
    count = np.asarray([len(k) for k in kps], np.int32)
    kp, desc = np.zeros((B, max(n_max, 1), 4), np.int32), np.zeros((B, max(n_max, 1), 32), np.uint8)
    img = np.zeros(max(B * lay["image_stride"], 16), np.uint8)
    for b in range(B):
        kp[b, :count[b]], desc[b, :count[b]] = kps[b], descs[b]
        for l, pl in enumerate(planes[b]):
            h, wl = pl.shape
            o = b * lay["image_stride"] + int(lay["image"][l])
            img[o:o + h * lay["pitch"][l]].reshape(h, lay["pitch"][l])[:, :wl] = pl
    return dict(B=B, count=m.up(count), kp=m.up(kp), desc=m.up(desc), ws=m.up(img)), count, kp, desc


def stereo_match_arrays(kp_left: Sequence, desc_left: Sequence, planes_left: Sequence, kp_right: Sequence, desc_right: Sequence,
                        planes_right: Sequence, scale, pairs=None, *, bf, fx=None, min_d: float = 0.0, max_d: Optional[float] = None,
                        th_orb: int = TH_ORB, w: int = 5, Ls: int = 5, reject: bool = True, ctx: Optional[Context] = None) -> StereoResult:
    """The same on host arrays: per image ``kp`` int [n,4] = (x, y, level, bin) in level coordinates, ``desc`` u8 [n,32] and
    ``planes`` = the L pyramid levels u8 [h_l, w_l] (one shape for every image of both sides); ``scale`` the f32 [L] table
    (``scale_table``).  They are uploaded into the extractor's layout.  ``pairs`` defaults to image b with image b."""
    bf, min_d, max_d, th_orb, w, Ls = _check_params(bf, fx, min_d, max_d, th_orb, w, Ls)
    sc = np.ascontiguousarray(scale, np.float32).reshape(-1)
    L = len(sc)
    if not 1 <= L <= MAX_LEVELS or not ((sc >= 1) & (sc <= 65536)).all():
        raise ValueError(f"scale must hold 1 to {MAX_LEVELS} values in [1, 65536]")
    sides = (list(kp_left), list(desc_left), list(planes_left)), (list(kp_right), list(desc_right), list(planes_right))
    shapes = None
    blocks: List[tuple] = []
    for kps, descs, planes in sides:
        if not len(kps) == len(descs) == len(planes):
            raise ValueError("kp, desc and planes must list the same images")
        kk, dd, pp = [], [], []
        for k, d, pl in zip(kps, descs, planes):
            k, d = np.asarray(k), np.asarray(d)
            k = k.reshape(-1, 4) if k.size == 0 else k
            d = d.reshape(-1, 32) if d.size == 0 else d
            if k.dtype.kind not in "iu" or k.ndim != 2 or k.shape[1] != 4:
                raise ValueError("kp must be integers of shape [n, 4]")
            if d.dtype != np.uint8 or d.shape != (len(k), 32):
                raise ValueError("desc must be uint8 of shape [n, 32]")
            pl = [np.asarray(q) for q in pl]
            if len(pl) != L or any(q.dtype != np.uint8 or q.ndim != 2 or q.size == 0 or max(q.shape) > MAX_SIDE for q in pl):
                raise ValueError(f"planes must be {L} non-empty uint8 images per image")
            if shapes is None:
                shapes = [q.shape for q in pl]
            if [q.shape for q in pl] != shapes:
                raise ValueError("every image of both sides must have one pyramid shape")
            if len(k) and ((k[:, 2] < 0) | (k[:, 2] >= L)).any():
                raise ValueError("a keypoint level is outside the pyramid")
            lv = k[:, 2].astype(np.int64)
            hw = np.asarray(shapes)[lv] if len(k) else np.zeros((0, 2), np.int64)
            if len(k) and ((k[:, 0] < 0) | (k[:, 0] >= hw[:, 1]) | (k[:, 1] < 0) | (k[:, 1] >= hw[:, 0])).any():
                raise ValueError("a keypoint lies outside its level")
            kk.append(k.astype(np.int32)), dd.append(d), pp.append(pl)
        blocks.append((kk, dd, pp))
    BL, BR = len(blocks[0][0]), len(blocks[1][0])
    if pairs is None:
        if BL != BR:
            raise ValueError("without pairs the two sides must list the same number of images")
        pairs = np.stack([np.arange(BL), np.arange(BL)], 1)
    pairs = _check_pairs(pairs, BL, BR)
    n_max = max([len(k) for k in blocks[0][0] + blocks[1][0]] + [0])
    if n_max > MAX_ROWS:
        raise ValueError(f"at most {MAX_ROWS} rows per image")
    out_empty = len(pairs) == 0 or n_max == 0 or shapes is None
    pitch = np.asarray([(s[1] + 3) // 4 * 4 for s in (shapes or [])], np.int32)
    offs, at = [], 0
    for s, pt in zip(shapes or [], pitch):
        offs.append(at)
        at += (int(pt) * s[0] + 15) // 16 * 16
    lay = dict(image_base=0, image_stride=at, image=np.asarray(offs, np.uint64), pitch=pitch, w=np.asarray([s[1] for s in (shapes or [])], np.int32),
               h=np.asarray([s[0] for s in (shapes or [])], np.int32))
    if out_empty:
        z = {k: np.zeros((len(pairs), n_max), t) for k, t in (("right", np.int32), ("u_right", np.float64), ("depth", np.float64),
                                                              ("orb_dist", np.int32), ("sad", np.int32), ("status", np.uint8))}
        return StereoResult(pairs, sc, bf, z, np.zeros((len(pairs), 2), np.int32), np.zeros(BL, np.int32), np.zeros((BL, 0, 4), np.int32),
                            np.zeros((BL, 0, 32), np.uint8))
    ctx = ctx or default_context()
    m = _Buffers(ctx)
    try:
        left, count, kp, desc = _host_block(m, *blocks[0], n_max, lay)
        right = _host_block(m, *blocks[1], n_max, lay)[0]
        out = stereo_match_device(ctx, pairs, left, right, n_max, lay, sc, bf, min_d, max_d, th_orb, w, Ls, reject)
        return StereoResult(pairs, sc, bf, out, out["counts"], count, kp, desc)
    finally:
        m.free()
