"""Two-view geometry on the GPU (``slam_tv_*``): what the reference's ``utils.py`` gets from cv2.

``pose_estimation_2d2d`` (``utils.py:10-28``) is ``cv2.findEssentialMat`` + ``cv2.recoverPose``; ``triangulation``
(``utils.py:32-55``) is ``cv2.triangulatePoints`` and a division.  Here the same three steps run for many frame pairs per
call, on arrays: points 1 are the reference's ``source_pts`` (last frame), points 2 its ``query_pts`` (current frame),
``x2^T E x1 = 0`` and ``X2 = R X1 + t`` with ``|t| = 1``.

PARITY UNPINNED: cv2 is absent here, so the calls are restated from the algorithms' definitions (five-point solver, Sampson
distance with OpenCV's threshold rule, cheirality vote with OpenCV's candidate order and distance limit, DLT).  OpenCV's own
random draws, its early termination and the sign its SVD gives ``t`` before the vote are not reproduced: a fixed number of
hypotheses from a documented counter-based generator is scored instead, so a result is a pure function of
(matches, intrinsics, hypotheses, threshold, seed).  There is no CPU fallback.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from ._args import _Buffers
from ._geometry import (MAX_HYPOTHESES, MAX_PAIRS, _cand_offsets, _check_cap, _check_ransac_args, _concat_flags, _flags,  # noqa: F401
                        _intrinsics, _mask_down, _pair, _pair_arrays, _points, _solve_samples, _split_mask, _Vote)
from ._lib import check
from .device import Context, default_context

DEFAULT_HYPOTHESES = 256        # the smallest power of two above ln(0.001) / ln(1 - 0.5**5) = 218: confidence 0.999 at 50 % inliers
DEFAULT_THRESHOLD = 1.0         # pixels, cv2.findEssentialMat's default
DEFAULT_DISTANCE = 50.0         # cv2.recoverPose's distanceThresh


def fivepoint_arrays(x1, x2, ctx: Optional[Context] = None):
    """All real essential matrices through five normalised correspondences per sample (``slam_tv_fivepoint_f64``):
    ``x1``, ``x2`` [S,5,2] (or [5,2]) -> (E [S,10,9] with Frobenius norm 1, unused slots zero; nroots int32 [S])."""
    x1, x2 = np.asarray(x1, np.float64), np.asarray(x2, np.float64)
    if x1.shape != x2.shape or x1.shape[-2:] != (5, 2) or x1.ndim not in (2, 3):
        raise ValueError(f"x1 and x2 must both have shape [S,5,2], got {x1.shape} and {x2.shape}")
    x1, x2 = np.ascontiguousarray(x1.reshape(-1, 5, 2)), np.ascontiguousarray(x2.reshape(-1, 5, 2))
    S = x1.shape[0]
    if S == 0:
        return np.zeros((0, 10, 9)), np.zeros(0, np.int32)
    return _solve_samples(ctx, "slam_tv_fivepoint_f64", x1, x2, (10, 9))


def find_essential_offsets(px1, px2, offsets, K, hypotheses: int = DEFAULT_HYPOTHESES, threshold: float = DEFAULT_THRESHOLD,
                           seed: int = 0, ctx: Optional[Context] = None):
    """``slam_tv_essential_ransac_f64`` on concatenated matches: pair b owns ``[offsets[b], offsets[b+1])``.
    Returns (E [B,9], inlier bool [M], stats int32 [B,4])."""
    fx, fy, cx, cy = _intrinsics(K)
    H, thr, seed = _check_ransac_args(hypotheses, threshold, seed)
    px1, px2 = _pair(px1, px2, "px1", "px2", 2)
    offsets, B = _cand_offsets(offsets, MAX_PAIRS, "pairs")
    if B == 0:
        return np.zeros((0, 9)), np.zeros(len(px1), bool), np.zeros((0, 4), np.int32)
    ctx = ctx or default_context()
    m = _Buffers(ctx)
    try:
        return _Vote(m, ctx.lib.slam_tv_essential_ransac_f64, (px1, px2), offsets, (fx, fy, cx, cy, H, thr, seed), 9).download()
    finally:
        m.free()


def find_essential_batch(pairs: Sequence, K, hypotheses: int = DEFAULT_HYPOTHESES, threshold: float = DEFAULT_THRESHOLD,
                         seed: int = 0, ctx: Optional[Context] = None):
    """``cv2.findEssentialMat`` for a list of ``(px1, px2)`` pairs in one call: (E [B,3,3], list of bool masks, stats [B,4])."""
    px1, px2, off = _pair_arrays(pairs)
    E, mask, st = find_essential_offsets(px1, px2, off, K, hypotheses, threshold, seed, ctx)
    return E.reshape(-1, 3, 3), _split_mask(mask, off), st


def find_essential_arrays(px1, px2, K, hypotheses: int = DEFAULT_HYPOTHESES, threshold: float = DEFAULT_THRESHOLD, seed: int = 0,
                          ctx: Optional[Context] = None):
    """``cv2.findEssentialMat(px1, px2, cameraMatrix=K)`` for one pair: (E [3,3], inlier mask bool [N]).  Fewer than five
    matches: a zero matrix and an empty vote, as the call defines it."""
    E, masks, _ = find_essential_batch([(px1, px2)], K, hypotheses, threshold, seed, ctx)
    return E[0], masks[0]


def recover_pose_offsets(E, px1, px2, offsets, K, inlier=None, distance_thresh: float = DEFAULT_DISTANCE,
                         ctx: Optional[Context] = None):
    """``slam_tv_recover_pose_f64``: (pose [B,3,4], good bool [M], stats int32 [B,2])."""
    fx, fy, cx, cy = _intrinsics(K)
    if not (np.isfinite(distance_thresh) and distance_thresh > 0):
        raise ValueError("distance_thresh must be positive")
    px1, px2 = _pair(px1, px2, "px1", "px2", 2)
    offsets = np.ascontiguousarray(offsets, np.int32).reshape(-1)
    B, M = len(offsets) - 1, len(px1)
    E = np.ascontiguousarray(E, np.float64)
    if E.size != 9 * max(B, 0):
        raise ValueError(f"E must hold one 3x3 matrix per pair ({B}), got shape {E.shape}")
    inlier = _flags(inlier, M)
    if B <= 0:
        return np.zeros((0, 3, 4)), np.zeros(M, bool), np.zeros((0, 2), np.int32)
    ctx = ctx or default_context()
    m = _Buffers(ctx)
    try:
        d1, d2, do, dE = m.up(px1), m.up(px2), m.up(offsets), m.up(E.reshape(-1))
        di = m.up(inlier) if inlier is not None else None
        dp, dm, ds = m.new(B * 96), m.new(M), m.new(B * 8)
        check(ctx.lib.slam_tv_recover_pose_f64(ctx.handle, B, do.ptr, d1.ptr, d2.ptr, M, fx, fy, cx, cy, dE.ptr,
                                               di.ptr if di is not None else None, float(distance_thresh), dp.ptr, dm.ptr, ds.ptr))
        pose, st = dp.download(np.float64, (B, 3, 4)), ds.download(np.int32, (B, 2))
        return pose, _mask_down(dm, M), st
    finally:
        m.free()


def recover_pose_batch(E, pairs: Sequence, K, inliers=None, distance_thresh: float = DEFAULT_DISTANCE, ctx: Optional[Context] = None):
    """``cv2.recoverPose`` for a list of pairs: (R [B,3,3], t [B,3], list of bool masks, stats [B,2])."""
    px1, px2, off = _pair_arrays(pairs)
    pose, good, st = recover_pose_offsets(E, px1, px2, off, K, _concat_flags(inliers, len(off) - 1), distance_thresh, ctx)
    return pose[:, :, :3].copy(), pose[:, :, 3].copy(), _split_mask(good, off), st


def recover_pose_arrays(E, px1, px2, K, inlier=None, distance_thresh: float = DEFAULT_DISTANCE, ctx: Optional[Context] = None):
    """``cv2.recoverPose(E, px1, px2, cameraMatrix=K)`` for one pair: (number of good points, R [3,3], t [3], mask bool [N])."""
    R, t, masks, st = recover_pose_batch(np.asarray(E, np.float64).reshape(1, 9), [(px1, px2)], K,
                                         None if inlier is None else [inlier], distance_thresh, ctx)
    return int(st[0, 0]), R[0], t[0], masks[0]


def triangulate_arrays(P1, P2, x1, x2, ctx: Optional[Context] = None):
    """``cv2.triangulatePoints(P1, P2, x1.T, x2.T)`` and the division of ``utils.py:52-53``: 3x4 projections, points [N,2]
    -> (X [N,3], w [N]) with w the homogeneous coordinate of the unit solution (near 0: a point at infinity)."""
    P1, P2 = np.asarray(P1, np.float64), np.asarray(P2, np.float64)
    if P1.size != 12 or P2.size != 12:
        raise ValueError("P1 and P2 must be 3x4 projection matrices")
    x1, x2 = _points(x1, "x1"), _points(x2, "x2")
    if len(x1) != len(x2):
        raise ValueError(f"{len(x1)} points in view 1 but {len(x2)} in view 2")
    N = len(x1)
    if N == 0:
        return np.zeros((0, 3)), np.zeros(0)
    ctx = ctx or default_context()
    m = _Buffers(ctx)
    try:
        dP1, dP2 = m.up(np.ascontiguousarray(P1.reshape(12))), m.up(np.ascontiguousarray(P2.reshape(12)))
        d1, d2 = m.up(x1), m.up(x2)
        dX, dw = m.new(N * 24), m.new(N * 8)
        check(ctx.lib.slam_tv_triangulate_f64(ctx.handle, N, dP1.ptr, dP2.ptr, d1.ptr, d2.ptr, dX.ptr, dw.ptr))
        return dX.download(np.float64, (N, 3)), dw.download(np.float64, (N,))
    finally:
        m.free()


def estimate_two_view(px1, px2, K, hypotheses: int = DEFAULT_HYPOTHESES, threshold: float = DEFAULT_THRESHOLD, seed: int = 0,
                      distance_thresh: float = DEFAULT_DISTANCE, ctx: Optional[Context] = None):
    """The whole of ``pose_estimation_2d2d`` (``utils.py:10-28``) on arrays: (R [3,3], t [3], inlier mask bool [N]) with
    ``X2 = R X1 + t``.  The mask is the essential matrix's RANSAC vote (``findEssentialMat``'s); like the reference
    (``utils.py:25``), ``recoverPose`` is given every match.  Fewer than five matches: identity, zero, empty vote."""
    R, t, masks, _ = verify_pairs([(px1, px2)], K, hypotheses, threshold, seed, distance_thresh, ctx)
    return R[0], t[0], masks[0]


def verify_pairs(pairs: Sequence, K, hypotheses: int = DEFAULT_HYPOTHESES, threshold: float = DEFAULT_THRESHOLD, seed: int = 0,
                 distance_thresh: float = DEFAULT_DISTANCE, ctx: Optional[Context] = None):
    """``estimate_two_view`` for a list of ``(px1, px2)`` candidates in two launches on one upload:
    (R [B,3,3], t [B,3], list of RANSAC inlier masks, inlier counts int [B])."""
    fx, fy, cx, cy = _intrinsics(K)
    H, thr, seed = _check_ransac_args(hypotheses, threshold, seed)
    if not (np.isfinite(distance_thresh) and distance_thresh > 0):
        raise ValueError("distance_thresh must be positive")
    px1, px2, off = _pair_arrays(pairs)
    B, M = len(off) - 1, len(px1)
    _check_cap(B, MAX_PAIRS, "pairs")
    if B == 0:
        return np.zeros((0, 3, 3)), np.zeros((0, 3)), [], np.zeros(0, np.int64)
    ctx = ctx or default_context()
    m = _Buffers(ctx)
    try:
        d1, d2, do = m.up(px1), m.up(px2), m.up(off)
        dE, dm, ds = m.new(B * 72), m.new(M), m.new(B * 16)
        dp, dg, dq = m.new(B * 96), m.new(M), m.new(B * 8)
        check(ctx.lib.slam_tv_essential_ransac_f64(ctx.handle, B, do.ptr, d1.ptr, d2.ptr, M, fx, fy, cx, cy, H, thr, seed,
                                                   dE.ptr, dm.ptr, ds.ptr))
        check(ctx.lib.slam_tv_recover_pose_f64(ctx.handle, B, do.ptr, d1.ptr, d2.ptr, M, fx, fy, cx, cy, dE.ptr, None,
                                               float(distance_thresh), dp.ptr, dg.ptr, dq.ptr))
        pose, st = dp.download(np.float64, (B, 3, 4)), ds.download(np.int32, (B, 4))
        mask = _mask_down(dm, M)
    finally:
        m.free()
    t = pose[:, :, 3].copy()
    t[st[:, 1] < 0] = 0.0
    return pose[:, :, :3].copy(), t, _split_mask(mask, off), st[:, 0].astype(np.int64)


def mean_reprojection_error(points, px, pose, K, ctx: Optional[Context] = None) -> float:
    """``Frontend._get_reprojection_error`` (``frontend.py:216-222``): the mean pixel distance between ``px`` [N,2] and the
    projection of ``points`` [N,3] under the 4x4 (or 3x4) ``pose``, from the residuals of ``slam_reproj_rj_f64``."""
    from .reproj import build_linearization

    fx, fy, cx, cy = _intrinsics(K)
    points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    px = _points(px, "px")
    if len(points) != len(px):
        raise ValueError("one pixel per point")
    if len(points) == 0:
        raise ValueError("no points")
    T = np.eye(4)
    T[:3, :4] = np.asarray(pose, np.float64).reshape(-1, 4)[:3, :4]
    n = len(points)
    e, _, _ = build_linearization(T[None], points, np.zeros(n, np.int32), np.arange(n, dtype=np.int32), px, fx, fy, cx, cy,
                                  False, ctx or default_context())
    return float(np.linalg.norm(e, axis=1).mean())
