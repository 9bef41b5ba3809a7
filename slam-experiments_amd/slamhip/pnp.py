"""Absolute pose from 2D-3D correspondences on the GPU (``slam_pnp_*``): ``cv2.solvePnPRansac`` with ``SOLVEPNP_P3P`` for
many candidates per call.

The reference has no call site: the nearest is ``Frontend._reinitialize_from_keyframe`` (``frontend.py:223-229``), which drops
the map because it has no such estimate.  A keyframe's map points matched against another frame's keypoints are 3D-2D
correspondences; a pose from those is in map scale with all six degrees of freedom, which a two-view estimate (unit
translation, arbitrary under pure rotation) is not.  ``X_cam = R X + t``.

PARITY UNPINNED: cv2 is absent here, so the call is restated from the algorithm's definition (P3P minimal solver, reprojection
error in pixels against OpenCV's ``reprojectionError``).  OpenCV's own random draws, its early termination and its final
refit are not reproduced: a fixed number of hypotheses from a documented counter-based generator is scored instead, so a
result is a pure function of (correspondences, intrinsics, hypotheses, threshold, seed).  There is no CPU fallback.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from ._args import _Buffers
from ._geometry import (MAX_PAIRS, _cand_offsets, _check_cap, _check_edge_args, _check_ransac_args, _concat, _edge_info, _edge_pairs,
                        _intrinsics, _points, _solve_samples, _split_mask, _Vote)
from ._lib import check
from .device import Context, default_context
from .pose_opt import CHI2_THRESHOLD, HUBER_DELTA

DEFAULT_HYPOTHESES = 256        # as the essential-matrix RANSAC; ln(0.001) / ln(1 - 0.5**3) = 52 would do at 50 % inliers
DEFAULT_THRESHOLD = 8.0         # pixels, cv2.solvePnPRansac's reprojectionError default
REFINE_ROUNDS, REFINE_ITERATIONS = 4, 10        # Frontend._correct_current_pose (frontend.py:298-393)


def _ransac(m: _Buffers, X, px, off, K, hypotheses, threshold, seed) -> _Vote:
    """``slam_pnp_ransac_f64`` on checked arrays, under the caller's buffers (the refinement starts from the poses on the device)."""
    fx, fy, cx, cy = K
    return _Vote(m, m.ctx.lib.slam_pnp_ransac_f64, (X, px), off, (fx, fy, cx, cy, hypotheses, threshold, seed), 12)


def p3p_arrays(X, x, ctx: Optional[Context] = None):
    """Every pose that sees three world points along three normalised image points, per sample (``slam_pnp_p3p_f64``):
    ``X`` [S,3,3] (or [3,3]), ``x`` [S,3,2] (or [3,2]) -> (pose [S,4,3,4], unused slots zero; nsol int32 [S])."""
    X, x = np.asarray(X, np.float64), np.asarray(x, np.float64)
    if X.shape[-2:] != (3, 3) or x.shape[-2:] != (3, 2) or X.ndim not in (2, 3) or x.ndim != X.ndim or X.shape[:-2] != x.shape[:-2]:
        raise ValueError(f"X must have shape [S,3,3] and x [S,3,2], got {X.shape} and {x.shape}")
    X, x = np.ascontiguousarray(X.reshape(-1, 3, 3)), np.ascontiguousarray(x.reshape(-1, 3, 2))
    S = X.shape[0]
    if S == 0:
        return np.zeros((0, 4, 3, 4)), np.zeros(0, np.int32)
    return _solve_samples(ctx, "slam_pnp_p3p_f64", X, x, (4, 3, 4))


def solve_pnp_ransac_offsets(points, px, offsets, K, hypotheses: int = DEFAULT_HYPOTHESES, threshold: float = DEFAULT_THRESHOLD,
                             seed: int = 0, ctx: Optional[Context] = None):
    """``slam_pnp_ransac_f64`` on concatenated correspondences: candidate b owns ``[offsets[b], offsets[b+1])``.
    Returns (pose [B,3,4], inlier bool [M], stats int32 [B,4])."""
    K = _intrinsics(K)
    H, thr, seed = _check_ransac_args(hypotheses, threshold, seed)
    points, px = _points(points, "points", 3), _points(px, "px")
    if len(points) != len(px):
        raise ValueError(f"{len(points)} points but {len(px)} pixels")
    offsets, B = _cand_offsets(offsets, MAX_PAIRS, "candidates")
    if B == 0:
        return np.zeros((0, 3, 4)), np.zeros(len(points), bool), np.zeros((0, 4), np.int32)
    m = _Buffers(ctx or default_context())
    try:
        return _ransac(m, points, px, offsets, K, H, thr, seed).download(3, 4)
    finally:
        m.free()


def solve_pnp_ransac_batch(cands: Sequence, K, hypotheses: int = DEFAULT_HYPOTHESES, threshold: float = DEFAULT_THRESHOLD,
                           seed: int = 0, refine: bool = True, ctx: Optional[Context] = None):
    """``cv2.solvePnPRansac(points, px, K, None, flags=cv2.SOLVEPNP_P3P)`` for a list of ``(points [N_b,3], px [N_b,2])``
    candidates in one call: (poses [B,3,4], list of bool masks, inlier counts int [B], stats int32 [B,4], refined counts).

    The masks and the inlier counts are the RANSAC vote.  With ``refine`` the RANSAC inliers of every candidate that has a
    model go, from the RANSAC pose, through ``slam_pose_optimize_batch_f64`` in one launch (4 rounds x 10 LM iterations,
    chi2 gate 5.991^2, as ``Frontend._correct_current_pose``); the returned poses are then the refined ones and the fifth
    value holds the refinement's inlier counts int [B] (None without ``refine``).  A candidate of fewer than 3
    correspondences, or one where no hypothesis gave a model, comes back with the identity, an empty vote, stats
    {0, -1, -1, 0} and is not refined."""
    fx, fy, cx, cy = _intrinsics(K)
    H, thr, seed = _check_ransac_args(hypotheses, threshold, seed)
    X, px, off = _concat(cands, "candidate", (("points", 3), ("px", 2)), "correspondences", "{} points but {} pixels")
    B = len(off) - 1
    _check_cap(B, MAX_PAIRS, "candidates")
    if B == 0:
        return np.zeros((0, 3, 4)), [], np.zeros(0, np.int64), np.zeros((0, 4), np.int32), (np.zeros(0, np.int64) if refine else None)
    ctx = ctx or default_context()
    m = _Buffers(ctx)
    try:
        vote = _ransac(m, X, px, off, (fx, fy, cx, cy), H, thr, seed)
        pose, mask, st = vote.download(3, 4)
        refined = None
        if refine:
            # the optimiser takes whole slices: the inliers are packed on the host (the vote has to come down anyway) and
            # the refinement starts from the RANSAC poses still on the device
            keep = np.flatnonzero(mask)
            off2 = np.searchsorted(keep, off).astype(np.int32)
            O = len(keep)
            refined = np.zeros(B, np.int64)
            if O:
                dX2, dp2, do2 = m.up(np.ascontiguousarray(X[keep])), m.up(np.ascontiguousarray(px[keep])), m.up(off2)
                dT2, di2, dc2, ds2 = m.new(B * 96), m.new(O), m.new(O * 8), m.new(B * 8)
                check(ctx.lib.slam_pose_optimize_batch_f64(ctx.handle, B, vote.model.ptr, dX2.ptr, dp2.ptr, do2.ptr, O, fx, fy, cx, cy,
                                                           REFINE_ROUNDS, REFINE_ITERATIONS, CHI2_THRESHOLD, HUBER_DELTA,
                                                           dT2.ptr, di2.ptr, dc2.ptr, ds2.ptr))
                out, rs = dT2.download(np.float64, (B, 3, 4)), ds2.download(np.int32, (B, 2))
                has = (st[:, 1] >= 0) & (np.diff(off2) > 0) & np.isfinite(out).all((1, 2))
                pose[has] = out[has]
                refined[has] = rs[has, 0]
    finally:
        m.free()
    return pose, _split_mask(mask, off), st[:, 0].astype(np.int64), st, refined


def solve_pnp_ransac(points, px, K, hypotheses: int = DEFAULT_HYPOTHESES, threshold: float = DEFAULT_THRESHOLD, seed: int = 0,
                     refine: bool = True, ctx: Optional[Context] = None):
    """One candidate: (ok, pose [3,4], inlier mask bool [N]); ``ok`` is False (identity, empty vote) when there are fewer than
    3 correspondences or no hypothesis gave a model."""
    pose, masks, _, st, _ = solve_pnp_ransac_batch([(points, px)], K, hypotheses, threshold, seed, refine, ctx)
    return bool(st[0, 1] >= 0), pose[0], masks[0]


def _pose44(a, name):
    a = np.asarray(a, np.float64)
    if a.ndim == 2 and a.shape[1] == 12:
        a = a.reshape(-1, 3, 4)
    if a.ndim != 3 or a.shape[1:] not in ((3, 4), (4, 4)):
        raise ValueError(f"{name} must have shape [N,3,4], [N,4,4] or [N,12], got {a.shape}")
    T = np.tile(np.eye(4), (len(a), 1, 1))
    T[:, :3, :] = a[:, :3, :]
    return T


def loop_edges_from_pnp(pairs, poses, inlier_counts, map_poses, min_inliers: int = 20, rotation_sigma: float = 0.01,
                        translation_sigma: float = 0.1):
    """Edges from ``solve_pnp_ransac_batch`` output, in the format of ``loop_edges_from_two_view``: ``pairs`` int [B,2] with
    ``pairs[b] = (i, j)``, ``poses[b]`` the estimated world -> camera j pose (from keyframe i's map points matched in frame
    j), ``map_poses[i]`` the world -> camera i pose the map holds -> (edges int32 [E,2], meas [E,3,4], info [E,6,6]) for the
    pairs with at least ``min_inliers`` inliers and i != j.

    The measurement is the relative pose ``T_j T_i^-1`` (``X_j = R X_i + t``), what ``optimize_pose_graph`` expects.  The
    pose is in map scale, so BOTH blocks of the information are set: ``inliers / min_inliers / sigma^2`` times the
    identity, with the rotation and the translation sigma."""
    pairs = _edge_pairs(pairs)
    B = len(pairs)
    T = _pose44(poses, "poses") if B else np.zeros((0, 4, 4))
    Tm = _pose44(map_poses, "map_poses")
    n = np.asarray(inlier_counts).reshape(-1)
    if not (len(T) == len(n) == B):
        raise ValueError(f"{B} pairs but {len(T)} poses and {len(n)} inlier counts")
    _check_edge_args(min_inliers, rotation_sigma, translation_sigma)
    if B and (pairs.min() < 0 or pairs.max() >= len(Tm)):
        raise ValueError(f"pair index outside the {len(Tm)} map poses")
    k = np.flatnonzero((n >= min_inliers) & (pairs[:, 0] != pairs[:, 1]))
    meas = np.zeros((len(k), 3, 4))
    for e, b in enumerate(k):
        Ti = Tm[pairs[b, 0]]
        inv = np.eye(4)
        inv[:3, :3] = Ti[:3, :3].T
        inv[:3, 3] = -Ti[:3, :3].T @ Ti[:3, 3]
        meas[e] = (T[b] @ inv)[:3]
    return np.ascontiguousarray(pairs[k], np.int32), meas, _edge_info(n[k] / float(min_inliers), rotation_sigma, translation_sigma)
