"""Sim(3) alignment of two copies of the same map points on the GPU (``slam_sim3_*``): ORB-SLAM's ``Sim3Solver`` (Horn's
three-point closed form under RANSAC) for many loop candidates per call, and a least-squares refit on the inliers.

The reference has no call site: it closes no loops, and its driver prints the estimated translation beside the ground truth
with no alignment at all (``euroc.py:63-66``), which for a monocular run compares nothing - gauge and scale are free.  A
monocular map drifts in scale, so the constraint between two keyframes that each hold their own copy of the same map points
is a similarity ``X2 = s R X1 + t``; the same closed form aligns an estimated trajectory to its ground truth (ATE).

PARITY UNPINNED: ORB-SLAM and cv2 are absent here, so the calls are restated from the algorithm's definition (Horn 1987,
Umeyama 1991; ORB-SLAM's two-sided reprojection test).  ``Sim3Solver``'s own random draws, its early termination and its
per-octave sigma table are not reproduced: a fixed number of hypotheses from a documented counter-based generator is scored,
and ``sigma2`` is where a caller puts the squared keypoint sigmas.  There is no CPU fallback.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from ._args import _Buffers
from ._geometry import (MAX_PAIRS, _cand_offsets, _check_ransac_args, _concat, _edge_info, _edge_pairs, _intrinsics, _model_srt,
                        _pair, _rows, _solve_samples, _split_mask, _Vote)
from ._lib import check
from .device import Context, default_context

DEFAULT_HYPOTHESES = 256        # as the other RANSAC calls; ORB-SLAM's Sim3Solver: at most 300 iterations
DEFAULT_CHI2_GATE = 9.210       # chi-square of 2 degrees of freedom at 99 %, ORB-SLAM's Sim3Solver
DEFAULT_MAX_LOG_SCALE = 0.05    # |log s| an SE(3) edge may hide: 5 % of scale, about the noise of a 20-inlier scale estimate


def _points_pair(X1, X2):
    """The two point sets of a call, f64 [M,3] each."""
    return _pair(X1, X2, "X1", "X2", 3, "correspondences")


def sim3_threepoint_arrays(X1, X2, fix_scale: bool = False, ctx: Optional[Context] = None):
    """The similarity through three correspondences per sample (``slam_sim3_threepoint_f64``): ``X1``, ``X2`` [S,3,3] (or
    [3,3]) -> (s [S], R [S,3,3], t [S,3], ok int32 [S]); a sample without a model has the identity, s = 1 and ok = 0."""
    X1, X2 = np.asarray(X1, np.float64), np.asarray(X2, np.float64)
    if X1.shape != X2.shape or X1.shape[-2:] != (3, 3) or X1.ndim not in (2, 3):
        raise ValueError(f"X1 and X2 must both have shape [S,3,3], got {X1.shape} and {X2.shape}")
    X1, X2 = np.ascontiguousarray(X1.reshape(-1, 3, 3)), np.ascontiguousarray(X2.reshape(-1, 3, 3))
    S = X1.shape[0]
    if S == 0:
        return np.zeros(0), np.zeros((0, 3, 3)), np.zeros((0, 3)), np.zeros(0, np.int32)
    model, ok = _solve_samples(ctx, "slam_sim3_threepoint_f64", X1, X2, (13,), int(bool(fix_scale)))
    return _model_srt(model) + (ok,)


def estimate_sim3_offsets(X1, X2, offsets, K, hypotheses: int = DEFAULT_HYPOTHESES, chi2_gate: float = DEFAULT_CHI2_GATE,
                          sigma2=None, fix_scale: bool = False, seed: int = 0, refit: bool = True, ctx: Optional[Context] = None):
    """``slam_sim3_ransac_f64`` on concatenated correspondences: candidate b owns ``[offsets[b], offsets[b+1])`` of ``X1`` /
    ``X2`` [M,3]; ``sigma2`` [M,2] are the squared keypoint sigmas in image 1 and image 2 (None: all 1).
    Returns (s [B], R [B,3,3], t [B,3], inlier bool [M], stats int32 [B,4], refit stats int32 [B,2] or None).

    The mask and ``stats = {inlier count, winning hypothesis, 0, models scored}`` are the RANSAC vote.  With ``refit`` the
    RANSAC inliers of every candidate go through ``slam_sim3_refit_f64`` while everything is still on the device (one
    upload, the mask never leaves it); a candidate whose refit is ok (``refit stats = {points used, ok}``) returns the
    least-squares model, any other the RANSAC one.  A candidate of fewer than 3 correspondences, or one where no hypothesis
    gave a model, comes back with the identity, s = 1, an empty vote and stats {0, -1, -1, 0}."""
    fx, fy, cx, cy = _intrinsics(K)
    H, gate, seed = _check_ransac_args(hypotheses, chi2_gate, seed)
    X1, X2 = _points_pair(X1, X2)
    M = len(X1)
    sg = None if sigma2 is None else _rows(sigma2, M, "sigma2")
    offsets, B = _cand_offsets(offsets, MAX_PAIRS, "candidates")
    if B == 0:
        return (np.zeros(0), np.zeros((0, 3, 3)), np.zeros((0, 3)), np.zeros(M, bool), np.zeros((0, 4), np.int32),
                np.zeros((0, 2), np.int32) if refit else None)
    ctx = ctx or default_context()
    m = _Buffers(ctx)
    try:
        fix = int(bool(fix_scale))
        vote = _Vote(m, ctx.lib.slam_sim3_ransac_f64, (X1, X2), offsets, (fx, fy, cx, cy, H, gate, fix, seed), 13, tail=(sg,))
        rs = None
        if refit:                                       # on the mask still on the device
            dT2, ds2 = m.new(B * 104), m.new(B * 8)
            check(ctx.lib.slam_sim3_refit_f64(ctx.handle, B, vote.offsets.ptr, vote.arrays[0].ptr, vote.arrays[1].ptr, M, vote.mask.ptr, fix,
                                              dT2.ptr, ds2.ptr))
        model, mask, st = vote.download()
        if refit:
            fit, rs = dT2.download(np.float64, (B, 13)), ds2.download(np.int32, (B, 2))
            use = (st[:, 1] >= 0) & (rs[:, 1] != 0)
            model[use] = fit[use]
    finally:
        m.free()
    return _model_srt(model) + (mask, st, rs)


def estimate_sim3_batch(cands: Sequence, K, hypotheses: int = DEFAULT_HYPOTHESES, chi2_gate: float = DEFAULT_CHI2_GATE,
                        fix_scale: bool = False, seed: int = 0, refit: bool = True, ctx: Optional[Context] = None):
    """ORB-SLAM's ``Sim3Solver`` for a list of ``(X1 [N_b,3], X2 [N_b,3])`` or ``(X1, X2, sigma2 [N_b,2])`` candidates in
    one call: (s [B], R [B,3,3], t [B,3], list of bool masks, stats int32 [B,4], refit stats or None), as
    ``estimate_sim3_offsets``."""
    X1, X2, sg, off = _concat(cands, "candidate", (("X1", 3), ("X2", 3)), "correspondences", sigma2=True)
    s, R, t, mask, st, rs = estimate_sim3_offsets(X1, X2, off, K, hypotheses, chi2_gate, sg, fix_scale, seed, refit, ctx)
    return s, R, t, _split_mask(mask, off), st, rs


def estimate_sim3(X1, X2, K, hypotheses: int = DEFAULT_HYPOTHESES, chi2_gate: float = DEFAULT_CHI2_GATE, sigma2=None,
                  fix_scale: bool = False, seed: int = 0, refit: bool = True, ctx: Optional[Context] = None):
    """One candidate: (ok, s, R [3,3], t [3], inlier mask bool [N]); ``ok`` is False (identity, s = 1, empty vote) when
    there are fewer than 3 correspondences or no hypothesis gave a model."""
    X1, X2 = _points_pair(X1, X2)
    s, R, t, mask, st, _ = estimate_sim3_offsets(X1, X2, [0, len(X1)], K, hypotheses, chi2_gate, sigma2, fix_scale, seed, refit, ctx)
    return bool(st[0, 1] >= 0), float(s[0]), R[0], t[0], mask


def fit_sim3_offsets(X1, X2, offsets, mask=None, fix_scale: bool = False, ctx: Optional[Context] = None):
    """``slam_sim3_refit_f64``: the least-squares similarity of every candidate's selected correspondences ->
    (s [B], R [B,3,3], t [B,3], stats int32 [B,2] = {points used, ok})."""
    X1, X2 = _points_pair(X1, X2)
    M = len(X1)
    offsets, B = _cand_offsets(offsets, 1 << 24, "candidates")
    if mask is not None:
        mask = np.asarray(mask)
        if mask.shape != (M,):
            raise ValueError(f"mask must have shape [{M}], got {mask.shape}")
        mask = np.ascontiguousarray(mask.astype(bool), np.uint8)
    if B == 0:
        return np.zeros(0), np.zeros((0, 3, 3)), np.zeros((0, 3)), np.zeros((0, 2), np.int32)
    ctx = ctx or default_context()
    m = _Buffers(ctx)
    try:
        d1, d2, do = m.up(X1), m.up(X2), m.up(offsets)
        dk = m.up(mask) if mask is not None else None
        dT, ds = m.new(B * 104), m.new(B * 8)
        check(ctx.lib.slam_sim3_refit_f64(ctx.handle, B, do.ptr, d1.ptr, d2.ptr, M, dk.ptr if dk is not None else None, int(bool(fix_scale)),
                                          dT.ptr, ds.ptr))
        return _model_srt(dT.download(np.float64, (B, 13))) + (ds.download(np.int32, (B, 2)),)
    finally:
        m.free()


def fit_sim3(X1, X2, mask=None, fix_scale: bool = False, ctx: Optional[Context] = None):
    """The least-squares similarity ``X2 ~ s R X1 + t`` of two point sets [N,3] (the rows with ``mask``; None: all):
    (ok, s, R [3,3], t [3]).  ``ok`` is False (identity, s = 1) with fewer than 3 selected points, collinear or repeated
    points, or non-finite data."""
    X1, X2 = _points_pair(X1, X2)
    s, R, t, st = fit_sim3_offsets(X1, X2, [0, len(X1)], mask, fix_scale, ctx)
    return bool(st[0, 1]), float(s[0]), R[0], t[0]


def align_trajectory(estimated_xyz, ground_truth_xyz, fix_scale: bool = False, ctx: Optional[Context] = None):
    """Absolute trajectory error after the least-squares Sim(3) alignment (SE(3) with ``fix_scale``) of the estimated
    positions [N,3] to the ground truth [N,3]: (s, R, t, aligned [N,3] = s R x + t, ate_rmse).  What ``euroc.py:63-66``
    should have done before comparing: a monocular estimate has a free gauge and a free scale.  A trajectory without a fit
    (fewer than 3 poses, all on one line) raises ``ValueError``."""
    est, gt = _points_pair(estimated_xyz, ground_truth_xyz)
    ok, s, R, t = fit_sim3(est, gt, None, fix_scale, ctx)
    if not ok:
        raise ValueError("the trajectories have no unique alignment (fewer than 3 poses, collinear positions or non-finite data)")
    aligned = s * (est @ R.T) + t
    return s, R, t, aligned, float(np.sqrt(((aligned - gt) ** 2).sum(1).mean()))


def loop_edges_from_sim3(pairs, models, inlier_counts, min_inliers: int = 20, max_log_scale: float = DEFAULT_MAX_LOG_SCALE,
                         rotation_sigma: float = 0.01, translation_sigma: float = 0.1):
    """Edges from ``estimate_sim3_batch`` output, in the format of ``loop_edges_from_pnp``: ``pairs`` int [B,2] with
    ``pairs[b] = (i, j)``, ``models = (s [B], R [B,3,3], t [B,3])`` with ``X_j = s R X_i + t`` ->
    (edges int32 [E,2], meas [E,3,4], info [E,6,6], scales [B]).

    An edge is emitted for the pairs with at least ``min_inliers`` inliers, i != j and ``|log s| <= max_log_scale``: its
    measurement is the SE(3) part in FRAME-1 SCALE, ``[R | t / s]`` (``X_j / s = R X_i + t / s``), what
    ``optimize_pose_graph`` expects, with BOTH information blocks set (``inliers / min_inliers / sigma^2`` times the
    identity).  ``scales`` holds s for ALL candidates: an SE(3) graph cannot absorb scale drift, so a candidate beyond
    ``max_log_scale`` is reported there and gets no edge.  Edges with real scale drift go to the Sim(3) pose graph:
    ``slamhip.sim3_graph.sim3_edges_from_sim3`` and ``optimize_sim3_graph``."""
    pairs = _edge_pairs(pairs)
    B = len(pairs)
    if len(models) != 3:
        raise ValueError("models must be (s [B], R [B,3,3], t [B,3])")
    s = np.asarray(models[0], np.float64).reshape(-1)
    R = np.asarray(models[1], np.float64).reshape(-1, 3, 3)
    t = np.asarray(models[2], np.float64).reshape(-1, 3)
    n = np.asarray(inlier_counts).reshape(-1)
    if not (len(s) == len(R) == len(t) == len(n) == B):
        raise ValueError(f"{B} pairs but {len(s)} scales, {len(R)} rotations, {len(t)} translations and {len(n)} inlier counts")
    if min_inliers < 1 or rotation_sigma <= 0 or translation_sigma <= 0 or not max_log_scale >= 0:
        raise ValueError("min_inliers >= 1, positive sigmas and max_log_scale >= 0")
    if B and pairs.min() < 0:
        raise ValueError("negative pair index")
    with np.errstate(all="ignore"):
        drift = np.abs(np.log(s))
    k = np.flatnonzero((n >= min_inliers) & (pairs[:, 0] != pairs[:, 1]) & (s > 0) & (drift <= max_log_scale))
    meas = np.zeros((len(k), 3, 4))
    meas[:, :, :3] = R[k]
    meas[:, :, 3] = t[k] / s[k, None]
    return np.ascontiguousarray(pairs[k], np.int32), meas, _edge_info(n[k] / float(min_inliers), rotation_sigma, translation_sigma), s.copy()
