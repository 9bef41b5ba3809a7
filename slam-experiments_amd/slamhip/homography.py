"""Homography estimation on the GPU (``slam_hg_*``): the branch of ``pose_estimation_2d2d`` the reference leaves unwritten
(``utils.py:27-29``: ``raise NotImplementedError`` above a commented-out ``cv2.findHomography(source_pts, query_pts,
method=RANSAC, ransacReprojThreshold=3)``), its decomposition into poses, and the choice between the homography and the
essential matrix that ORB-SLAM's initialiser makes by score - for many frame pairs per call.

A plane (a wall, a desk, a floor) and a camera turning on the spot are where the essential matrix has no usable answer
(DESIGN.md 4b's table): the homography has one.  Conventions as ``two_view``: points 1 are ``source_pts``, points 2
``query_pts``, ``p2 ~ H p1`` in pixels, ``X2 = R X1 + t`` with ``|t| = 1``, plane normals in frame 1.

PARITY UNPINNED: cv2 is absent here, so the calls are restated from the algorithms' definitions (four-point solver, one-way
transfer error, the decomposition of Ma et al., the cheirality vote of ``recoverPose``, ORB-SLAM's scores).  OpenCV's own random
draws, its early termination and its refit on the inliers are not reproduced: a fixed number of hypotheses from the documented
counter-based generator is scored instead.  There is no CPU fallback.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from ._args import _Buffers
from ._geometry import (MAX_PAIRS, MAX_TOTAL, _cand_offsets, _check_cap, _check_ransac_args, _concat_flags, _flags, _intrinsics, _mask_down,
                        _pair, _pair_arrays, _solve_samples, _split_mask, _Vote)
from ._lib import check
from .device import Context, default_context
from .two_view import DEFAULT_DISTANCE, DEFAULT_HYPOTHESES
from .two_view import DEFAULT_THRESHOLD as DEFAULT_THRESHOLD_E

DEFAULT_THRESHOLD_H = 3.0       # pixels: cv2.findHomography's default, and the value in the reference's comment
DEFAULT_RATIO = 0.45            # ORB-SLAM: the homography is taken when S_H / (S_H + S_E) is above it
DEFAULT_SIGMA = 1.0             # pixels, the standard deviation the scores assume
DEFAULT_AMBIGUITY = 0.75        # ORB-SLAM: ambiguous when the second-best candidate has this share of the best one's points
ROTATION_ONLY = -2              # stats[1] of the decomposition when H is a rotation
NO_MODEL = -1


def _matches(px1, px2, offsets):
    """The checked matches of an offsets call: (px1 [M,2], px2 [M,2], int32 offsets [B + 1], B, M)."""
    px1, px2 = _pair(px1, px2, "px1", "px2", 2)
    offsets, B = _cand_offsets(offsets, MAX_PAIRS, "pairs")
    if len(px1) >= MAX_TOTAL:
        raise ValueError("more than 2^28 matches in one call")
    return px1, px2, offsets, B, len(px1)


def _matrices(A, B, name):
    A = np.ascontiguousarray(A, np.float64)
    if A.size != 9 * max(B, 0):
        raise ValueError(f"{name} must hold one 3x3 matrix per pair ({B}), got shape {A.shape}")
    return A.reshape(-1)


def _positive(v, name):
    if not (np.isfinite(v) and v > 0):
        raise ValueError(f"{name} must be positive")
    return float(v)


def fourpoint_homography_arrays(p1, p2, ctx: Optional[Context] = None):
    """The homography through four correspondences per sample (``slam_hg_fourpoint_f64``): ``p1``, ``p2`` [S,4,2] (or
    [4,2]), pixels or any other unit -> (H [S,3,3] with ``p2 ~ H p1``, Frobenius norm 1, positive projective weights at the
    sample, zero where there is no model; ok bool [S])."""
    p1, p2 = np.asarray(p1, np.float64), np.asarray(p2, np.float64)
    if p1.shape != p2.shape or p1.shape[-2:] != (4, 2) or p1.ndim not in (2, 3):
        raise ValueError(f"p1 and p2 must both have shape [S,4,2], got {p1.shape} and {p2.shape}")
    p1, p2 = np.ascontiguousarray(p1.reshape(-1, 4, 2)), np.ascontiguousarray(p2.reshape(-1, 4, 2))
    S = p1.shape[0]
    if S == 0:
        return np.zeros((0, 3, 3)), np.zeros(0, bool)
    H, ok = _solve_samples(ctx, "slam_hg_fourpoint_f64", p1, p2, (3, 3))
    return H, ok.astype(bool)


def find_homography_offsets(px1, px2, offsets, hypotheses: int = DEFAULT_HYPOTHESES, threshold: float = DEFAULT_THRESHOLD_H,
                            seed: int = 0, ctx: Optional[Context] = None):
    """``slam_hg_ransac_f64`` on concatenated matches: pair b owns ``[offsets[b], offsets[b+1])``.
    Returns (H [B,9], inlier bool [M], stats int32 [B,4])."""
    H, thr, seed = _check_ransac_args(hypotheses, threshold, seed)
    px1, px2, offsets, B, M = _matches(px1, px2, offsets)
    if B == 0:
        return np.zeros((0, 9)), np.zeros(M, bool), np.zeros((0, 4), np.int32)
    ctx = ctx or default_context()
    m = _Buffers(ctx)
    try:
        return _Vote(m, ctx.lib.slam_hg_ransac_f64, (px1, px2), offsets, (H, thr, seed), 9).download()
    finally:
        m.free()


def find_homography_batch(pairs: Sequence, hypotheses: int = DEFAULT_HYPOTHESES, threshold: float = DEFAULT_THRESHOLD_H, seed: int = 0,
                          ctx: Optional[Context] = None):
    """``cv2.findHomography(px1, px2, cv2.RANSAC, threshold)`` for a list of ``(px1, px2)`` pairs in one call:
    (H [B,3,3], list of bool masks, stats [B,4])."""
    px1, px2, off = _pair_arrays(pairs)
    H, mask, st = find_homography_offsets(px1, px2, off, hypotheses, threshold, seed, ctx)
    return H.reshape(-1, 3, 3), _split_mask(mask, off), st


def find_homography_arrays(px1, px2, hypotheses: int = DEFAULT_HYPOTHESES, threshold: float = DEFAULT_THRESHOLD_H, seed: int = 0,
                           ctx: Optional[Context] = None):
    """``cv2.findHomography(px1, px2, cv2.RANSAC, threshold)`` for one pair: (H [3,3], inlier mask bool [N]).  Fewer than
    four matches, or no sample with a model: a zero matrix and an empty vote."""
    H, masks, _ = find_homography_batch([(px1, px2)], hypotheses, threshold, seed, ctx)
    return H[0], masks[0]


def decompose_homography_offsets(H, px1, px2, offsets, K, inlier=None, distance_thresh: float = DEFAULT_DISTANCE,
                                 ctx: Optional[Context] = None):
    """``slam_hg_decompose_f64``: dict with ``pose_all`` [B,4,3,4], ``normal_all`` [B,4,3], ``count`` int32 [B,4], ``pose``
    [B,3,4], ``sv`` [B,3], ``good`` bool [M], ``stats`` int32 [B,4] = {best count, best candidate (-2: rotation only, -1: no
    model), second-best count, number of candidates}."""
    fx, fy, cx, cy = _intrinsics(K)
    dist = _positive(distance_thresh, "distance_thresh")
    px1, px2, offsets, B, M = _matches(px1, px2, offsets)
    H = _matrices(H, B, "H")
    inlier = _flags(inlier, M)
    if B == 0:
        return dict(pose_all=np.zeros((0, 4, 3, 4)), normal_all=np.zeros((0, 4, 3)), count=np.zeros((0, 4), np.int32),
                    pose=np.zeros((0, 3, 4)), sv=np.zeros((0, 3)), good=np.zeros(M, bool), stats=np.zeros((0, 4), np.int32))
    ctx = ctx or default_context()
    m = _Buffers(ctx)
    try:
        d1, d2, do, dH = m.up(px1), m.up(px2), m.up(offsets), m.up(H)
        di = m.up(inlier) if inlier is not None else None
        dpa, dna, dc, dp, dsv, dg, ds = m.new(B * 384), m.new(B * 96), m.new(B * 16), m.new(B * 96), m.new(B * 24), m.new(M), m.new(B * 16)
        check(ctx.lib.slam_hg_decompose_f64(ctx.handle, B, do.ptr, d1.ptr, d2.ptr, M, fx, fy, cx, cy, dH.ptr,
                                            di.ptr if di is not None else None, dist, dpa.ptr, dna.ptr, dc.ptr, dp.ptr, dsv.ptr, dg.ptr,
                                            ds.ptr))
        return dict(pose_all=dpa.download(np.float64, (B, 4, 3, 4)), normal_all=dna.download(np.float64, (B, 4, 3)),
                    count=dc.download(np.int32, (B, 4)), pose=dp.download(np.float64, (B, 3, 4)), sv=dsv.download(np.float64, (B, 3)),
                    good=_mask_down(dg, M), stats=ds.download(np.int32, (B, 4)))
    finally:
        m.free()


def decompose_homography_batch(H, pairs: Sequence, K, inliers=None, distance_thresh: float = DEFAULT_DISTANCE,
                               ctx: Optional[Context] = None):
    """``cv2.decomposeHomographyMat`` and the cheirality vote for a list of pairs: the dict of
    ``decompose_homography_offsets`` with ``good`` as a list of bool masks."""
    px1, px2, off = _pair_arrays(pairs)
    out = decompose_homography_offsets(H, px1, px2, off, K, _concat_flags(inliers, len(off) - 1), distance_thresh, ctx)
    out["good"] = _split_mask(out["good"], off)
    return out


def decompose_homography_arrays(H, px1, px2, K, inlier=None, distance_thresh: float = DEFAULT_DISTANCE, ctx: Optional[Context] = None):
    """One pair: (candidates [4,3,4], normals [4,3], counts int32 [4], stats int32 [4]); fewer candidates leave zero slots."""
    out = decompose_homography_batch(np.asarray(H, np.float64).reshape(1, 9), [(px1, px2)], K, None if inlier is None else [inlier],
                                     distance_thresh, ctx)
    return out["pose_all"][0], out["normal_all"][0], out["count"][0], out["stats"][0]


def model_scores_offsets(H, E, px1, px2, offsets, K, sigma: float = DEFAULT_SIGMA, ctx: Optional[Context] = None):
    """``slam_hg_model_score_f64``: (score int64 [B,2] = {S_H, S_E} in units of 2^-20, ratio [B] = S_H / (S_H + S_E))."""
    fx, fy, cx, cy = _intrinsics(K)
    sigma = _positive(sigma, "sigma")
    if not (0.0 < sigma * sigma < 1e200):
        raise ValueError("sigma squared must be a positive finite double")
    px1, px2, offsets, B, M = _matches(px1, px2, offsets)
    H, E = _matrices(H, B, "H"), _matrices(E, B, "E")
    if B == 0:
        return np.zeros((0, 2), np.int64), np.zeros(0)
    ctx = ctx or default_context()
    m = _Buffers(ctx)
    try:
        d1, d2, do, dH, dE = m.up(px1), m.up(px2), m.up(offsets), m.up(H), m.up(E)
        dsc, dr = m.new(B * 16), m.new(B * 8)
        check(ctx.lib.slam_hg_model_score_f64(ctx.handle, B, do.ptr, d1.ptr, d2.ptr, M, fx, fy, cx, cy, dH.ptr, dE.ptr, sigma, dsc.ptr,
                                              dr.ptr))
        return dsc.download(np.int64, (B, 2)), dr.download(np.float64, (B,))
    finally:
        m.free()


def verify_pairs_auto(pairs: Sequence, K, hypotheses: int = DEFAULT_HYPOTHESES, threshold_e: float = DEFAULT_THRESHOLD_E,
                      threshold_h: float = DEFAULT_THRESHOLD_H, ratio: float = DEFAULT_RATIO, seed: int = 0,
                      sigma: float = DEFAULT_SIGMA, ambiguity: float = DEFAULT_AMBIGUITY, distance_thresh: float = DEFAULT_DISTANCE,
                      ctx: Optional[Context] = None):
    """``estimate_two_view_auto`` for a list of ``(px1, px2)`` candidates on one upload, one call of each kernel entry for the
    whole list (E-RANSAC, H-RANSAC, scores, decomposition, ``recoverPose``): a list of its dicts."""
    fx, fy, cx, cy = _intrinsics(K)
    H, thr_e, seed = _check_ransac_args(hypotheses, threshold_e, seed)
    thr_h = _positive(threshold_h, "threshold_h")
    sigma, dist = _positive(sigma, "sigma"), _positive(distance_thresh, "distance_thresh")
    if not (np.isfinite(ratio) and 0.0 <= ratio <= 1.0):
        raise ValueError("ratio must be in [0, 1]")
    if not (np.isfinite(ambiguity) and 0.0 < ambiguity <= 1.0):
        raise ValueError("ambiguity must be in (0, 1]")
    px1, px2, off = _pair_arrays(pairs)
    B, M = len(off) - 1, len(px1)
    _check_cap(B, MAX_PAIRS, "pairs")
    if B == 0:
        return []
    ctx = ctx or default_context()
    lib, h = ctx.lib, ctx.handle
    m = _Buffers(ctx)
    try:
        d1, d2, do = m.up(px1), m.up(px2), m.up(off)
        dE, dme, dse = m.new(B * 72), m.new(M), m.new(B * 16)
        dH, dmh, dsh = m.new(B * 72), m.new(M), m.new(B * 16)
        dsc, dr = m.new(B * 16), m.new(B * 8)
        dpa, dna, dc, dph, dsv, dgh, dsd = m.new(B * 384), m.new(B * 96), m.new(B * 16), m.new(B * 96), m.new(B * 24), m.new(M), m.new(B * 16)
        dpe, dge, dsr = m.new(B * 96), m.new(M), m.new(B * 8)
        check(lib.slam_tv_essential_ransac_f64(h, B, do.ptr, d1.ptr, d2.ptr, M, fx, fy, cx, cy, H, thr_e, seed, dE.ptr, dme.ptr, dse.ptr))
        check(lib.slam_hg_ransac_f64(h, B, do.ptr, d1.ptr, d2.ptr, M, H, thr_h, seed, dH.ptr, dmh.ptr, dsh.ptr))
        check(lib.slam_hg_model_score_f64(h, B, do.ptr, d1.ptr, d2.ptr, M, fx, fy, cx, cy, dH.ptr, dE.ptr, sigma, dsc.ptr, dr.ptr))
        # the homography is decomposed on its own inliers; recoverPose is given every match, as the reference does (utils.py:25)
        check(lib.slam_hg_decompose_f64(h, B, do.ptr, d1.ptr, d2.ptr, M, fx, fy, cx, cy, dH.ptr, dmh.ptr, dist, dpa.ptr, dna.ptr, dc.ptr,
                                        dph.ptr, dsv.ptr, dgh.ptr, dsd.ptr))
        check(lib.slam_tv_recover_pose_f64(h, B, do.ptr, d1.ptr, d2.ptr, M, fx, fy, cx, cy, dE.ptr, None, dist, dpe.ptr, dge.ptr, dsr.ptr))
        Em, Hm = dE.download(np.float64, (B, 3, 3)), dH.download(np.float64, (B, 3, 3))
        se, sh, sd = dse.download(np.int32, (B, 4)), dsh.download(np.int32, (B, 4)), dsd.download(np.int32, (B, 4))
        score, rat = dsc.download(np.int64, (B, 2)), dr.download(np.float64, (B,))
        pa, na, cnt = dpa.download(np.float64, (B, 4, 3, 4)), dna.download(np.float64, (B, 4, 3)), dc.download(np.int32, (B, 4))
        ph, pe, sv = dph.download(np.float64, (B, 3, 4)), dpe.download(np.float64, (B, 3, 4)), dsv.download(np.float64, (B, 3))
        me, mh = _mask_down(dme, M), _mask_down(dmh, M)
    finally:
        m.free()
    out = []
    for b in range(B):
        use_h = bool(rat[b] > ratio) and sd[b, 1] != NO_MODEL
        sl = slice(off[b], off[b + 1])
        if use_h:
            pose, inl, ncand = ph[b].copy(), mh[sl].copy(), int(sd[b, 3])
            rot_only = bool(sd[b, 1] == ROTATION_ONLY)
            amb = bool(not rot_only and sd[b, 0] > 0 and sd[b, 2] >= ambiguity * sd[b, 0])
        else:
            pose, inl, ncand, rot_only, amb = pe[b].copy(), me[sl].copy(), 0, False, False
            if se[b, 1] < 0:
                pose[:, 3] = 0.0                        # no essential matrix: identity and zero, as estimate_two_view
        out.append(dict(model="H" if use_h else "E", ratio=float(rat[b]), score=score[b].copy(), pose=pose, R=pose[:, :3].copy(),
                        t=pose[:, 3].copy(), inliers=inl, H=Hm[b], E=Em[b], candidates=pa[b, :ncand].copy(), normals=na[b, :ncand].copy(),
                        counts=cnt[b, :ncand].copy(), singular_values=sv[b], rotation_only=rot_only, ambiguous=amb,
                        stats_h=sh[b], stats_e=se[b], stats_decompose=sd[b]))
    return out


def estimate_two_view_auto(px1, px2, K, hypotheses: int = DEFAULT_HYPOTHESES, threshold_e: float = DEFAULT_THRESHOLD_E,
                           threshold_h: float = DEFAULT_THRESHOLD_H, ratio: float = DEFAULT_RATIO, seed: int = 0,
                           sigma: float = DEFAULT_SIGMA, ambiguity: float = DEFAULT_AMBIGUITY, distance_thresh: float = DEFAULT_DISTANCE,
                           ctx: Optional[Context] = None):
    """``pose_estimation_2d2d`` with both of its branches and ORB-SLAM's choice between them.  The essential-matrix RANSAC
    (``estimate_two_view``'s), the homography RANSAC and the two scores run on the matches; where ``S_H / (S_H + S_E)`` is above
    ``ratio`` the pose comes from the homography's decomposition, otherwise from ``recoverPose``.  Returns a dict:

    ``model`` "H" or "E"; ``ratio``; ``score`` int64 {S_H, S_E}; ``pose`` [3,4] (also ``R``, ``t``; ``t`` is zero for a rotation);
    ``inliers`` the chosen model's RANSAC vote; ``H``, ``E``; for H ``candidates`` [C,3,4], ``normals`` [C,3], ``counts`` [C]
    (C = 4, or 1 for a rotation; empty for E); ``rotation_only``; ``ambiguous``: the second-best candidate has at least
    ``ambiguity`` of the best one's points (a plane seen fronto-parallel has two poses that explain it equally well: the
    first is returned and the flag says so)."""
    return verify_pairs_auto([(px1, px2)], K, hypotheses, threshold_e, threshold_h, ratio, seed, sigma, ambiguity, distance_thresh, ctx)[0]
