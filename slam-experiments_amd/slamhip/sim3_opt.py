"""Sim(3) refinement by reprojection error on the GPU (``slam_sim3_optimize_f64``): ORB-SLAM's ``Optimizer::OptimizeSim3``,
the step its ``ComputeSim3`` runs between the ``Sim3Solver`` (``estimate_sim3_batch``) and the fusion (``fuse_by_sim3``), for
many loop candidates per call.  A 7-DoF Levenberg-Marquardt refinement of ``X2 = s R X1 + t`` on the reprojection error of the
matched map points in both images against the MEASURED keypoints under a Huber kernel, a chi-square gate, a second refinement
on the survivors and the count of survivors a loop is accepted on.

PARITY UNPINNED: ORB-SLAM and g2o are absent here; the call is restated from the algorithm's definition with a rational
retraction (Cayley rotation, quadratic scale) in place of ``Sim3::exp`` so that a host build gives the device's bits, and
the map points are constants.  The result is a model, so no consumer sees the chart.  There is no CPU fallback.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from ._args import _Buffers
from ._geometry import _cand_offsets, _concat, _intrinsics, _mask_down, _model_srt, _pair, _rows, _split_mask
from ._lib import check
from .device import Context, default_context
from .sim3 import estimate_sim3_batch

DEFAULT_TH2 = 10.0                    # ORB-SLAM's ComputeSim3: OptimizeSim3(..., th2 = 10, ...)
DEFAULT_ITERATIONS = (5, 10, 5)       # stage 1; stage 2 after outliers left; stage 2 when none left
DEFAULT_MIN_PAIRS = 10                # fewer survivors of stage 1: the candidate is rejected
DEFAULT_MIN_INLIERS = 20              # ORB-SLAM accepts the loop on nInliers >= 20
MAX_CANDIDATES = 65535
REJECTED, BAD_MODEL, STALLED = 1, 2, 4   # status bits of stats[:, 3]


def _is_srt(models) -> bool:
    return isinstance(models, (tuple, list)) and len(models) == 3 and np.ndim(models[1]) >= 2


def _models13(models, B: Optional[int] = None) -> np.ndarray:
    """[B,13] from a flat array or from (s [B], R [B,3,3], t [B,3])."""
    if _is_srt(models):
        s = np.asarray(models[0], np.float64).reshape(-1)
        R = np.asarray(models[1], np.float64).reshape(-1, 3, 3)
        t = np.asarray(models[2], np.float64).reshape(-1, 3)
        if not len(s) == len(R) == len(t):
            raise ValueError("models must be (s [B], R [B,3,3], t [B,3])")
        Z = np.concatenate([np.concatenate([R, t[:, :, None]], 2).reshape(-1, 12), s[:, None]], 1)
    else:
        Z = np.asarray(models, np.float64).reshape(-1, 13)
    if B is not None and len(Z) != B:
        raise ValueError(f"{B} candidates but {len(Z)} models")
    return np.ascontiguousarray(Z)


def _check_args(th2, iterations, min_pairs):
    th2 = float(th2)
    if not (th2 > 0 and np.isfinite(th2)):
        raise ValueError("th2 must be positive and finite")
    it = [int(v) for v in iterations]
    if len(it) != 3 or min(it) < 0 or max(it) > 1000:
        raise ValueError("iterations must be three counts in [0, 1000]: (stage 1, stage 2 after outliers, stage 2 without)")
    if int(min_pairs) < 1:
        raise ValueError("min_pairs must be at least 1")
    return th2, it, int(min_pairs)


def optimize_sim3_offsets(X1, X2, px1, px2, offsets, models, K, sigma2=None, th2: float = DEFAULT_TH2,
                          iterations: Sequence[int] = DEFAULT_ITERATIONS, min_pairs: int = DEFAULT_MIN_PAIRS, fix_scale: bool = False,
                          ctx: Optional[Context] = None):
    """``slam_sim3_optimize_f64`` on concatenated correspondences: candidate b owns ``[offsets[b], offsets[b+1])`` of ``X1`` /
    ``X2`` [M,3] (the matched map points, each in its own camera frame) and ``px1`` / ``px2`` [M,2] (their measured keypoints
    in image 1 / image 2); ``sigma2`` [M,2] the squared keypoint sigmas (None: all 1); ``models`` [B,13] or (s, R, t) the
    starts, ``X2 = s R X1 + t``.
    Returns (s [B], R [B,3,3], t [B,3], inlier bool [M], stats int32 [B,4] = {inliers, accepted steps, nBad, status},
    chi2 f64 [M,2] = (c1, c2) at the returned model, NaN where the header says so).  A rejected candidate (status & 1)
    returns its input model, an empty mask and a count of 0."""
    fx, fy, cx, cy = _intrinsics(K)
    th2, it, min_pairs = _check_args(th2, iterations, min_pairs)
    X1, X2 = _pair(X1, X2, "X1", "X2", 3, "correspondences")
    M = len(X1)
    px1, px2 = _rows(px1, M, "px1"), _rows(px2, M, "px2")
    sg = None if sigma2 is None else _rows(sigma2, M, "sigma2")
    offsets, B = _cand_offsets(offsets, MAX_CANDIDATES, "candidates")
    Z = _models13(models, B)
    if B == 0:
        return np.zeros(0), np.zeros((0, 3, 3)), np.zeros((0, 3)), np.zeros(M, bool), np.zeros((0, 4), np.int32), np.full((M, 2), np.nan)
    ctx = ctx or default_context()
    m = _Buffers(ctx)
    try:
        d1, d2, dp1, dp2, do, dz = m.up(X1), m.up(X2), m.up(px1), m.up(px2), m.up(offsets), m.up(Z)
        dsg = m.up(sg) if sg is not None else None
        dT, dm, dc, ds = m.new(B * 104), m.new(M), m.up(np.full((max(M, 1), 2), np.nan)), m.new(B * 16)
        check(ctx.lib.slam_sim3_optimize_f64(ctx.handle, B, do.ptr, d1.ptr, d2.ptr, dp1.ptr, dp2.ptr, M, dsg.ptr if dsg is not None else None,
                                             dz.ptr, fx, fy, cx, cy, th2, it[0], it[1], it[2], min_pairs, int(bool(fix_scale)), dT.ptr,
                                             dm.ptr, dc.ptr, ds.ptr))
        model, st = dT.download(np.float64, (B, 13)), ds.download(np.int32, (B, 4))
        mask = _mask_down(dm, M)
        chi2 = dc.download(np.float64, (max(M, 1), 2))[:M]
    finally:
        m.free()
    return _model_srt(model) + (mask, st, chi2)


def optimize_sim3_batch(cands: Sequence, models, K, th2: float = DEFAULT_TH2, iterations: Sequence[int] = DEFAULT_ITERATIONS,
                        min_pairs: int = DEFAULT_MIN_PAIRS, fix_scale: bool = False, ctx: Optional[Context] = None):
    """``Optimizer::OptimizeSim3`` for a list of ``(X1 [N_b,3], X2 [N_b,3], px1 [N_b,2], px2 [N_b,2])`` or ``(..., sigma2
    [N_b,2])`` candidates in one call: (s [B], R [B,3,3], t [B,3], list of bool masks, stats int32 [B,4], list of chi2
    [N_b,2]), as ``optimize_sim3_offsets``."""
    X1, X2, px1, px2, sg, off = _concat(cands, "candidate", (("X1", 3), ("X2", 3), ("px1", 2), ("px2", 2)), "correspondences", sigma2=True)
    s, R, t, mask, st, chi2 = optimize_sim3_offsets(X1, X2, px1, px2, off, models, K, sg, th2, iterations, min_pairs, fix_scale, ctx)
    return s, R, t, _split_mask(mask, off), st, _split_mask(chi2, off)


def optimize_sim3(X1, X2, px1, px2, model, K, sigma2=None, th2: float = DEFAULT_TH2, iterations: Sequence[int] = DEFAULT_ITERATIONS,
                  min_pairs: int = DEFAULT_MIN_PAIRS, fix_scale: bool = False, ctx: Optional[Context] = None):
    """One candidate: (ok, s, R [3,3], t [3], inlier mask bool [N], stats int32 [4], chi2 [N,2]); ``ok`` is False when the
    candidate was rejected (the input model comes back, the mask is empty)."""
    X1, X2 = _pair(X1, X2, "X1", "X2", 3, "correspondences")
    s, R, t, mask, st, chi2 = optimize_sim3_offsets(X1, X2, px1, px2, [0, len(X1)], model, K, sigma2, th2, iterations, min_pairs, fix_scale, ctx)
    return not bool(st[0, 3] & REJECTED), float(s[0]), R[0], t[0], mask, st[0], chi2


def sim3_to_s12(model) -> np.ndarray:
    """The inverse of a model ``X2 = s R X1 + t`` as ``[sR | t]`` f64 [3,4] taking camera-2 coordinates into camera 1,
    ``X1 = (1 / s) R^T (X2 - t)``: the form ``search_by_sim3`` and ``fuse_by_sim3`` take.  ``model``: [13], [B,13] or
    (s, R, t) (-> [3,4], or [B,3,4] for batched input)."""
    batched = np.ndim(model[1]) == 3 if _is_srt(model) else np.ndim(model) == 2
    s, R, t = _model_srt(_models13(model))
    if not (np.isfinite(s).all() and (s > 0).all()):
        raise ValueError("a similarity needs a finite positive scale")
    Ri = np.swapaxes(R, 1, 2) / s[:, None, None]
    out = np.concatenate([Ri, -(Ri @ t[:, :, None])], 2)
    return out if batched else out[0]


def compute_sim3(cands: Sequence, K, min_inliers: int = DEFAULT_MIN_INLIERS, hypotheses: int = 256, chi2_gate: float = 9.210,
                 th2: float = DEFAULT_TH2, iterations: Sequence[int] = DEFAULT_ITERATIONS, min_pairs: int = DEFAULT_MIN_PAIRS,
                 fix_scale: bool = False, seed: int = 0, ctx: Optional[Context] = None):
    """The estimation half of ORB-SLAM's ``LoopClosing::ComputeSim3`` for a list of ``(X1, X2, px1, px2[, sigma2])``
    candidates: ``estimate_sim3_batch`` (RANSAC + refit), then ``optimize_sim3_batch`` on each candidate's RANSAC inliers.
    Returns (models = (s [B], R [B,3,3], t [B,3]) - the form ``sim3_edges_from_sim3`` takes -, list of bool masks over each
    candidate's ORIGINAL indexing, counts int32 [B], accepted bool [B] = count >= ``min_inliers``, stats int32 [B,4]).
    A candidate the refinement rejects keeps its RANSAC model with a count of 0."""
    if int(min_inliers) < 1:
        raise ValueError("min_inliers must be at least 1")
    cands = [tuple(c) for c in cands]
    for i, c in enumerate(cands):
        if len(c) not in (4, 5):
            raise ValueError(f"candidate {i}: expected (X1, X2, px1, px2) or (X1, X2, px1, px2, sigma2)")
    has = [len(c) == 5 and c[4] is not None for c in cands]
    s, R, t, rmasks, _, _ = estimate_sim3_batch([(c[0], c[1]) + ((c[4],) if h else ()) for c, h in zip(cands, has)], K, hypotheses,
                                                chi2_gate, fix_scale, seed, True, ctx)
    sub = []
    for c, h, mk in zip(cands, has, rmasks):
        pick = lambda a, w: np.asarray(a, np.float64).reshape(len(mk), w)[mk]
        sub.append((pick(c[0], 3), pick(c[1], 3), pick(c[2], 2), pick(c[3], 2)) + ((pick(c[4], 2),) if h else ()))
    s, R, t, omasks, st, _ = optimize_sim3_batch(sub, (s, R, t), K, th2, iterations, min_pairs, fix_scale, ctx)
    masks = []
    for mk, om in zip(rmasks, omasks):
        full = np.zeros(len(mk), bool)
        full[np.flatnonzero(mk)[om]] = True
        masks.append(full)
    counts = st[:, 0].copy() if len(st) else np.zeros(0, np.int32)
    return (s, R, t), masks, counts, counts >= int(min_inliers), st
