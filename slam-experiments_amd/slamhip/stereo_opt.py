"""Stereo and level-weighted edges under the pose optimisation and the sparse bundle adjustment.

ORB-SLAM's ``Optimizer::PoseOptimization`` and ``Optimizer::LocalBundleAdjustment`` on arrays: every observation is a
monocular edge (two residuals) or a stereo edge (three: ``u_right`` is the third measurement) with an information
``1 / scale[level]^2``; the chi-square gate and the Huber width depend on the kind of the edge.  The edge model is one
text for host and device (``csrc/stereo_edge.h``); the kernels are ``csrc/pose_stereo.hip`` and ``csrc/ba_stereo.hip``.
There is no CPU fallback.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from ._frames import pose_rows, refine_frames
from ._lib import check
from .ba import BAResult, fixed_pose_mask, lm_schedule, state_arrays
from .ba_sparse import DEFAULT_PCG_TOL, SparseBAProblem, _deltas, _stereo_arrays
from .device import Context, default_context
from .pose_graph import DEFAULT_PCG_MAX_ITER, _check_solver_args

CHI2_MONO, CHI2_STEREO = 5.991, 7.815                     # the 95 % quantiles of chi-square with 2 and 3 degrees of freedom
DELTA_MONO, DELTA_STEREO = CHI2_MONO ** 0.5, CHI2_STEREO ** 0.5
STAGE = 512                                               # SLAM_POSE_STEREO_STAGE: edges of a frame the kernel keeps in LDS


@dataclass
class StereoEdges:
    """The measurements of a set of edges: ``meas3`` f64 [O,3] = (mu, mv, mr), mr NaN for a monocular edge; ``info`` f64 [O],
    the inverse variance of each (0 switches an edge off); ``bf`` focal length times baseline."""

    meas3: np.ndarray
    info: np.ndarray
    bf: float

    def __len__(self):
        return len(self.info)


def stereo_edges(result, b: int, rows=None, scale=None) -> StereoEdges:
    """The edges of pair ``b`` of a ``StereoResult`` (all left rows, or ``rows``): (mu, mv) = ``xy``, mr = ``u_right`` where the
    status is matched and NaN elsewhere, info = 1 / scale[level]^2 (``scale``: the result's table unless given)."""
    if not 0 <= int(b) < len(result):
        raise ValueError(f"pair {b} is outside the result's {len(result)} pairs")
    b = int(b)
    n = len(result.status[b])
    rows = np.arange(n) if rows is None else np.asarray(rows)
    if rows.size == 0:
        rows = np.zeros(0, np.int64)
    if rows.dtype.kind not in "iu" or rows.ndim != 1 or (len(rows) and (rows.min() < 0 or rows.max() >= n)):
        raise ValueError(f"rows must be integers in [0, {n})")
    sc = np.asarray(result.scale if scale is None else scale, np.float64).reshape(-1)
    lv = np.asarray(result.level[b])[rows]
    if len(lv) and (lv.min() < 0 or lv.max() >= len(sc)):
        raise ValueError("a keypoint level is outside the scale table")
    if not (np.isfinite(sc).all() and (sc > 0).all()):
        raise ValueError("scale must be positive and finite")
    ur = np.where(np.asarray(result.status[b])[rows] == 0, np.asarray(result.u_right[b], np.float64)[rows], np.nan)
    meas3 = np.concatenate([np.asarray(result.xy[b], np.float64)[rows].reshape(-1, 2), ur.reshape(-1, 1)], 1)
    return StereoEdges(np.ascontiguousarray(meas3), 1.0 / (sc[lv] * sc[lv]), float(result.bf))


def _model_args(intrinsics, bf, gates, deltas):
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    bf = float(bf)
    if not (np.isfinite([fx, fy, cx, cy]).all() and fx != 0 and fy != 0):
        raise ValueError("intrinsics must be finite, fx and fy not 0")
    if not (np.isfinite(bf) and bf > 0):
        raise ValueError("bf must be positive and finite")
    g = np.asarray(gates, np.float64).reshape(-1)
    if g.shape != (2,) or not (g >= 0).all():
        raise ValueError("the gates (chi2_mono, chi2_stereo) must not be negative")
    return fx, fy, cx, cy, bf, float(g[0]), float(g[1]), _deltas(deltas)


def stereo_edge_linearization(poses, points, obs_pose_idx, obs_point_idx, edges: StereoEdges, intrinsics,
                              deltas=(0.0, 0.0), ctx: Optional[Context] = None):
    """``slam_reproj_rj_stereo_f64``: every edge linearised -> dict(e [O,3], Jpose [O,3,6], Jpoint [O,3,3], chi2 [O], w [O]).
    ``poses`` [K,4,4] / [K,3,4] / [K,12], ``points`` [L,3]; row 2 of a monocular edge is 0."""
    T12, X, K, L = state_arrays(poses, points)
    op, ol = np.ascontiguousarray(obs_pose_idx, np.int32).reshape(-1), np.ascontiguousarray(obs_point_idx, np.int32).reshape(-1)
    O = len(op)
    if len(ol) != O:
        raise ValueError("obs_pose_idx and obs_point_idx must have one entry per observation")
    meas3, info, bf = _stereo_arrays(edges, O)
    fx, fy, cx, cy, bf, _, _, (dm, ds) = _model_args(intrinsics, bf, (0.0, 0.0), deltas)
    ctx = ctx or default_context()
    o = max(O, 1)
    bufs = []
    try:
        up = lambda a: bufs.append(ctx.upload(a)) or bufs[-1]          # noqa: E731
        new = lambda n: bufs.append(ctx.malloc(n)) or bufs[-1]         # noqa: E731
        d_T, d_X = up(T12), up(X)
        d_op, d_ol = up(op if O else np.zeros(1, np.int32)), up(ol if O else np.zeros(1, np.int32))
        d_m, d_s = up(meas3 if O else np.zeros((1, 3))), up(info if O else np.zeros(1))
        d_e, d_jp, d_jq, d_c, d_w = new(o * 24), new(o * 144), new(o * 72), new(o * 8), new(o * 8)
        check(ctx.lib.slam_reproj_rj_stereo_f64(ctx.handle, d_T.ptr, K, d_X.ptr, L, d_op.ptr, d_ol.ptr, d_m.ptr, d_s.ptr, O, fx, fy, cx, cy, bf,
                                                dm, ds, d_e.ptr, d_jp.ptr, d_jq.ptr, d_c.ptr, d_w.ptr))
        return dict(e=d_e.download(np.float64, (o, 3))[:O], Jpose=d_jp.download(np.float64, (o, 3, 6))[:O],
                    Jpoint=d_jq.download(np.float64, (o, 3, 3))[:O], chi2=d_c.download(np.float64, (o,))[:O],
                    w=d_w.download(np.float64, (o,))[:O])
    finally:
        for b in bufs:
            b.free()


def optimize_poses_stereo(poses, points_list, edges_list, intrinsics, bf, rounds: int = 4, iterations: int = 10,
                          gates=(CHI2_MONO, CHI2_STEREO), deltas=(DELTA_MONO, DELTA_STEREO), ctx: Optional[Context] = None,
                          stats_out: Optional[list] = None):
    """ORB-SLAM's ``Optimizer::PoseOptimization`` for B independent frames in ONE kernel launch (one workgroup per frame,
    ``slam_pose_optimize_stereo_batch_f64``): ``poses`` [B,4,4] (or [B,3,4]), ``points_list[b]`` [O_b,3] map points,
    ``edges_list[b]`` a ``StereoEdges`` of O_b edges.  ORB-SLAM's defaults: 4 rounds of 10 iterations, gates 5.991 / 7.815 on the
    weighted chi2, Huber widths their square roots, dropped after round index 2.  Returns a list of ``PoseOptResult`` (chi2: the
    weighted chi2; inliers: information > 0, positive depth and the gate of the edge's kind).  ``stats_out``, when a list, receives
    the int32 [B,4] table {inliers, accepted steps, stereo inliers, edges with information > 0}."""
    B = np.asarray(poses).shape[0]
    if len(points_list) != B or len(edges_list) != B:
        raise ValueError("one point array and one set of edges per pose")
    fx, fy, cx, cy, bf, gm, gs, (dm, ds) = _model_args(intrinsics, bf, gates, deltas)
    for name, v, hi in (("rounds", rounds, 64), ("iterations", iterations, 1000)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= hi:
            raise ValueError(f"{name} must be an integer in [0, {hi}]")
    if B == 0:
        return []
    pts = [np.ascontiguousarray(p, np.float64).reshape(-1, 3) for p in points_list]
    arr = [_stereo_arrays(e, len(p)) for e, p in zip(edges_list, pts)]
    if any(a[2] != bf for a in arr):
        raise ValueError("every set of edges must carry the bf of the call")
    ctx = ctx or default_context()

    def call(d_pose, d_cols, d_off, O, d_out, d_inl, d_chi, d_st):
        check(ctx.lib.slam_pose_optimize_stereo_batch_f64(ctx.handle, B, d_pose.ptr, d_cols[0].ptr, d_cols[1].ptr, d_cols[2].ptr, d_off.ptr, O, fx,
                                                          fy, cx, cy, bf, int(rounds), int(iterations), gm, gs, dm, ds, d_out.ptr, d_inl.ptr,
                                                          d_chi.ptr, d_st.ptr))

    res, st = refine_frames(ctx, pose_rows(poses), [p.shape[0] for p in pts], [(pts, 3), ([a[0] for a in arr], 3), ([a[1] for a in arr], 1)], 4,
                            call)
    if stats_out is not None:
        stats_out.append(st)
    return res


def local_bundle_adjust(poses, points, obs_pose_idx, obs_point_idx, stereo: StereoEdges, intrinsics, fixed_poses: Sequence[int] = (0,),
                        first: int = 5, second: int = 10, gates=(CHI2_MONO, CHI2_STEREO), deltas=(DELTA_MONO, DELTA_STEREO),
                        pcg_tol: float = DEFAULT_PCG_TOL, pcg_max_iter: int = DEFAULT_PCG_MAX_ITER, ctx: Optional[Context] = None):
    """The schedule of ORB-SLAM's ``Optimizer::LocalBundleAdjustment`` on the sparse adjustment: ``first`` iterations under the
    Huber kernel, a classification, the outliers switched off (information 0, in the device table: the problem is not
    rebuilt) and the kernel dropped, ``second`` more iterations, a second classification.

    Returns ``(BAResult, outliers, stats)``: ``outliers`` int64, ascending: the observations switched off after the first
    stage and those the second classification turns down (ORB-SLAM erases both from the map at this point; an edge the caller
    gave information 0 is neither); stats = dict(trials, cg_iterations, status, unconverged, outliers_first, edges, pairs).
    An edge is an inlier iff its information is > 0, its depth positive and its weighted chi2 within the gate of its kind."""
    T12, X, K, L = state_arrays(poses, points)
    fx, fy, cx, cy, bf, gm, gs, dl = _model_args(intrinsics, stereo.bf, gates, deltas)
    for n in (first, second):
        _check_solver_args(n, min(dl), pcg_tol, pcg_max_iter)
    fixed = fixed_pose_mask(fixed_poses, K)
    ctx = ctx or default_context()
    prob = SparseBAProblem(ctx, K, L, obs_pose_idx, obs_point_idx, None, (fx, fy, cx, cy), fixed, "host", stereo)
    st = dict(trials=0, cg_iterations=0, status=0, unconverged=0, outliers_first=0, edges=prob.E, pairs=prob.P)

    def stage(iterations, delta):
        def trial(lam, cost):
            st["trials"] += 1
            prob.reduce(lam)
            cg = prob.solve(lam, pcg_tol, pcg_max_iter)
            st["cg_iterations"] += cg["iterations"]
            st["status"] |= cg["status"]
            if not cg["converged"]:
                st["unconverged"] += 1
                return cost, np.nan, np.nan
            denominator, new = prob.step(lam, delta)
            return cost, new, denominator

        def accept(it):
            prob.accept()
            if it + 1 < int(iterations):
                prob.linearize(delta)

        cost0, dmax = prob.linearize(delta)
        cost, _, accepted = lm_schedule(iterations, cost0, dmax, trial, accept)
        return cost0, cost, accepted

    try:
        prob.set_state(T12, X)
        info = np.ascontiguousarray(stereo.info, np.float64)
        cost0, _, acc1 = stage(first, dl)
        _, inl = prob.classify(gm, gs)
        st["outliers_first"] = int((~inl & (info > 0)).sum())
        prob.set_info(np.where(inl, info, 0.0))
        _, cost, acc2 = stage(second, (0.0, 0.0))
        _, inl = prob.classify(gm, gs)                        # a switched-off edge is no inlier: the list is the union of both stages
        Tout, Xout = prob.state()
    finally:
        prob.free()
    Tr = np.tile(np.eye(4), (K, 1, 1))
    Tr[:, :3, :4] = Tout.reshape(K, 3, 4)
    return BAResult(poses=Tr, points=Xout, chi2_initial=cost0, chi2_final=cost, iterations=acc1 + acc2), np.flatnonzero(~inl & (info > 0)), st
