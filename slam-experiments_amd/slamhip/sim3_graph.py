"""Sim(3) pose-graph optimisation on the GPU (``slam_s3g_*``): ORB-SLAM's ``OptimizeEssentialGraph`` on arrays.

The last step of the loop-closure chain for a monocular map: ``KeyframeDatabase`` proposes keyframe pairs,
``estimate_sim3_batch`` turns them into similarities ``X_j = s R X_i + t``, ``sim3_edges_from_sim3`` turns EVERY accepted
one into a 7-DoF edge (at any scale), ``lift_se3_graph`` brings the odometry edges along, ``optimize_sim3_graph`` spreads
the scale drift over the trajectory, ``sims_to_poses`` and ``correct_points`` bring keyframes and map points back.

Conventions (``include/slamhip.h``): a vertex is ``S = (s, R, t)`` with ``X_cam = s R X_world + t``, stored ``[13]``: the
row-major 3x4 ``[R|t]`` then ``s`` (the model layout of ``slamhip.sim3``).  Tangent ``[w, v, sigma]``; chart
``Phi(d) = Exp_SE3(w, v) o Scale(e^sigma)``; update ``S <- Phi(d) o S``.  Edge ``(i, j)`` carries ``Z ~ S_j S_i^-1``;
``r = Phi^-1(S_j S_i^-1 Z^-1) = [Log_SE3(R_D, t_D), log s_D]``; ``F = sum rho(r^T Omega r)``, ``Omega`` [7,7] in
``[w, v, sigma]`` order.  The chart is the exact inverse of the retraction and differs from g2o's ``Sim3::log`` at second
order in ``sigma * v``: PARITY UNPINNED against g2o / ORB-SLAM (absent here).  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from ._geometry import _check_edge_args, _edge_info, _edge_pairs
from ._lib import addr, check
from .device import Context, default_context
from .pose_graph import (DEFAULT_ITERATIONS, DEFAULT_PCG_MAX_ITER, DEFAULT_PCG_TOL, MAX_EDGES, MAX_VERTICES, STATS_FIELDS, _Dev,
                         _check_solver_args, _edges_array, _poses12, vertex_lists)

STATUS_BITS = {1: "index", 2: "angle", 4: "precond", 8: "breakdown", 16: "nonfinite", 32: "scale"}


# ---------------------------------------------------------------- argument coercion -----------------------------------------
def is_srt(sims) -> bool:
    """True for the tuple form (s [N], R [N,3,3], t [N,3]); a list of three 13-vectors is an array of three vertices"""
    return (isinstance(sims, (tuple, list)) and len(sims) == 3 and np.ndim(sims[0]) == 1 and np.ndim(sims[1]) == 3 and
            np.shape(sims[1])[1:] == (3, 3) and np.ndim(sims[2]) == 2 and np.shape(sims[2])[1] == 3)


def _sims13(sims, name="sims") -> np.ndarray:
    """[N,13] or the tuple (s [N], R [N,3,3], t [N,3]) -> contiguous float64 [N,13]"""
    if is_srt(sims):
        s = np.asarray(sims[0], np.float64).reshape(-1)
        R = np.asarray(sims[1], np.float64).reshape(-1, 3, 3)
        t = np.asarray(sims[2], np.float64).reshape(-1, 3)
        if not (len(s) == len(R) == len(t)):
            raise ValueError(f"{name}: {len(s)} scales, {len(R)} rotations and {len(t)} translations")
        out = np.empty((len(s), 13))
        out[:, :12] = np.concatenate([R, t[:, :, None]], 2).reshape(-1, 12)
        out[:, 12] = s
        return out
    a = np.asarray(sims)
    if a.dtype.kind not in "fiu":
        raise ValueError(f"{name} must be numeric, got dtype {a.dtype}")
    if a.size == 0:
        return np.zeros((0, 13))
    if a.ndim != 2 or a.shape[1] != 13:
        raise ValueError(f"{name} must have shape [N,13] or be the tuple (s, R, t), got {a.shape}")
    return np.ascontiguousarray(a, np.float64)


def split(sims):
    """(s [...], R [...,3,3], t [...,3]) of sims [...,13]."""
    m = np.asarray(sims, np.float64)
    T = m[..., :12].reshape(m.shape[:-1] + (3, 4))
    return m[..., 12].copy(), T[..., :3].copy(), T[..., 3].copy()


def _as_input(out13, src):
    if is_srt(src):
        return split(out13)
    return out13


def _graph_arrays(sims, edges, meas, info, fixed):
    S = _sims13(sims)
    V = len(S)
    e = _edges_array(edges)
    E = len(e)
    Z = _sims13(meas, "meas")
    if len(Z) != E:
        raise ValueError(f"{E} edges but {len(Z)} measurements")
    Om = np.asarray(info)
    if Om.dtype.kind not in "fiu":
        raise ValueError(f"info must be numeric, got dtype {Om.dtype}")
    if Om.size == 0:
        Om = np.zeros((0, 7, 7))
    if Om.shape != (E, 7, 7):
        raise ValueError(f"info must have shape [E,7,7] = ({E}, 7, 7), got {Om.shape}")
    Om = np.ascontiguousarray(Om, np.float64)
    fx = None
    if fixed is not None:
        fx = np.asarray(fixed)
        if fx.shape != (V,):
            raise ValueError(f"fixed must be a mask of shape [V] = ({V},), got {fx.shape}")
        fx = np.ascontiguousarray(fx != 0, np.uint8)
    if V > MAX_VERTICES or E > MAX_EDGES:
        raise ValueError(f"at most {MAX_VERTICES} vertices and {MAX_EDGES} edges")
    return S, e, Z, Om, fx


def status_names(status: int):
    return [name for bit, name in STATUS_BITS.items() if int(status) & bit]


def plan(V: int, E: int) -> dict:
    """The launch plan for a graph of V vertices and E edges, without a device (``slam_s3g_plan``), and the workspace it takes."""
    from . import _lib

    lib = _lib.load()
    p = (ctypes.c_int32 * 8)()
    n = ctypes.c_uint64(0)
    check(lib.slam_s3g_plan(int(V), int(E), p))
    check(lib.slam_s3g_workspace(int(V), int(E), ctypes.byref(n)))
    names = ("product_blocks", "hub_blocks", "vertices_per_block", "hub_degree", "edge_blocks", "cg_check", "launches_per_cg_iteration",
             "slot_row_doubles")
    out = dict(zip(names, p))
    out["workspace_bytes"] = n.value
    return out


# ---------------------------------------------------------------- the calls ---------------------------------------------------
def optimize_sim3_graph(sims, edges, meas, info, fixed, iterations: int = DEFAULT_ITERATIONS, huber_delta: float = 0.0,
                        pcg_tol: float = DEFAULT_PCG_TOL, pcg_max_iter: int = DEFAULT_PCG_MAX_ITER, fix_scale: bool = False,
                        ctx: Optional[Context] = None):
    """ORB-SLAM's ``OptimizeEssentialGraph`` on arrays: ``sims`` [V,13] or the tuple ``(s, R, t)``, ``edges`` int [E,2],
    ``meas`` (the same formats, ``S_j S_i^-1``), ``info`` [E,7,7] in ``[w, v, sigma]`` order, ``fixed`` mask [V] (at least one
    set) -> (sims in the input's form, stats dict: chi2_initial, chi2_final, iterations, trials, cg_iterations, lam, status).
    ``fix_scale`` (``mbFixScale``) freezes every scale: each ``s`` comes back bit for bit."""
    S, e, Z, Om, fx = _graph_arrays(sims, edges, meas, info, fixed)
    if fx is None:
        raise ValueError("fixed must be given: a graph needs at least one fixed vertex")
    _check_solver_args(iterations, huber_delta, pcg_tol, pcg_max_iter)
    V, E = len(S), len(e)
    if V and not fx.any():
        raise ValueError("a graph needs at least one fixed vertex")
    out = np.empty_like(S)
    stats = np.zeros(8)
    if V:
        ctx = ctx or default_context()
        check(ctx.lib.slam_s3g_optimize_host_f64(ctx.handle, V, E, addr(S), addr(e) if E else None, addr(Z) if E else None,
                                                 addr(Om) if E else None, addr(fx), int(iterations), float(huber_delta), float(pcg_tol),
                                                 int(pcg_max_iter), int(bool(fix_scale)), addr(out), addr(stats)))
    st = dict(zip(STATS_FIELDS, stats[:7]))
    for k in ("iterations", "trials", "cg_iterations", "status"):
        st[k] = int(st[k])
    return _as_input(out, sims), st


def sim3_graph_linearize(sims, edges, meas, info, huber_delta: float = 0.0, ctx: Optional[Context] = None):
    """``slam_s3g_linearize_f64``: (cost, gradient b [V,7], diagonal blocks [V,7,7], edge blocks W_e [E,7,7], status)."""
    S, e, Z, Om, _ = _graph_arrays(sims, edges, meas, info, None)
    V, E = len(S), len(e)
    if V == 0:
        return 0.0, np.zeros((0, 7)), np.zeros((0, 7, 7)), np.zeros((0, 7, 7)), 0
    ptr, adj = vertex_lists(V, e)
    ctx = ctx or default_context()
    m = _Dev(ctx)
    try:
        dS, de, dZ, dO, dp, da = m.up(S), m.up(e), m.up(Z), m.up(Om), m.up(ptr), m.up(adj)
        dc, dg, dH, dW = m.new(8), m.new(V * 56), m.new(V * 392), m.new(E * 392)
        status = ctypes.c_int32(0)
        check(ctx.lib.slam_s3g_linearize_f64(ctx.handle, V, E, dS.ptr, de.ptr, dZ.ptr, dO.ptr, dp.ptr, da.ptr, float(huber_delta),
                                             dc.ptr, dg.ptr, dH.ptr, dW.ptr, ctypes.byref(status)))
        cost = float(dc.download(np.float64, (1,))[0])
        W = dW.download(np.float64, (E, 7, 7)) if E else np.zeros((0, 7, 7))
        return cost, dg.download(np.float64, (V, 7)), dH.download(np.float64, (V, 7, 7)), W, int(status.value)
    finally:
        m.free()


def _system_arrays(edges, fixed, Hdiag, W):
    Hd = np.ascontiguousarray(Hdiag, np.float64)
    if Hd.ndim != 3 or Hd.shape[1:] != (7, 7):
        raise ValueError(f"Hdiag must have shape [V,7,7], got {Hd.shape}")
    V = len(Hd)
    e = _edges_array(edges)
    Wb = np.ascontiguousarray(W, np.float64).reshape(-1, 7, 7)
    if len(Wb) != len(e):
        raise ValueError(f"{len(e)} edges but {len(Wb)} edge blocks")
    fx = np.asarray(fixed)
    if fx.shape != (V,):
        raise ValueError(f"fixed must have shape [V] = ({V},), got {fx.shape}")
    return V, e, Hd, Wb, np.ascontiguousarray(fx != 0, np.uint8)


def sim3_graph_hmul(edges, fixed, Hdiag, W, lam: float, x, ctx: Optional[Context] = None) -> np.ndarray:
    """``slam_s3g_hmul_f64``: y [V,7] = (H + lam I) x over the free vertices, H from ``sim3_graph_linearize``'s blocks."""
    V, e, Hd, Wb, fx = _system_arrays(edges, fixed, Hdiag, W)
    x = np.ascontiguousarray(x, np.float64)
    if x.size != 7 * V:
        raise ValueError(f"x must hold 7 V = {7 * V} values, got {x.size}")
    if V == 0:
        return np.zeros((0, 7))
    ptr, adj = vertex_lists(V, e)
    ctx = ctx or default_context()
    m = _Dev(ctx)
    try:
        de, dp, da, df, dH, dW, dx = m.up(e), m.up(ptr), m.up(adj), m.up(fx), m.up(Hd), m.up(Wb), m.up(x)
        dy = m.new(V * 56)
        check(ctx.lib.slam_s3g_hmul_f64(ctx.handle, V, len(e), de.ptr, dp.ptr, da.ptr, df.ptr, dH.ptr, dW.ptr, float(lam), dx.ptr, dy.ptr))
        return dy.download(np.float64, (V, 7))
    finally:
        m.free()


def sim3_graph_pcg(edges, fixed, Hdiag, W, b, lam: float, tol: float = DEFAULT_PCG_TOL, max_iter: int = DEFAULT_PCG_MAX_ITER,
                   ctx: Optional[Context] = None):
    """``slam_s3g_pcg_f64``: x [V,7] with (H + lam I) x = -b over the free vertices, and
    dict(iterations, converged, relres, status)."""
    V, e, Hd, Wb, fx = _system_arrays(edges, fixed, Hdiag, W)
    b = np.ascontiguousarray(b, np.float64)
    if b.size != 7 * V:
        raise ValueError(f"b must hold 7 V = {7 * V} values, got {b.size}")
    _check_solver_args(0, 0.0, tol, max_iter)
    if V == 0:
        return np.zeros((0, 7)), dict(iterations=0, converged=True, relres=0.0, status=0)
    ptr, adj = vertex_lists(V, e)
    ctx = ctx or default_context()
    m = _Dev(ctx)
    try:
        de, dp, da, df, dH, dW, db = m.up(e), m.up(ptr), m.up(adj), m.up(fx), m.up(Hd), m.up(Wb), m.up(b)
        dx = m.new(V * 56)
        st = np.zeros(4)
        check(ctx.lib.slam_s3g_pcg_f64(ctx.handle, V, len(e), de.ptr, dp.ptr, da.ptr, df.ptr, dH.ptr, dW.ptr, db.ptr, float(lam), float(tol),
                                       int(max_iter), dx.ptr, addr(st)))
        return dx.download(np.float64, (V, 7)), dict(iterations=int(st[0]), converged=bool(st[1]), relres=float(st[2]), status=int(st[3]))
    finally:
        m.free()


# ---------------------------------------------------------------- building the graph, reading the result ---------------------
def sim3_edges_from_sim3(pairs, models, inlier_counts, min_inliers: int = 20, rotation_sigma: float = 0.01,
                         translation_sigma: float = 0.1, scale_sigma: float = 0.05):
    """7-DoF edges from ``estimate_sim3_batch`` output: ``pairs`` int [B,2] with ``pairs[b] = (i, j)``, ``models =
    (s [B], R [B,3,3], t [B,3])`` with ``X_j = s R X_i + t`` -> (edges int32 [E,2], meas [E,13], info [E,7,7]).

    An edge is emitted for EVERY pair with at least ``min_inliers`` inliers, i != j and a finite positive scale - at any
    scale, which is what ``loop_edges_from_sim3`` cannot do.  The measurement is the model unchanged; the information is
    diagonal, ``inliers / min_inliers / sigma^2`` per block."""
    pairs = _edge_pairs(pairs)
    B = len(pairs)
    if len(models) != 3:
        raise ValueError("models must be (s [B], R [B,3,3], t [B,3])")
    Z = _sims13((np.asarray(models[0], np.float64).reshape(-1), models[1], models[2]), "models")
    n = np.asarray(inlier_counts).reshape(-1)
    if not (len(Z) == len(n) == B):
        raise ValueError(f"{B} pairs but {len(Z)} models and {len(n)} inlier counts")
    _check_edge_args(min_inliers, rotation_sigma, translation_sigma, scale_sigma)
    if B and pairs.min() < 0:
        raise ValueError("negative pair index")
    s = Z[:, 12]
    k = np.flatnonzero((n >= min_inliers) & (pairs[:, 0] != pairs[:, 1]) & np.isfinite(s) & (s > 0))
    return np.ascontiguousarray(pairs[k], np.int32), Z[k].copy(), _edge_info(n[k] / float(min_inliers), rotation_sigma, translation_sigma,
                                                                            scale_sigma)


def lift_se3_graph(poses, edges, meas, info, scale_sigma: float = 0.05):
    """An SE(3) graph (``optimize_pose_graph``'s arguments: poses and measurements [N,12] / [N,3,4] / [N,4,4], info [E,6,6])
    in Sim(3) form: (sims [V,13], edges int32 [E,2], meas [E,13], info [E,7,7]) with every ``s = 1`` and the 6x6
    information in the corner of a 7x7 one that has ``1 / scale_sigma^2`` on sigma."""
    if scale_sigma <= 0:
        raise ValueError("scale_sigma must be positive")
    T, Z, e = _poses12(poses), _poses12(meas, "meas"), _edges_array(edges)
    Om = np.asarray(info, np.float64).reshape(-1, 6, 6)
    if not (len(Z) == len(e) == len(Om)):
        raise ValueError(f"{len(e)} edges but {len(Z)} measurements and {len(Om)} information matrices")
    lift = lambda A: np.concatenate([A, np.ones((len(A), 1))], 1)
    info7 = np.zeros((len(e), 7, 7))
    info7[:, :6, :6] = Om
    info7[:, 6, 6] = 1.0 / scale_sigma ** 2
    return lift(T), e, lift(Z), info7


def sims_to_poses(sims) -> np.ndarray:
    """``[R | t / s]`` [V,3,4]: the metric pose of each keyframe (``X_cam / s = R X_world + t / s``)."""
    s, R, t = split(_sims13(sims))
    return np.concatenate([R, (t / s[:, None])[:, :, None]], 2)


def correct_points(points, ref_keyframe, sims_before, sims_after) -> np.ndarray:
    """ORB-SLAM's map-point correction after the essential-graph step: ``X' = S_after^-1 S_before X`` through each point's
    reference keyframe (``points`` [N,3] world, ``ref_keyframe`` int [N]).  numpy on the host: not a hot path."""
    X = np.asarray(points, np.float64).reshape(-1, 3)
    k = np.asarray(ref_keyframe).reshape(-1)
    if k.dtype.kind not in "iu" or len(k) != len(X):
        raise ValueError("ref_keyframe must be one integer per point")
    sb, Rb, tb = split(_sims13(sims_before, "sims_before"))
    sa, Ra, ta = split(_sims13(sims_after, "sims_after"))
    if len(sb) != len(sa):
        raise ValueError("sims_before and sims_after must describe the same keyframes")
    if len(k) and (k.min() < 0 or k.max() >= len(sb)):
        raise ValueError("ref_keyframe outside [0, V)")
    cam = sb[k, None] * np.einsum("nij,nj->ni", Rb[k], X) + tb[k]
    return np.einsum("nji,nj->ni", Ra[k], cam - ta[k]) / sa[k, None]
