"""SE(3) pose-graph optimisation on the GPU (``slam_pg_*``): what ``pose_graph_sphere_example.py`` does with g2o.

The example reads ``VERTEX_SE3:QUAT`` / ``EDGE_SE3:QUAT`` lines into ``VertexSE3`` / ``EdgeSE3``, fixes vertex 0 and runs 15
Levenberg-Marquardt iterations (``pose_graph_sphere_example.py:7,24-30,45-57``).  Here the graph is arrays and the whole
loop runs in ``slam_pg_optimize_host_f64``: block-sparse 6x6 products and a block-Jacobi PCG in place of g2o's sparse
direct solver.  It is also the consumer of the loop-closure chain: ``KeyframeDatabase`` proposes keyframe pairs,
``verify_pairs`` / ``recover_pose_batch`` turn them into relative motions, ``loop_edges_from_two_view`` turns those
into edges, ``optimize_pose_graph`` corrects the trajectory.

Conventions (``include/slamhip.h``): poses ``T = [R|t]`` with ``X_cam = R X_world + t`` (the project's Tcw), tangent
``[w, v]`` rotation first, update ``T <- Exp(d) T``.  Edge ``(i, j)`` carries ``Z``, a measured ``T_j T_i^-1`` (exactly
``Frontend._relative_motion`` and ``recover_pose_batch``'s ``X2 = R X1 + t``); ``r = Log(T_j T_i^-1 Z^-1)``;
``F = sum rho(r^T Omega r)`` without a factor 1/2; ``Omega`` [6,6] in ``[w, v]`` order.

PARITY UNPINNED against g2o (absent here).  g2o's ``EdgeSE3`` works on ``X = T^-1`` with ``Z_g = Z^-1`` and the error
``[translation, quaternion vector part]`` of ``Z_g^-1 X_i^-1 X_j``, the inverse of our ``T_j T_i^-1 Z^-1``: ``read_g2o``
inverts poses and measurements, permutes the information to rotation first and scales it for ``q ~ w/2``.
There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Tuple

import numpy as np

from ._geometry import _check_edge_args, _edge_info, _edge_pairs
from ._lib import addr, check
from .device import Context, default_context

DEFAULT_ITERATIONS = 15          # pose_graph_sphere_example.py:57
DEFAULT_PCG_TOL = 1e-8
DEFAULT_PCG_MAX_ITER = 500
MAX_VERTICES = 1 << 24
MAX_EDGES = 1 << 25
STATUS_BITS = {1: "index", 2: "angle", 4: "precond", 8: "breakdown", 16: "nonfinite"}
STATS_FIELDS = ("chi2_initial", "chi2_final", "iterations", "trials", "cg_iterations", "lam", "status")


# ---------------------------------------------------------------- argument coercion -----------------------------------------
def _poses12(poses, name="poses") -> np.ndarray:
    """[V,12], [V,3,4] or [V,4,4] -> contiguous float64 [V,12]"""
    a = np.asarray(poses)
    if a.dtype.kind not in "fiu":
        raise ValueError(f"{name} must be numeric, got dtype {a.dtype}")
    a = a.astype(np.float64, copy=False)
    if a.ndim == 2 and a.shape[1] == 12:
        out = a
    elif a.ndim == 3 and a.shape[1:] == (3, 4):
        out = a.reshape(-1, 12)
    elif a.ndim == 3 and a.shape[1:] == (4, 4):
        out = a[:, :3, :].reshape(-1, 12)
    elif a.size == 0:
        out = np.zeros((0, 12))
    else:
        raise ValueError(f"{name} must have shape [V,12], [V,3,4] or [V,4,4], got {a.shape}")
    return np.ascontiguousarray(out)


def _edges_array(edges) -> np.ndarray:
    """integer [E,2] -> contiguous int32 [E,2]; anything else is a ValueError (no silent truncation)"""
    e = np.asarray(edges)
    if e.size == 0:
        e = np.zeros((0, 2), np.int32)
    if e.dtype.kind not in "iu":
        raise ValueError(f"edges must be integers, got dtype {e.dtype}")
    if e.ndim != 2 or e.shape[1] != 2:
        raise ValueError(f"edges must have shape [E,2], got {e.shape}")
    if e.size and (e.max() > 2**31 - 1 or e.min() < -2**31):
        raise ValueError("edge indices do not fit int32")
    return np.ascontiguousarray(e, np.int32)


def _graph_arrays(poses, edges, meas, info, fixed):
    T = _poses12(poses)
    V = len(T)
    e = _edges_array(edges)
    E = len(e)
    Z = _poses12(meas, "meas")
    if len(Z) != E:
        raise ValueError(f"{E} edges but {len(Z)} measurements")
    Om = np.asarray(info)
    if Om.dtype.kind not in "fiu":
        raise ValueError(f"info must be numeric, got dtype {Om.dtype}")
    if Om.size == 0:
        Om = np.zeros((0, 6, 6))
    if Om.shape != (E, 6, 6):
        raise ValueError(f"info must have shape [E,6,6] = ({E}, 6, 6), got {Om.shape}")
    Om = np.ascontiguousarray(Om, np.float64)
    fx = None
    if fixed is not None:
        fx = np.asarray(fixed)
        if fx.shape != (V,):
            raise ValueError(f"fixed must be a mask of shape [V] = ({V},), got {fx.shape}")
        fx = np.ascontiguousarray(fx != 0, np.uint8)
    if V > MAX_VERTICES or E > MAX_EDGES:
        raise ValueError(f"at most {MAX_VERTICES} vertices and {MAX_EDGES} edges")
    return T, e, Z, Om, fx


def vertex_lists(V: int, edges: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """The vertex -> edge lists the device entry points take: (ptr int32 [V+1], adj int32 [2E]); the slots of vertex v hold
    ``2 e + side`` (side 0: v is the edge's first index) in ascending edge order.  Indices outside [0, V) get no slot (the
    device check refuses such a graph)."""
    flat = np.asarray(edges, np.int64).reshape(-1)
    ok = (flat >= 0) & (flat < V)
    a = np.flatnonzero(ok)
    order = np.argsort(flat[a], kind="stable")
    ptr = np.zeros(V + 1, np.int64)
    np.add.at(ptr, flat[a] + 1, 1)
    adj = np.full(len(flat), -1, np.int32)
    adj[:len(a)] = a[order]
    return np.cumsum(ptr).astype(np.int32), adj


def status_names(status: int):
    return [name for bit, name in STATUS_BITS.items() if int(status) & bit]


def plan(V: int, E: int) -> dict:
    """The launch plan for a graph of V vertices and E edges, without a device (``slam_pg_plan``), and the workspace it takes."""
    from . import _lib

    lib = _lib.load()
    p = (ctypes.c_int32 * 8)()
    n = ctypes.c_uint64(0)
    check(lib.slam_pg_plan(int(V), int(E), p))
    check(lib.slam_pg_workspace(int(V), int(E), ctypes.byref(n)))
    names = ("product_blocks", "hub_blocks", "vertices_per_block", "hub_degree", "edge_blocks", "cg_check", "launches_per_cg_iteration")
    out = dict(zip(names, p))
    out["workspace_bytes"] = n.value
    return out


# ---------------------------------------------------------------- the calls ---------------------------------------------------
def _check_solver_args(iterations, huber_delta, pcg_tol, pcg_max_iter):
    if not isinstance(iterations, (int, np.integer)) or isinstance(iterations, bool) or not 0 <= int(iterations) <= 10000:
        raise ValueError("iterations must be an integer in [0, 10000]")
    if not (np.isfinite(huber_delta) and huber_delta >= 0):
        raise ValueError("huber_delta must be >= 0")
    if not (0 < pcg_tol < 1):
        raise ValueError("pcg_tol must be in (0, 1)")
    if not isinstance(pcg_max_iter, (int, np.integer)) or isinstance(pcg_max_iter, bool) or not 1 <= int(pcg_max_iter) <= 1 << 20:
        raise ValueError("pcg_max_iter must be an integer in [1, 2^20]")


def optimize_pose_graph(poses, edges, meas, info, fixed, iterations: int = DEFAULT_ITERATIONS, huber_delta: float = 0.0,
                        pcg_tol: float = DEFAULT_PCG_TOL, pcg_max_iter: int = DEFAULT_PCG_MAX_ITER, ctx: Optional[Context] = None):
    """``optimizer.optimize(15)`` (``pose_graph_sphere_example.py:56-57``) on arrays: poses [V,12] / [V,3,4] / [V,4,4] (Tcw),
    edges int [E,2], meas (the same pose formats, ``T_j T_i^-1``), info [E,6,6], fixed mask [V] (at least one set) ->
    (poses in the input's format, stats dict: chi2_initial, chi2_final, iterations, trials, cg_iterations, lam, status)."""
    T, e, Z, Om, fx = _graph_arrays(poses, edges, meas, info, fixed)
    if fx is None:
        raise ValueError("fixed must be given: a graph needs at least one fixed vertex")
    _check_solver_args(iterations, huber_delta, pcg_tol, pcg_max_iter)
    V, E = len(T), len(e)
    if V and not fx.any():
        raise ValueError("a graph needs at least one fixed vertex (the example fixes vertex 0)")
    out = np.empty_like(T)
    stats = np.zeros(8)
    if V:
        ctx = ctx or default_context()
        check(ctx.lib.slam_pg_optimize_host_f64(ctx.handle, V, E, addr(T), addr(e) if E else None, addr(Z) if E else None,
                                                addr(Om) if E else None, addr(fx), int(iterations), float(huber_delta), float(pcg_tol),
                                                int(pcg_max_iter), addr(out), addr(stats)))
    st = dict(zip(STATS_FIELDS, stats[:7]))
    for k in ("iterations", "trials", "cg_iterations", "status"):
        st[k] = int(st[k])
    src = np.asarray(poses)
    if src.ndim == 3 and src.shape[1:] == (4, 4):
        full = np.array(src, np.float64)
        full[:, :3, :] = out.reshape(-1, 3, 4)
        return full, st
    return (out.reshape(-1, 3, 4) if src.ndim == 3 else out), st


class _Dev:
    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, []

    def up(self, a):
        b = self.ctx.upload(a if a.size else np.zeros(2, a.dtype))
        self.bufs.append(b)
        return b

    def new(self, nbytes):
        b = self.ctx.malloc(max(int(nbytes), 16))
        self.bufs.append(b)
        return b

    def free(self):
        for b in self.bufs:
            b.free()


def pose_graph_linearize(poses, edges, meas, info, huber_delta: float = 0.0, ctx: Optional[Context] = None):
    """``slam_pg_linearize_f64``: (cost, gradient b [V,6], diagonal blocks [V,6,6], edge blocks W_e [E,6,6], status)."""
    T, e, Z, Om, _ = _graph_arrays(poses, edges, meas, info, None)
    V, E = len(T), len(e)
    if V == 0:
        return 0.0, np.zeros((0, 6)), np.zeros((0, 6, 6)), np.zeros((0, 6, 6)), 0
    ptr, adj = vertex_lists(V, e)
    ctx = ctx or default_context()
    m = _Dev(ctx)
    try:
        dT, de, dZ, dO, dp, da = m.up(T), m.up(e), m.up(Z), m.up(Om), m.up(ptr), m.up(adj)
        dc, dg, dH, dW = m.new(8), m.new(V * 48), m.new(V * 288), m.new(E * 288)
        status = ctypes.c_int32(0)
        check(ctx.lib.slam_pg_linearize_f64(ctx.handle, V, E, dT.ptr, de.ptr, dZ.ptr, dO.ptr, dp.ptr, da.ptr, float(huber_delta),
                                            dc.ptr, dg.ptr, dH.ptr, dW.ptr, ctypes.byref(status)))
        cost = float(dc.download(np.float64, (1,))[0])
        W = dW.download(np.float64, (E, 6, 6)) if E else np.zeros((0, 6, 6))
        return cost, dg.download(np.float64, (V, 6)), dH.download(np.float64, (V, 6, 6)), W, int(status.value)
    finally:
        m.free()


def _system_arrays(edges, fixed, Hdiag, W):
    Hd = np.ascontiguousarray(Hdiag, np.float64)
    if Hd.ndim != 3 or Hd.shape[1:] != (6, 6):
        raise ValueError(f"Hdiag must have shape [V,6,6], got {Hd.shape}")
    V = len(Hd)
    e = _edges_array(edges)
    Wb = np.ascontiguousarray(W, np.float64).reshape(-1, 6, 6)
    if len(Wb) != len(e):
        raise ValueError(f"{len(e)} edges but {len(Wb)} edge blocks")
    fx = np.asarray(fixed)
    if fx.shape != (V,):
        raise ValueError(f"fixed must have shape [V] = ({V},), got {fx.shape}")
    return V, e, Hd, Wb, np.ascontiguousarray(fx != 0, np.uint8)


def pose_graph_hmul(edges, fixed, Hdiag, W, lam: float, x, ctx: Optional[Context] = None) -> np.ndarray:
    """``slam_pg_hmul_f64``: y [V,6] = (H + lam I) x over the free vertices, H from ``pose_graph_linearize``'s blocks."""
    V, e, Hd, Wb, fx = _system_arrays(edges, fixed, Hdiag, W)
    x = np.ascontiguousarray(x, np.float64)
    if x.size != 6 * V:
        raise ValueError(f"x must hold 6 V = {6 * V} values, got {x.size}")
    if V == 0:
        return np.zeros((0, 6))
    ptr, adj = vertex_lists(V, e)
    ctx = ctx or default_context()
    m = _Dev(ctx)
    try:
        de, dp, da, df, dH, dW, dx = m.up(e), m.up(ptr), m.up(adj), m.up(fx), m.up(Hd), m.up(Wb), m.up(x)
        dy = m.new(V * 48)
        check(ctx.lib.slam_pg_hmul_f64(ctx.handle, V, len(e), de.ptr, dp.ptr, da.ptr, df.ptr, dH.ptr, dW.ptr, float(lam), dx.ptr, dy.ptr))
        return dy.download(np.float64, (V, 6))
    finally:
        m.free()


def pose_graph_pcg(edges, fixed, Hdiag, W, b, lam: float, tol: float = DEFAULT_PCG_TOL, max_iter: int = DEFAULT_PCG_MAX_ITER,
                   ctx: Optional[Context] = None):
    """``slam_pg_pcg_f64``: x [V,6] with (H + lam I) x = -b over the free vertices, and
    dict(iterations, converged, relres, status)."""
    V, e, Hd, Wb, fx = _system_arrays(edges, fixed, Hdiag, W)
    b = np.ascontiguousarray(b, np.float64)
    if b.size != 6 * V:
        raise ValueError(f"b must hold 6 V = {6 * V} values, got {b.size}")
    _check_solver_args(0, 0.0, tol, max_iter)
    if V == 0:
        return np.zeros((0, 6)), dict(iterations=0, converged=True, relres=0.0, status=0)
    ptr, adj = vertex_lists(V, e)
    ctx = ctx or default_context()
    m = _Dev(ctx)
    try:
        de, dp, da, df, dH, dW, db = m.up(e), m.up(ptr), m.up(adj), m.up(fx), m.up(Hd), m.up(Wb), m.up(b)
        dx = m.new(V * 48)
        st = np.zeros(4)
        check(ctx.lib.slam_pg_pcg_f64(ctx.handle, V, len(e), de.ptr, dp.ptr, da.ptr, df.ptr, dH.ptr, dW.ptr, db.ptr, float(lam), float(tol),
                                      int(max_iter), dx.ptr, addr(st)))
        return dx.download(np.float64, (V, 6)), dict(iterations=int(st[0]), converged=bool(st[1]), relres=float(st[2]), status=int(st[3]))
    finally:
        m.free()


# ---------------------------------------------------------------- loop closures -> edges -------------------------------------
def loop_edges_from_two_view(pairs, R, t, inlier_counts, min_inliers: int = 20, rotation_sigma: float = 0.01, scale=None,
                             translation_sigma: float = 0.1):
    """Edges from ``verify_pairs`` / ``recover_pose_batch`` output: ``pairs`` int [B,2] (keyframe i of view 1, keyframe j of
    view 2), ``R`` [B,3,3], ``t`` [B,3] with ``X2 = R X1 + t``, ``inlier_counts`` [B] -> (edges int32 [E,2], meas [E,3,4],
    info [E,6,6]) for the pairs with at least ``min_inliers`` inliers.

    The rotation block of the information is ``inliers / min_inliers / rotation_sigma^2`` times the identity.  A two-view
    translation has unit length - its scale is unknown - so the translation block is ZERO unless ``scale`` (a number or one
    per pair: the metric length of each translation) is given; then ``t`` is multiplied by it and the block is
    ``1 / translation_sigma^2``.  With zero translation information an edge constrains the relative rotation only."""
    pairs = _edge_pairs(pairs)
    B = len(pairs)
    R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    t = np.asarray(t, np.float64).reshape(-1, 3)
    n = np.asarray(inlier_counts).reshape(-1)
    if not (len(R) == len(t) == len(n) == B):
        raise ValueError(f"{B} pairs but {len(R)} rotations, {len(t)} translations, {len(n)} inlier counts")
    _check_edge_args(min_inliers, rotation_sigma, translation_sigma)
    s = None
    if scale is not None:
        s = np.broadcast_to(np.asarray(scale, np.float64), (B,))
        if not (np.isfinite(s).all() and (s > 0).all()):
            raise ValueError("scale must be positive")
    keep = (n >= min_inliers) & (pairs[:, 0] != pairs[:, 1])
    k = np.flatnonzero(keep)
    meas = np.zeros((len(k), 3, 4))
    meas[:, :, :3] = R[k]
    meas[:, :, 3] = t[k] * (s[k, None] if s is not None else 1.0)
    info = _edge_info(n[k] / float(min_inliers), rotation_sigma, None)
    if s is not None:                                   # the one block that is not weighted by the inliers
        info[:, [3, 4, 5], [3, 4, 5]] = 1.0 / translation_sigma ** 2
    return np.ascontiguousarray(pairs[k], np.int32), meas, info


# ---------------------------------------------------------------- g2o text -----------------------------------------------------
def _quat_to_rot(q):
    """[x, y, z, w] (normalised here) -> R"""
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _rot_to_quat(R):
    """R -> [x, y, z, w] with w >= 0 (Shepperd's choice of the largest pivot)"""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    cand = [tr, R[0, 0], R[1, 1], R[2, 2]]
    i = int(np.argmax(cand))
    if i == 0:
        w = 0.5 * np.sqrt(1 + tr)
        q = [(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w]
    else:
        a = i - 1
        b, c = (a + 1) % 3, (a + 2) % 3
        s = 0.5 * np.sqrt(1 + R[a, a] - R[b, b] - R[c, c])
        q = [0.0, 0.0, 0.0, (R[c, b] - R[b, c]) / (4 * s)]
        q[a], q[b], q[c] = s, (R[b, a] + R[a, b]) / (4 * s), (R[c, a] + R[a, c]) / (4 * s)
    q = np.asarray(q)
    return -q if q[3] < 0 else q


def _invert34(T):
    Rt = T[:3, :3].T
    return np.concatenate([Rt, -(Rt @ T[:3, 3:])], 1)


# g2o's EdgeSE3 error is [translation (3), quaternion vector part (3)]; ours [w (3), v (3)] with q ~ w / 2
_PERM = np.array([3, 4, 5, 0, 1, 2])
_SCALE = np.array([0.5, 0.5, 0.5, 1.0, 1.0, 1.0])


def _info_from_g2o(upper21):
    M = np.zeros((6, 6))
    M[np.triu_indices(6)] = upper21
    M = M + np.triu(M, 1).T
    return M[np.ix_(_PERM, _PERM)] * np.outer(_SCALE, _SCALE)


def _info_to_g2o(info):
    inv_perm = np.argsort(_PERM)
    M = (np.asarray(info, np.float64) / np.outer(_SCALE, _SCALE))[np.ix_(inv_perm, inv_perm)]
    return M[np.triu_indices(6)]


def read_g2o(path_or_text):
    """``VERTEX_SE3:QUAT`` and ``EDGE_SE3:QUAT`` records (the two the example reads, ``pose_graph_sphere_example.py:17,33``)
    from a file (an ``os.PathLike``, or a ``str`` without a line break) or from the text itself (a ``str`` with at least one
    line break) -> dict(ids int64 [V], poses [V,3,4], edges int32 [E,2] (indices into ids),
    meas [E,3,4], info [E,6,6]) in THIS project's conventions: a g2o vertex is a camera-to-world pose X and the project's
    pose is ``T = X^-1``; an edge measurement ``Z_g ~ X_i^-1 X_j`` becomes ``Z = Z_g^-1 ~ T_j T_i^-1``; the 21 upper-triangular
    information values (translation first, then the quaternion's vector part) are permuted to rotation first and scaled for
    ``q ~ w/2``: ``Omega_ww = Omega_qq / 4``, ``Omega_wv = Omega_qv / 2``.  Other record types are skipped."""
    if isinstance(path_or_text, os.PathLike) or (isinstance(path_or_text, str) and "\n" not in path_or_text):
        with open(path_or_text, encoding="utf-8") as f:      # a str without a line break is a path: a wrong one raises
            text = f.read()
    elif isinstance(path_or_text, str):
        text = path_or_text
    else:
        raise TypeError(f"read_g2o takes a path or the text, got {type(path_or_text).__name__}")
    ids, poses, raw_edges, meas, info = [], [], [], [], []
    for ln, line in enumerate(text.splitlines(), 1):
        arr = line.split()
        if not arr:
            continue
        if arr[0] == "VERTEX_SE3:QUAT":
            if len(arr) != 9:
                raise ValueError(f"line {ln}: VERTEX_SE3:QUAT takes id x y z qx qy qz qw")
            v = np.array(arr[2:], np.float64)
            X = np.concatenate([_quat_to_rot(v[3:]), v[:3, None]], 1)
            ids.append(int(arr[1]))
            poses.append(_invert34(X))
        elif arr[0] == "EDGE_SE3:QUAT":
            if len(arr) != 31:
                raise ValueError(f"line {ln}: EDGE_SE3:QUAT takes i j x y z qx qy qz qw and 21 information values")
            v = np.array(arr[3:], np.float64)
            Zg = np.concatenate([_quat_to_rot(v[3:7]), v[:3, None]], 1)
            raw_edges.append((int(arr[1]), int(arr[2])))
            meas.append(_invert34(Zg))
            info.append(_info_from_g2o(v[7:]))
    ids = np.asarray(ids, np.int64)
    if len(set(ids.tolist())) != len(ids):
        raise ValueError("a vertex id appears twice")
    index = {int(v): k for k, v in enumerate(ids)}
    try:
        edges = np.array([(index[i], index[j]) for i, j in raw_edges], np.int32).reshape(-1, 2)
    except KeyError as exc:
        raise ValueError(f"an edge names vertex {exc.args[0]}, which the file does not define") from None
    return dict(ids=ids, poses=np.array(poses).reshape(-1, 3, 4), edges=edges, meas=np.array(meas).reshape(-1, 3, 4),
                info=np.array(info).reshape(-1, 6, 6))


def write_g2o(poses, edges, meas, info, ids=None, path=None) -> str:
    """The inverse of ``read_g2o``: the text (also written to ``path`` if given), 17 significant digits."""
    T, e, Z, Om, _ = _graph_arrays(poses, edges, meas, info, None)
    ids = np.arange(len(T)) if ids is None else np.asarray(ids, np.int64)
    if len(ids) != len(T):
        raise ValueError("one id per pose")
    fmt = lambda vals: " ".join(repr(float(v)) for v in vals)
    lines = []
    for k, Tk in enumerate(T.reshape(-1, 3, 4)):
        X = _invert34(Tk)
        lines.append(f"VERTEX_SE3:QUAT {int(ids[k])} {fmt(X[:, 3])} {fmt(_rot_to_quat(X[:, :3]))}")
    for (i, j), Zk, Ok in zip(e, Z.reshape(-1, 3, 4), Om):
        Zg = _invert34(Zk)
        lines.append(f"EDGE_SE3:QUAT {int(ids[i])} {int(ids[j])} {fmt(Zg[:, 3])} {fmt(_rot_to_quat(Zg[:, :3]))} {fmt(_info_to_g2o(Ok))}")
    text = "\n".join(lines) + "\n"
    if path is not None:
        with open(path, "w", encoding="utf-8") as f:
            f.write(text)
    return text
