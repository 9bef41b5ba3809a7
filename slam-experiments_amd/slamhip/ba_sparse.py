"""Sparse bundle adjustment (``slam_bas_*``): the bundle adjustment that follows a closed loop.

``bundle_adjust_device`` forms the reduced camera system densely - a [K,L] lookup table, [K,K,36] blocks, a 6K x 6K host
solve - which holds a keyframe window.  Here the system exists only over the covisibility graph: one 6x6 block per pair of
free poses that see a common point, built on the device in the layout of the pose-graph solver and solved by it
(``slam_pg_pcg_f64``: block-Jacobi PCG with hub handling, fixed summation order, status bits).  Conventions, residuals,
Huber weight and the Levenberg-Marquardt schedule are those of ``bundle_adjust_device``.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np

from ._lib import addr, check, load
from .ba import BAResult, fixed_pose_mask, lm_schedule, observation_lists, state_arrays
from .device import Context, default_context
from .pose_graph import DEFAULT_PCG_MAX_ITER, MAX_EDGES, MAX_VERTICES, _check_solver_args, vertex_lists

DEFAULT_PCG_TOL = 1e-10           # 1e-8, the pose graph's default, leaves the poses 1e-7 from a direct solve: outside the BA suite's bar
MAX_POINTS = 1 << 28
MAX_OBS = 1 << 28
MAX_PAIRS = 1 << 30


def _index_arrays(obs_pose, obs_point, K: int, L: Optional[int]):
    op, ol = np.asarray(obs_pose), np.asarray(obs_point)
    if op.size == 0:
        op = np.zeros(0, np.int32)
    if ol.size == 0:
        ol = np.zeros(0, np.int32)
    if op.dtype.kind not in "iu" or ol.dtype.kind not in "iu":
        raise ValueError("observation indices must be integers")
    op, ol = op.reshape(-1), ol.reshape(-1)
    if len(op) != len(ol):
        raise ValueError("obs_pose and obs_point must have one entry per observation")
    if len(op) > MAX_OBS:
        raise ValueError(f"at most {MAX_OBS} observations")
    if not 1 <= K <= MAX_VERTICES:
        raise ValueError(f"K must be in [1, {MAX_VERTICES}]")
    if len(op) and (op.min() < 0 or op.max() >= K or ol.min() < 0 or (L is not None and ol.max() >= L) or ol.max() >= MAX_POINTS):
        raise ValueError("observation index out of range")
    return np.ascontiguousarray(op, np.int32), np.ascontiguousarray(ol, np.int32)


def _fixed_mask(fixed, K: int) -> np.ndarray:
    fx = np.asarray(fixed)
    if fx.shape != (K,):
        raise ValueError(f"fixed must be a mask of shape [K] = ({K},), got {fx.shape}")
    fx = fx != 0
    if not fx.any():
        raise ValueError("a bundle adjustment needs at least one fixed pose (the gauge)")
    return fx


def covisibility(obs_pose, obs_point, K: int, fixed, L: Optional[int] = None):
    """The covisibility graph of the free poses and the pair lists the device sums over.

    ``obs_pose`` / ``obs_point`` int [O]; ``fixed`` a mask [K] (at least one set); ``L`` the number of points when known.
    Returns ``(edges, weights, pair_ptr, pair_a, pair_b)``: ``edges`` int32 [E,2] with k1 < k2, every pair of free poses
    that observe a common point, ascending by (k1, k2); ``weights`` int32 [E], the number of common points (ORB-SLAM's
    covisibility weight); for edge e the slots [pair_ptr[e], pair_ptr[e+1]) of ``pair_a`` / ``pair_b`` (int32 [P]) hold the
    observation indices of (k1, l) and (k2, l) for every common point l, ascending in l - the order the device sums in.
    Raises ``ValueError`` for an index out of range, a (pose, point) pair observed twice, no fixed pose, or more pairs or
    edges than the device takes."""
    op, ol = _index_arrays(obs_pose, obs_point, int(K), L)
    K = int(K)
    fx = _fixed_mask(fixed, K)
    key = ol.astype(np.int64) * K + op
    order = np.argsort(key, kind="stable")                    # by point, then pose
    ks = key[order]
    if len(ks) > 1 and (ks[1:] == ks[:-1]).any():
        raise ValueError("a (pose, point) pair is observed more than once")
    oidx = order[~fx[op[order]]]                              # the observations of free poses, by (point, pose)
    lo = ol[oidx]
    starts = np.flatnonzero(np.r_[True, lo[1:] != lo[:-1]]) if len(lo) else np.zeros(0, np.int64)
    counts = np.diff(np.r_[starts, len(lo)])
    lengths = [int(n) for n in np.unique(counts) if n >= 2]
    total = sum(int((counts == n).sum()) * (n * (n - 1) // 2) for n in lengths)
    if total > MAX_PAIRS:
        raise ValueError(f"{total} covisible pairs: more than the {MAX_PAIRS} the device takes")
    pa, pb = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for n in lengths:                                         # one pass per track length, every point of that length at once
        rows = oidx[starts[counts == n][:, None] + np.arange(n)[None, :]]
        i, j = np.triu_indices(n, 1)
        pa.append(rows[:, i].reshape(-1))
        pb.append(rows[:, j].reshape(-1))
    pa, pb = np.concatenate(pa), np.concatenate(pb)
    k1, k2 = op[pa].astype(np.int64), op[pb].astype(np.int64)
    ek, lp = k1 * K + k2, ol[pa].astype(np.int64)
    span = int(lp.max()) + 1 if len(lp) else 1
    # (k1, k2, l) names a pair once, so ONE key sorts them and no two keys tie; three keys only where one would overflow
    order = np.argsort(ek * span + lp) if K * K * span < 2 ** 62 else np.lexsort((lp, k2, k1))
    pa, pb, ek = pa[order], pb[order], ek[order]
    first = np.flatnonzero(np.r_[True, ek[1:] != ek[:-1]]) if len(ek) else np.zeros(0, np.int64)
    E = len(first)
    if E > MAX_EDGES:
        raise ValueError(f"{E} covisibility edges: more than the {MAX_EDGES} the solver takes")
    edges = np.stack([ek[first] // K, ek[first] % K], 1).astype(np.int32).reshape(-1, 2)
    pair_ptr = np.r_[first, len(ek)].astype(np.int32)
    return edges, np.diff(pair_ptr).astype(np.int32), pair_ptr, pa.astype(np.int32), pb.astype(np.int32)


def _deltas(huber_delta):
    """(delta_mono, delta_stereo) of a Huber width given as one number (both kinds) or as a pair."""
    d = np.asarray(huber_delta, np.float64).reshape(-1)
    if d.size not in (1, 2) or not (np.isfinite(d).all() and (d >= 0).all()):
        raise ValueError("huber_delta must be a number >= 0, or a pair (mono, stereo) of them")
    return float(d[0]), float(d[-1])


def _stereo_arrays(stereo, O: int):
    """(meas3 [O,3], info [O], bf) of a ``StereoEdges`` for O observations, checked."""
    meas3 = np.ascontiguousarray(stereo.meas3, np.float64)
    info = np.ascontiguousarray(stereo.info, np.float64)
    if meas3.shape != (O, 3) or info.shape != (O,):
        raise ValueError(f"stereo edges must hold meas3 [O,3] and info [O] for O = {O} observations, got {meas3.shape} and {info.shape}")
    if not (np.isfinite(info).all() and (info >= 0).all()):
        raise ValueError("info must be finite and >= 0")
    if not np.isfinite(meas3[:, :2]).all() or np.isinf(meas3[:, 2]).any():
        raise ValueError("meas3 must be finite (mr: finite, or NaN for a monocular edge)")
    bf = float(stereo.bf)
    if not (np.isfinite(bf) and bf > 0):
        raise ValueError("bf must be positive and finite")
    return meas3, info, bf


def _covisibility_host(op, ol, K, fixed, L):
    """``covisibility`` for SparseBAProblem, which has an argument of the function's name (looked up at the call, as before)."""
    return covisibility(op, ol, K, fixed, L)


def workspace_bytes(K: int, L: int, O: int, E: int, P: int) -> int:
    """Device memory one problem takes in all (``slam_bas_workspace``); needs no device."""
    n = ctypes.c_uint64(0)
    check(load().slam_bas_workspace(int(K), int(L), int(O), int(E), int(P), ctypes.byref(n)))
    return n.value


def plan(K: int, L: int, O: int, E: int, P: int) -> dict:
    """The launch plan (``slam_bas_plan``) and the memory it takes; needs no device."""
    p = (ctypes.c_int32 * 8)()
    check(load().slam_bas_plan(int(K), int(L), int(O), int(E), int(P), p))
    names = ("obs_blocks", "point_blocks", "pose_blocks", "edge_blocks", "candidate_blocks", "threads", "lanes_per_edge")
    out = dict(zip(names, p))
    out["workspace_bytes"] = workspace_bytes(K, L, O, E, P)
    return out


class SparseBAProblem:
    """Device-resident state, index tables, blocks and solver buffers of one sparse bundle adjustment.  The arguments are
    checked on the host (``ValueError``) before anything is allocated or launched.  With ``covisibility="device"`` the
    covisibility tables are built by ``slam_covis_*`` from the uploaded observation lists instead of by ``covisibility`` (the
    same tables, bit for bit); a (pose, point) pair observed twice is then refused after that build's count phase, with
    everything freed.  With ``stereo`` (a ``StereoEdges``: meas3 [O,3], info [O], bf) the phases that read a measurement take
    their stereo / weighted forms (``slam_bas_*_stereo_f64``; ``meas`` may then be None) and ``classify`` / ``set_info`` serve
    the outlier schedule of ``local_bundle_adjust``; with ``None`` every call is the one it was."""

    def __init__(self, ctx: Context, K: int, L: int, obs_pose, obs_point, meas, intrinsics, fixed, covisibility: str = "host",
                 stereo=None):
        self._check = check
        self.ctx = ctx
        K, L = int(K), int(L)
        if not 1 <= L <= MAX_POINTS:
            raise ValueError(f"L must be in [1, {MAX_POINTS}]")
        if covisibility not in ("host", "device"):
            raise ValueError(f"covisibility must be 'host' or 'device', got {covisibility!r}")
        op, ol = _index_arrays(obs_pose, obs_point, K, L)
        O = len(op)
        self.stereo = stereo is not None
        if self.stereo:
            meas3, info, self.bf = _stereo_arrays(stereo, O)
            meas = meas3[:, :2] if meas is None else meas
        meas = np.ascontiguousarray(meas, np.float64).reshape(-1, 2)
        if meas.shape[0] != O:
            raise ValueError("obs_pose, obs_point and meas must have one row per observation")
        self.fixed = _fixed_mask(fixed, K)
        pad = lambda a: a if a.size else np.zeros(4, a.dtype)
        up, new = ctx.upload, ctx.malloc
        if covisibility == "device":
            self._device_covisibility(ctx, op, ol, K, L, pad)      # the pair tables never leave the device (slamhip.covis)
        else:
            self.edges, self.weights, pair_ptr, pair_a, pair_b = _covisibility_host(op, ol, K, self.fixed, L)
            self.P = len(pair_a)
        self.K, self.L, self.O, self.E = K, L, O, len(self.edges)
        self.fx, self.fy, self.cx, self.cy = (float(v) for v in intrinsics)
        pt_ptr, pt_obs, ps_ptr, ps_obs = observation_lists(op, ol, K, L)
        vtx_ptr, vtx_adj = vertex_lists(K, self.edges)
        o, e = max(O, 1), max(self.E, 1)
        if covisibility == "host":
            self.d_op, self.d_ol, self.d_fixed = up(pad(op)), up(pad(ol)), up(self.fixed.astype(np.uint8))
            self.d_edges, self.d_pair_ptr, self.d_pair_a, self.d_pair_b = up(pad(self.edges)), up(pair_ptr), up(pad(pair_a)), up(pad(pair_b))
        self.d_meas = up(meas if O else np.zeros((1, 2)))
        if self.stereo:
            self.d_meas3, self.d_info = up(meas3 if O else np.zeros((1, 3))), up(info if O else np.zeros(1))
        self.d_pt_ptr, self.d_pt_obs, self.d_ps_ptr, self.d_ps_obs = up(pt_ptr), up(pad(pt_obs)), up(ps_ptr), up(pad(ps_obs))
        self.d_vtx_ptr, self.d_vtx_adj = up(vtx_ptr), up(pad(vtx_adj))
        self.d_T, self.d_X = [new(K * 96), new(K * 96)], [new(L * 24), new(L * 24)]      # [0] the state, [1] the candidate
        self.d_Hpl, self.d_Hll, self.d_bl, self.d_E, self.d_Ebl = new(o * 144), new(L * 48), new(L * 24), new(L * 72), new(L * 24)
        self.d_Hpp, self.d_bp, self.d_cost, self.d_cost2 = new(K * 168), new(K * 48), new(K * 8), new(K * 8)
        self.d_Hdiag, self.d_W, self.d_b, self.d_dp, self.d_dl = new(K * 288), new(e * 288), new(K * 48), new(K * 48), new(L * 24)
        self.d_part, self.d_scal = new(1024 * 8), new(64)       # scalars: cost, largest diagonal, gain-ratio denominator, candidate cost

    def _device_covisibility(self, ctx: Context, op, ol, K: int, L: int, pad) -> None:
        """The observation tables go up first and ``slam_covis_*`` builds edges, weights and pair tables from them: the problem
        adopts the resident buffers, only ``edges`` and ``weights`` come down."""
        from .covis import build_tables

        self.d_op, self.d_ol, self.d_fixed = ctx.upload(pad(op)), ctx.upload(pad(ol)), ctx.upload(self.fixed.astype(np.uint8))
        try:
            tab = build_tables(ctx, self.d_op, self.d_ol, self.d_fixed, K, L, len(op))
        except BaseException:
            self.free()
            raise
        self.edges, self.weights, self.P = tab.edges, tab.weights, tab.P
        for name, buf in tab.release().items():
            setattr(self, name, buf)

    def _buffers(self):
        for name, b in list(vars(self).items()):
            if name.startswith("d_") and b is not None:
                for x in (b if isinstance(b, list) else [b]):
                    yield name, x

    def free(self) -> None:
        for name, b in self._buffers():
            b.free()
        for name in [n for n in vars(self) if n.startswith("d_")]:
            setattr(self, name, None)

    # ---- state ------------------------------------------------------------------------------------------------------------
    def set_state(self, poses12, points) -> None:
        self.d_T[0].upload(np.ascontiguousarray(poses12, np.float64).reshape(self.K, 12))
        self.d_X[0].upload(np.ascontiguousarray(points, np.float64).reshape(self.L, 3))

    def state(self):
        return self.d_T[0].download(np.float64, (self.K, 12)), self.d_X[0].download(np.float64, (self.L, 3))

    def accept(self) -> None:
        """The candidate becomes the state (the two buffers change places)."""
        self.d_T.reverse()
        self.d_X.reverse()

    # ---- the phases ---------------------------------------------------------------------------------------------------------
    def linearize(self, huber_delta: float):
        """``slam_bas_linearize_f64`` at the state -> (cost, largest diagonal entry of the free Hpp and every Hll)."""
        c = self.ctx
        if self.stereo:
            self._check(c.lib.slam_bas_linearize_stereo_f64(
                c.handle, self.K, self.L, self.O, self.d_T[0].ptr, self.d_X[0].ptr, self.d_op.ptr, self.d_ol.ptr, self.d_meas3.ptr,
                self.d_info.ptr, self.d_pt_ptr.ptr, self.d_pt_obs.ptr, self.d_ps_ptr.ptr, self.d_ps_obs.ptr, self.d_fixed.ptr, self.fx,
                self.fy, self.cx, self.cy, self.bf, *_deltas(huber_delta), self.d_Hpl.ptr, self.d_Hll.ptr, self.d_bl.ptr, self.d_Hpp.ptr,
                self.d_bp.ptr, self.d_cost.ptr, self.d_scal.ptr))
            s = self.d_scal.download(np.float64, (2,))
            return float(s[0]), float(s[1])
        self._check(c.lib.slam_bas_linearize_f64(
            c.handle, self.K, self.L, self.O, self.d_T[0].ptr, self.d_X[0].ptr, self.d_op.ptr, self.d_ol.ptr, self.d_meas.ptr,
            self.d_pt_ptr.ptr, self.d_pt_obs.ptr, self.d_ps_ptr.ptr, self.d_ps_obs.ptr, self.d_fixed.ptr, self.fx, self.fy, self.cx,
            self.cy, float(huber_delta), self.d_Hpl.ptr, self.d_Hll.ptr, self.d_bl.ptr, self.d_Hpp.ptr, self.d_bp.ptr, self.d_cost.ptr,
            self.d_scal.ptr))
        s = self.d_scal.download(np.float64, (2,))
        return float(s[0]), float(s[1])

    def reduce(self, lam: float) -> None:
        """``slam_bas_reduce_f64``: E, Hdiag, W, b at damping ``lam`` from the blocks of the last ``linearize``."""
        c = self.ctx
        self._check(c.lib.slam_bas_reduce_f64(
            c.handle, self.K, self.L, self.O, self.E, self.P, self.d_ol.ptr, self.d_pt_ptr.ptr, self.d_ps_ptr.ptr, self.d_ps_obs.ptr,
            self.d_pair_ptr.ptr, self.d_pair_a.ptr, self.d_pair_b.ptr, self.d_Hpl.ptr, self.d_Hll.ptr, self.d_bl.ptr, self.d_Hpp.ptr,
            self.d_bp.ptr, float(lam), self.d_E.ptr, self.d_Ebl.ptr, self.d_Hdiag.ptr, self.d_W.ptr, self.d_b.ptr))

    def reduced_system(self):
        """The blocks of the last ``reduce`` on the host: (Hdiag [K,6,6], W [E,6,6], b [K,6])."""
        return (self.d_Hdiag.download(np.float64, (self.K, 6, 6)), self.d_W.download(np.float64, (self.E, 6, 6)),
                self.d_b.download(np.float64, (self.K, 6)))

    def solve(self, lam: float, tol: float, max_iter: int) -> dict:
        """``slam_pg_pcg_f64`` on the blocks of the last ``reduce``: (S + lam I) dp = -b into the step buffer."""
        c = self.ctx
        st = np.zeros(4)
        self._check(c.lib.slam_pg_pcg_f64(c.handle, self.K, self.E, self.d_edges.ptr, self.d_vtx_ptr.ptr, self.d_vtx_adj.ptr, self.d_fixed.ptr,
                                          self.d_Hdiag.ptr, self.d_W.ptr, self.d_b.ptr, float(lam), float(tol), int(max_iter), self.d_dp.ptr,
                                          addr(st)))
        return dict(iterations=int(st[0]), converged=bool(st[1]), relres=float(st[2]), status=int(st[3]))

    def hmul(self, lam: float, x) -> np.ndarray:
        """``slam_pg_hmul_f64`` on the blocks of the last ``reduce``: (S + lam I) x over the free poses, [K,6]."""
        c = self.ctx
        dx, dy = c.upload(np.ascontiguousarray(x, np.float64).reshape(self.K, 6)), c.malloc(self.K * 48)
        try:
            self._check(c.lib.slam_pg_hmul_f64(c.handle, self.K, self.E, self.d_edges.ptr, self.d_vtx_ptr.ptr, self.d_vtx_adj.ptr,
                                               self.d_fixed.ptr, self.d_Hdiag.ptr, self.d_W.ptr, float(lam), dx.ptr, dy.ptr))
            return dy.download(np.float64, (self.K, 6))
        finally:
            dx.free()
            dy.free()

    def step(self, lam: float, huber_delta: float):
        """Back-substitution, the candidate state and its cost -> (gain-ratio denominator, cost at the candidate)."""
        c = self.ctx
        self._check(c.lib.slam_bas_backsub_f64(c.handle, self.K, self.L, self.O, self.d_pt_ptr.ptr, self.d_pt_obs.ptr, self.d_op.ptr,
                                               self.d_Hpl.ptr, self.d_E.ptr, self.d_bl.ptr, self.d_dp.ptr, self.d_dl.ptr))
        self._check(c.lib.slam_bas_candidate_f64(c.handle, self.K, self.L, self.d_fixed.ptr, self.d_T[0].ptr, self.d_X[0].ptr, self.d_dp.ptr,
                                                 self.d_dl.ptr, self.d_bp.ptr, self.d_bl.ptr, float(lam), self.d_T[1].ptr, self.d_X[1].ptr,
                                                 self.d_part.ptr, self.d_scal.view(16, 8).ptr))
        if self.stereo:
            self._check(c.lib.slam_bas_cost_stereo_f64(c.handle, self.K, self.L, self.O, self.d_T[1].ptr, self.d_X[1].ptr, self.d_op.ptr,
                                                       self.d_ol.ptr, self.d_meas3.ptr, self.d_info.ptr, self.d_ps_ptr.ptr, self.d_ps_obs.ptr,
                                                       self.fx, self.fy, self.cx, self.cy, self.bf, *_deltas(huber_delta), self.d_cost2.ptr,
                                                       self.d_scal.view(24, 8).ptr))
        else:
            self._check(c.lib.slam_bas_cost_f64(c.handle, self.K, self.L, self.O, self.d_T[1].ptr, self.d_X[1].ptr, self.d_op.ptr, self.d_ol.ptr,
                                                self.d_meas.ptr, self.d_ps_ptr.ptr, self.d_ps_obs.ptr, self.fx, self.fy, self.cx, self.cy,
                                                float(huber_delta), self.d_cost2.ptr, self.d_scal.view(24, 8).ptr))
        s = self.d_scal.download(np.float64, (4,))
        return float(s[2]), float(s[3])

    # ---- the stereo / weighted problem only ---------------------------------------------------------------------------------------
    def classify(self, chi2_mono: float, chi2_stereo: float):
        """``slam_bas_classify_stereo_f64`` at the state -> (weighted chi2 [O], inlier bool [O])."""
        if not self.stereo:
            raise ValueError("classify needs a problem built with stereo edges")
        if not (chi2_mono >= 0 and chi2_stereo >= 0):
            raise ValueError("the gates must not be negative")
        c, o = self.ctx, max(self.O, 1)
        d_chi, d_in = c.malloc(o * 8), c.malloc(o)
        try:
            self._check(c.lib.slam_bas_classify_stereo_f64(c.handle, self.K, self.L, self.O, self.d_T[0].ptr, self.d_X[0].ptr, self.d_op.ptr,
                                                           self.d_ol.ptr, self.d_meas3.ptr, self.d_info.ptr, self.fx, self.fy, self.cx, self.cy,
                                                           self.bf, float(chi2_mono), float(chi2_stereo), d_chi.ptr, d_in.ptr))
            return d_chi.download(np.float64, (o,))[:self.O], d_in.download(np.uint8, (o,))[:self.O].astype(bool)
        finally:
            d_chi.free()
            d_in.free()

    def set_info(self, info) -> None:
        """Replace the informations in the device table (0 switches an edge off); tables and blocks stay as they are."""
        if not self.stereo:
            raise ValueError("set_info needs a problem built with stereo edges")
        info = np.ascontiguousarray(info, np.float64)
        if info.shape != (self.O,) or not (np.isfinite(info).all() and (info >= 0).all()):
            raise ValueError("info must be [O], finite and >= 0")
        if self.O:
            self.d_info.upload(info)


def bundle_adjust_sparse(poses, points, obs_pose_idx, obs_point_idx, meas, intrinsics, iterations: int = 10,
                         fixed_poses: Sequence[int] = (0,), huber_delta: float = 0.0, pcg_tol: float = DEFAULT_PCG_TOL,
                         pcg_max_iter: int = DEFAULT_PCG_MAX_ITER, ctx: Optional[Context] = None, on_trial=None,
                         covisibility: str = "host", stereo=None):
    """``bundle_adjust_device`` for maps instead of windows: the reduced camera system as 6x6 blocks over the covisibility
    graph (``slam_bas_*``), solved by the pose-graph PCG (``slam_pg_pcg_f64``).  Same arguments, same Levenberg-Marquardt
    schedule; the state goes to the device once and comes back once, a trial moves a few scalars.

    Returns ``(BAResult, stats)`` with stats = dict(trials, cg_iterations, lam, status (the OR of the solves'
    ``SLAM_PG_STATUS_*`` bits), unconverged (solves that stopped at ``pcg_max_iter`` or broke down: each counted as a failed
    trial, the damping grows), edges, pairs).  ``on_trial(dict)`` is called after every trial (timing tools).
    ``covisibility``: "host" builds the covisibility tables with numpy (``covisibility``), "device" with ``slam_covis_*``
    (``slamhip.covis``); the tables, and with them every result, are the same bit for bit.
    ``stereo`` (a ``slamhip.StereoEdges``: meas3 [O,3] with mr NaN for a monocular edge, info [O], bf): the stereo / level-weighted
    edge model of DESIGN.md 4v under the same schedule; ``meas`` may then be None and ``huber_delta`` a pair (mono, stereo).
    ``None`` takes the path it took, call for call.
    Raises ``ValueError`` for an index out of range, a (pose, point) pair observed twice or no fixed pose, before any launch."""
    T12, X, K, L = state_arrays(poses, points)
    if stereo is None:
        _check_solver_args(iterations, huber_delta, pcg_tol, pcg_max_iter)
    else:
        _check_solver_args(iterations, min(_deltas(huber_delta)), pcg_tol, pcg_max_iter)
    fixed = fixed_pose_mask(fixed_poses, K)
    ctx = ctx or default_context()
    prob = SparseBAProblem(ctx, K, L, obs_pose_idx, obs_point_idx, meas, intrinsics, fixed, covisibility, stereo)
    st = dict(trials=0, cg_iterations=0, lam=0.0, status=0, unconverged=0, edges=prob.E, pairs=prob.P)

    def trial(lam, cost):
        nonlocal cg
        st["trials"] += 1
        prob.reduce(lam)
        cg = prob.solve(lam, pcg_tol, pcg_max_iter)
        st["cg_iterations"] += cg["iterations"]
        st["status"] |= cg["status"]
        if not cg["converged"]:
            st["unconverged"] += 1                            # never accepted: the damping grows and the trial is reported
            return cost, np.nan, np.nan
        denominator, new = prob.step(lam, huber_delta)
        return cost, new, denominator

    def accept(it):
        prob.accept()
        if it + 1 < int(iterations):
            prob.linearize(huber_delta)

    report = on_trial and (lambda it, lam, cost, new, rho, ok:
                           on_trial(dict(iteration=it, lam=lam, cg=cg, cost=cost, new=new, rho=rho, accepted=ok)))

    try:
        prob.set_state(T12, X)
        cg, (cost0, dmax) = None, prob.linearize(huber_delta)
        cost, st["lam"], accepted = lm_schedule(iterations, cost0, dmax, trial, accept, report)
        Tout, Xout = prob.state()
    finally:
        prob.free()
    Tr = np.tile(np.eye(4), (K, 1, 1))
    Tr[:, :3, :4] = Tout.reshape(K, 3, 4)
    return BAResult(poses=Tr, points=Xout, chi2_initial=cost0, chi2_final=cost, iterations=accepted), st
