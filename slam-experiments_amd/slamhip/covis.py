"""The covisibility graph (``slam_covis_*``): ORB-SLAM's ``KeyFrame::UpdateConnections`` for a whole map at once.

``covisibility_device`` is ``slamhip.covisibility`` on the device, bit for bit: edges between the poses that see a common
point, their weights, and the pair lists the sparse bundle adjustment sums over.  The pair tables stay on the device; the host
learns a few scalars and the E-sized arrays.  ``CovisibilityGraph`` is what ORB-SLAM reads off the graph (best covisibles,
spanning tree, essential graph), numpy over the E-sized arrays with rules that do not depend on iteration order.

The reference has no covisibility graph.  PARITY UNPINNED: integers only, every output a function of the input alone.  There is
no CPU fallback: ``slamhip.covisibility`` stays as the statement the device is held to.
"""
from __future__ import annotations

import ctypes
import time
from typing import Optional, Sequence, Tuple

import numpy as np

from ._lib import check, load
from .ba_sparse import MAX_OBS, MAX_PAIRS, MAX_POINTS, _fixed_mask, _index_arrays  # noqa: F401
from .device import Context, default_context
from .pose_graph import MAX_EDGES, MAX_VERTICES

LIMIT_NAMES = ("threads", "sort_tile", "digit_bits", "scan_tile", "ballot_lanes", "key32_max_K", "list_thresholds", "scalar_bytes")
PLAN_NAMES = ("obs_key_bits", "obs_passes", "obs_key_bytes", "obs_tiles", "pair_key_bits", "pair_passes", "pair_key_bytes", "pair_tiles")


def limits() -> dict:
    """The library's constants (``slam_covis_limits``); needs no device."""
    lim = (ctypes.c_int32 * 8)()
    check(load().slam_covis_limits(lim))
    return dict(zip(LIMIT_NAMES, lim))


def workspace_bytes(K: int, L: int, O: int, P: int = 0) -> Tuple[int, int]:
    """Bytes of the count and of the pair workspace (``slam_covis_workspace``); needs no device."""
    n = (ctypes.c_uint64 * 2)()
    check(load().slam_covis_workspace(int(K), int(L), int(O), int(P), n))
    return int(n[0]), int(n[1])


def plan(K: int, L: int, O: int, P: int = 0) -> dict:
    """Key widths, passes and tiles of the two sorts (``slam_covis_plan``) and the memory they take; needs no device."""
    p = (ctypes.c_int32 * 8)()
    check(load().slam_covis_plan(int(K), int(L), int(O), int(P), p))
    out = dict(zip(PLAN_NAMES, p))
    out["count_workspace_bytes"], out["pair_workspace_bytes"] = workspace_bytes(K, L, O, P)
    return out


class CovisibilityTables:
    """The five arrays of ``slamhip.covisibility`` on the device: ``d_edges`` [E,2], ``d_weights`` [E], ``d_pair_ptr`` [E+1],
    ``d_pair_a`` / ``d_pair_b`` [P].  ``E``, ``P``, ``edges`` and ``weights`` are on the host as well; ``free_observations`` is
    the number of observations of free poses."""

    def __init__(self, ctx: Context, K: int, L: int, O: int):
        self.ctx, self.K, self.L, self.O = ctx, K, L, O
        self.E = self.P = self.free_observations = 0
        self.edges, self.weights = np.zeros((0, 2), np.int32), np.zeros(0, np.int32)
        self.d_edges = self.d_weights = self.d_pair_ptr = self.d_pair_a = self.d_pair_b = None

    def download(self):
        """``(edges, weights, pair_ptr, pair_a, pair_b)`` as ``slamhip.covisibility`` returns them."""
        return (self.edges.copy(), self.weights.copy(), self.d_pair_ptr.download(np.int32, (self.E + 1,)),
                self.d_pair_a.download(np.int32, (self.P,)), self.d_pair_b.download(np.int32, (self.P,)))

    def graph(self) -> "CovisibilityGraph":
        return CovisibilityGraph(self.K, self.edges, self.weights)

    def release(self) -> dict:
        """Hands the five buffers to the caller, who frees them; the tables keep the host arrays."""
        out = {n: getattr(self, n) for n in ("d_edges", "d_weights", "d_pair_ptr", "d_pair_a", "d_pair_b")}
        self.d_edges = self.d_weights = self.d_pair_ptr = self.d_pair_a = self.d_pair_b = None
        return out

    def free(self) -> None:
        for n in ("d_edges", "d_weights", "d_pair_ptr", "d_pair_a", "d_pair_b"):
            b = getattr(self, n)
            if b is not None:
                b.free()
                setattr(self, n, None)

    @classmethod
    def from_observations(cls, observations, K: int, fixed=None, ctx: Optional[Context] = None, _limits=None) -> "CovisibilityTables":
        """The graph of a ``MapObservations`` (``obs[:,0]`` the pose, one list per point): ``pair_a`` / ``pair_b`` are slots of
        ``observations.obs``.  ``fixed`` as in ``covisibility_device``."""
        K, M, nnz = int(K), len(observations), observations.nnz
        if not 1 <= K <= MAX_VERTICES:
            raise ValueError(f"K must be in [1, {MAX_VERTICES}]")
        if nnz > MAX_OBS:
            raise ValueError(f"at most {MAX_OBS} observations")
        if nnz and int(observations.obs[:, 0].max()) >= K:
            raise ValueError("observation index out of range")
        fx = None if fixed is None else _fixed_mask(fixed, K)
        ctx = ctx or observations.ctx or default_context()
        dev = observations._resident(ctx)
        tmp = []
        try:
            d_op, d_ol = _new(ctx, tmp, max(nnz, 1) * 4), _new(ctx, tmp, max(nnz, 1) * 4)
            d_fx = None if fx is None else _up(ctx, tmp, fx.astype(np.uint8))
            check(ctx.lib.slam_covis_rows(ctx.handle, max(M, 1), nnz, dev["offsets"].ptr, dev["obs"].ptr, d_op.ptr, d_ol.ptr))
            return build_tables(ctx, d_op, d_ol, d_fx, K, max(M, 1), nnz, _limits)
        finally:
            for b in tmp:
                b.free()


def _new(ctx: Context, held: list, nbytes: int):
    held.append(ctx.malloc(nbytes))
    return held[-1]


def _up(ctx: Context, held: list, a: np.ndarray):
    held.append(ctx.upload(a))
    return held[-1]


def build_tables(ctx: Context, d_obs_pose, d_obs_point, d_fixed, K: int, L: int, O: int, _limits=None, phases: Optional[dict] = None):
    """The three phases over observation tables that are already on the device (``DeviceBuffer``; ``d_fixed`` may be None).
    The index ranges must have been checked on the host.  ``phases``: a dict that receives the seconds of the three calls, each
    ending in a wait, and of the allocations between them (timing tools)."""
    max_pairs, max_edges = _limits or (MAX_PAIRS, MAX_EDGES)
    lib, h = ctx.lib, ctx.handle
    t = CovisibilityTables(ctx, K, L, O)
    tmp: list = []
    spent = dict(count=0.0, pairs=0.0, edges=0.0, allocations=0.0)

    def clocked(name, fn, *a):
        t0 = time.perf_counter()
        out = fn(*a)
        spent[name] += time.perf_counter() - t0
        return out

    new = lambda nbytes: clocked("allocations", ctx.malloc, nbytes)  # noqa: E731
    try:
        ws = new(workspace_bytes(K, L, O)[0])
        tmp.append(ws)
        s = (ctypes.c_int64 * 4)()
        check(clocked("count", lib.slam_covis_count, h, K, L, O, d_obs_pose.ptr, d_obs_point.ptr, d_fixed.ptr if d_fixed is not None else None,
                      ws.ptr, s))
        t.free_observations, dup, P, bad = (int(v) for v in s)
        if bad:
            raise ValueError("observation index out of range")
        if dup:
            raise ValueError("a (pose, point) pair is observed more than once")
        if P > max_pairs:
            raise ValueError(f"{P} covisible pairs: more than the {max_pairs} the device takes")
        t.P = P
        t.d_pair_a = new(max(P, 1) * 4)
        t.d_pair_b = new(max(P, 1) * 4)
        ws2 = new(workspace_bytes(K, L, O, P)[1])
        tmp.append(ws2)
        e = ctypes.c_int64(0)
        check(clocked("pairs", lib.slam_covis_pairs, h, K, L, O, P, ws.ptr, ws2.ptr, t.d_pair_a.ptr, t.d_pair_b.ptr, ctypes.byref(e)))
        E = int(e.value)
        if E > max_edges:
            raise ValueError(f"{E} covisibility edges: more than the {max_edges} the solver takes")
        t.E = E
        t.d_edges = new(max(E, 1) * 8)
        t.d_weights = new(max(E, 1) * 4)
        t.d_pair_ptr = new((E + 1) * 4)

        def edges():
            check(lib.slam_covis_edges(h, K, P, E, ws2.ptr, t.d_edges.ptr, t.d_weights.ptr, t.d_pair_ptr.ptr))
            return t.d_edges.download(np.int32, (E, 2)), t.d_weights.download(np.int32, (E,))

        t.edges, t.weights = clocked("edges", edges)
        if phases is not None:
            phases.update(spent)
        return t
    except BaseException:
        t.free()
        raise
    finally:
        for b in tmp:
            b.free()


def covisibility_device(obs_pose, obs_point, K: int, fixed=None, L: Optional[int] = None, ctx: Optional[Context] = None, _limits=None,
                        phases: Optional[dict] = None) -> CovisibilityTables:
    """``slamhip.covisibility`` on the device -> ``CovisibilityTables``.

    ``fixed`` a mask [K] with at least one pose set, as ``covisibility`` takes it, or None: nothing is fixed, the graph as
    ORB-SLAM keeps it.  Index ranges are refused on the host before any launch; a (pose, point) pair observed more than once
    and more pairs than the device takes are refused after the count phase, before any table is filled, more edges than the
    solver takes before any edge is written - all ``ValueError`` with the messages of ``covisibility``, nothing left allocated.
    ``_limits = (pairs, edges)`` lowers the two limits (tests)."""
    K = int(K)
    op, ol = _index_arrays(obs_pose, obs_point, K, L)
    fx = None if fixed is None else _fixed_mask(fixed, K)
    if L is None:
        L = int(ol.max()) + 1 if len(ol) else 1
    L = int(L)
    if not 1 <= L <= MAX_POINTS:
        raise ValueError(f"L must be in [1, {MAX_POINTS}]")
    ctx = ctx or default_context()
    pad = lambda a: a if a.size else np.zeros(4, a.dtype)  # noqa: E731
    tmp: list = []
    try:
        d_op, d_ol = _up(ctx, tmp, pad(op)), _up(ctx, tmp, pad(ol))
        d_fx = None if fx is None else _up(ctx, tmp, fx.astype(np.uint8))
        return build_tables(ctx, d_op, d_ol, d_fx, K, L, len(op), _limits, phases)
    finally:
        for b in tmp:
            b.free()


class CovisibilityGraph:
    """What ORB-SLAM reads off the covisibility graph, from ``edges`` int [E,2] (k1 < k2, no pair twice) and ``weights`` [E] of
    ``covisibility`` / ``covisibility_device`` over ``K`` keyframes.  Every rule is a function of the graph alone."""

    def __init__(self, K: int, edges, weights):
        K = int(K)
        e = np.asarray(edges, np.int64).reshape(-1, 2)
        w = np.asarray(weights, np.int64).reshape(-1)
        if K < 1 or len(e) != len(w):
            raise ValueError("K >= 1 and one weight per edge")
        if len(e) and (e.min() < 0 or e.max() >= K or (e[:, 0] >= e[:, 1]).any() or w.min() < 1):
            raise ValueError("edges must hold 0 <= k1 < k2 < K and weights must be positive")
        if len(np.unique(e[:, 0] * K + e[:, 1])) != len(e):
            raise ValueError("an edge is listed twice")
        self.K, self.edges, self.weights = K, e.astype(np.int32), w.astype(np.int32)
        src, dst, ww = np.r_[e[:, 0], e[:, 1]], np.r_[e[:, 1], e[:, 0]], np.r_[w, w]
        order = np.lexsort((dst, -ww, src))                   # per vertex: weight descending, then index ascending
        self._adj, self._w = dst[order].astype(np.int32), ww[order].astype(np.int32)
        self._ptr = np.searchsorted(src[order], np.arange(K + 1))

    def _vertex(self, k) -> int:
        k = int(k)
        if not 0 <= k < self.K:
            raise ValueError(f"keyframe {k} is not in [0, {self.K})")
        return k

    def neighbours(self, k: int, min_weight: int = 15, with_weights: bool = False):
        """``GetCovisiblesByWeight``: the neighbours of ``k`` with at least ``min_weight`` common points, by (weight descending,
        index ascending) -> int32 ids (and their weights)."""
        k = self._vertex(k)
        a, w = self._adj[self._ptr[k]:self._ptr[k + 1]], self._w[self._ptr[k]:self._ptr[k + 1]]
        n = int(np.searchsorted(-w.astype(np.int64), -int(min_weight), side="right"))
        return (a[:n].copy(), w[:n].copy()) if with_weights else a[:n].copy()

    def best(self, k: int, n: int) -> np.ndarray:
        """``GetBestCovisibilityKeyFrames``: the first ``n`` of ``neighbours(k, min_weight=1)``."""
        if n < 0:
            raise ValueError("n must not be negative")
        return self.neighbours(k, 1)[:int(n)]

    def best_table(self, n: int) -> np.ndarray:
        """int32 [K,n]: row k = ``best(k, n)``, padded with -1 - the ``d_best`` of ``loop_candidates``."""
        if int(n) != n or n < 0:
            raise ValueError("n must be an integer >= 0")
        n = int(n)
        table = np.full((self.K, n), -1, np.int32)
        take = np.minimum(np.diff(self._ptr), n)
        row = np.repeat(np.arange(self.K, dtype=np.int64), take)
        col = np.arange(int(take.sum()), dtype=np.int64) - np.repeat(np.cumsum(take) - take, take)
        table[row, col] = self._adj[self._ptr[row] + col]
        return table

    def connected(self, k: int) -> np.ndarray:
        """``GetConnectedKeyFrames``: every neighbour of ``k``, ascending - the ``connected`` of ``detect_loop_candidates``."""
        return np.sort(self.neighbours(k, 1))

    def spanning_tree(self) -> np.ndarray:
        """int32 [K]: ``parent[k]`` the neighbour j < k of greatest weight (the lowest j on ties), -1 where k has none."""
        parent = np.full(self.K, -1, np.int32)
        e, w = self.edges.astype(np.int64), self.weights.astype(np.int64)
        if len(e):
            order = np.lexsort((e[:, 0], -w, e[:, 1]))
            child = e[order, 1]
            first = np.flatnonzero(np.r_[True, child[1:] != child[:-1]])
            parent[child[first]] = e[order[first], 0]
        return parent

    def essential_edges(self, min_weight: int = 100, extra: Sequence = ()) -> np.ndarray:
        """ORB-SLAM's essential graph: the spanning tree, the edges of at least ``min_weight`` common points and ``extra``
        (loop edges, any orientation) -> int32 [.,2], k1 < k2, ascending by (k1, k2), no edge twice."""
        parent = self.spanning_tree().astype(np.int64)
        child = np.flatnonzero(parent >= 0)
        x = np.asarray(extra, np.int64).reshape(-1, 2)
        if len(x) and (x.min() < 0 or x.max() >= self.K or (x[:, 0] == x[:, 1]).any()):
            raise ValueError(f"extra edges must join two different keyframes in [0, {self.K})")
        strong = self.edges[self.weights >= int(min_weight)].astype(np.int64)
        both = np.concatenate([np.stack([parent[child], child], 1), strong, np.sort(x, 1)])
        key = np.unique(both[:, 0] * self.K + both[:, 1])
        return np.stack([key // self.K, key % self.K], 1).astype(np.int32).reshape(-1, 2)
