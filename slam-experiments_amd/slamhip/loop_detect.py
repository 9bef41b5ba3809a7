"""Loop and relocalisation candidates (``slam_loop_*``): the covisibility-group stage of ORB-SLAM's
``KeyFrameDatabase::DetectLoopCandidates`` / ``DetectRelocalizationCandidates`` on the device, over the dense tables a
``BowDatabase`` leaves resident and a table of best covisibles, and ``LoopClosing::DetectLoop``'s consistency check over
consecutive keyframes on the host.

The reference detects no loops.  PARITY UNPINNED: integers only (the fixed-point scores of §4j, ``5 c > 4 cmax`` for 0.8 and
``4 acc > 3 acc_max`` for 0.75), every output a function of the input alone, ascending ids where ORB-SLAM follows list order.
There is no CPU fallback: ``loop_candidates_host`` is the numpy statement the device is held to, bit for bit.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np

from ._args import _Buffers
from ._lib import addr, check, load
from .bow import BowDatabase, Q_ONE, _as_vectors
from .covis import CovisibilityGraph
from .device import Context, DeviceBuffer, default_context

LIMIT_NAMES = ("threads", "tile_entries", "nb_max", "queries_max")
NB_MAX, QUERIES_MAX, ENTRIES_MAX = 16, 65535, 1 << 24
DERIVE = 0xFFFFFFFF                     # a min_s that asks for ORB-SLAM's minScore: the least s over the connected entries
NO_CONNECTED = 1 << 31                  # what that gives without a connected entry: a score of 1
MODES = {"loop": 0, "relocalization": 1}


def limits() -> dict:
    """The library's constants (``slam_loop_limits``); needs no device.  ``tile_entries``: the entries of E one workgroup takes."""
    lim = (ctypes.c_int32 * 4)()
    check(load().slam_loop_limits(lim))
    assert (lim[2], lim[3]) == (NB_MAX, QUERIES_MAX), "the library's limits are not this module's"
    return dict(zip(LIMIT_NAMES, lim))


def workspace_bytes(Q: int, E: int) -> int:
    """Bytes of the workspace of one call (``slam_loop_workspace``); needs no device."""
    n = ctypes.c_uint64(0)
    check(load().slam_loop_workspace(int(Q), int(E), ctypes.byref(n)))
    return int(n.value)


def _new(ctx: Context, held: Optional[_Buffers], nbytes: int, role: str):
    """Every device block this module allocates comes from here, and is freed with ``held`` where one is given.  ``role`` -
    "ws" for a workspace, "out" for an output - is not read here: it is there for the GPU tests, which replace this function
    to fill workspaces and outputs with different bytes before a call and to hand the same blocks out a second time."""
    b = ctx.malloc(max(int(nbytes), 16))
    if held is not None:
        held.bufs.append(b)
    return b


class BestTable:
    """A table of best covisibles resident on the device, for calls that would otherwise upload it every time (2.6 MB at
    65 536 keyframes x 10): ``host`` int32 [K,nb] (``graph.best_table(nb)`` of a ``CovisibilityGraph``, or an array) and
    ``buf``, its copy on ``ctx``.  A call over E <= K entries reads the first E rows, at the table's full width."""

    def __init__(self, graph_or_table, nb: int = 10, ctx: Optional[Context] = None):
        t = graph_or_table.best_table(nb) if isinstance(graph_or_table, CovisibilityGraph) else np.asarray(graph_or_table)
        if t.dtype.kind not in "iu" or t.ndim != 2 or not 1 <= t.shape[1] <= NB_MAX or t.shape[0] < 1:
            raise ValueError(f"a resident best table must be integers of shape [K, 1 .. {NB_MAX}], got {t.dtype} {t.shape}")
        if t.min() < -(1 << 31) or t.max() >= 1 << 31:
            raise ValueError("best_table must fit 32 bits")
        self.ctx = ctx or default_context()
        self.host = np.ascontiguousarray(t, np.int32)
        self.buf = self.ctx.upload(self.host)

    def free(self) -> None:
        if self.buf is not None:
            self.buf.free()
            self.buf = None


# ---- arguments ----------------------------------------------------------------------------------------------------------------------
class _Args:
    """The checked arguments of one call, as the library takes them."""

    def __init__(self, Q: int, E: int, best_table, connected, own_ids, limit, min_s, nb, mode: str):
        if mode not in MODES:
            raise ValueError(f"mode must be one of {sorted(MODES)}")
        if not 0 <= Q <= QUERIES_MAX or not 0 <= E <= ENTRIES_MAX:
            raise ValueError(f"at most {QUERIES_MAX} queries and 2^24 entries, got Q={Q}, E={E}")
        if isinstance(nb, bool) or int(nb) != nb or not 0 <= nb <= NB_MAX:
            raise ValueError(f"nb must be an integer in [0, {NB_MAX}]")
        self.Q, self.E, self.mode = Q, E, MODES[mode]
        self.d_best = None
        if isinstance(best_table, BestTable):
            if best_table.buf is None:
                raise ValueError("this best table has been freed")
            if nb < best_table.host.shape[1]:
                raise ValueError(f"a resident best table is read at its full width ({best_table.host.shape[1]}), got nb={nb}")
            self.d_best, best_table = best_table.buf, best_table.host
        if isinstance(best_table, CovisibilityGraph):
            if best_table.K < E:
                raise ValueError(f"the graph has {best_table.K} keyframes, the database {E} entries")
            best_table = best_table.best_table(int(nb))
        t = np.asarray(best_table)
        if t.size == 0:
            t = np.zeros((t.shape[0] if t.ndim == 2 else E, 0), np.int32)
        if t.dtype.kind not in "iu" or t.ndim != 2 or t.shape[0] < E:
            raise ValueError(f"best_table must be integers of shape [>= {E}, nb], got {t.dtype} {t.shape}")
        self.nb = min(int(nb), t.shape[1])
        t = t[:E, :self.nb]
        if t.size and (t.min() < -(1 << 31) or t.max() >= 1 << 31):
            raise ValueError("best_table must fit 32 bits")
        self.best = np.ascontiguousarray(t, np.int32)
        self.limit = self._per_query(limit, E, "limit", np.int32, 0, E + 1) if limit is not None else np.full(Q, E, np.int32)
        if self.mode == 1:
            if connected is not None or own_ids is not None or min_s is not None:
                raise ValueError("relocalisation takes no connected lists, own ids or threshold")
            self.own, self.min_s = np.full(Q, -1, np.int32), np.zeros(Q, np.uint32)
            self.excl, self.excl_off = np.zeros(0, np.int32), np.zeros(Q + 1, np.int64)
            return
        self.own = self._per_query(own_ids, -1, "own_ids", np.int32, -1, 1 << 31)
        self.min_s = self._per_query(min_s, DERIVE, "min_s", np.uint32, 0, 1 << 32)
        lists = [[] for _ in range(Q)] if connected is None else list(connected)
        if len(lists) != Q:
            raise ValueError(f"connected must hold one list per query ({Q}), got {len(lists)}")
        parts = []
        for q, c in enumerate(lists):
            c = np.asarray(c).reshape(-1)
            if c.size and c.dtype.kind not in "iu":
                raise ValueError("connected must be integer lists")
            c = c.astype(np.int64)
            if c.size and (c.min() < -(1 << 31) or c.max() >= 1 << 31):
                raise ValueError("connected ids must fit 32 bits")
            parts.append(np.r_[c, self.own[q]] if self.own[q] >= 0 else c)        # a keyframe is no candidate for itself
        self.excl_off = np.zeros(Q + 1, np.int64)
        self.excl_off[1:] = np.cumsum([len(p) for p in parts])
        self.excl = np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(0), np.int32)

    def _per_query(self, x, default, name: str, dtype, lo: int, hi: int) -> np.ndarray:
        a = np.full(self.Q, default, np.int64) if x is None else np.asarray(x)
        if a.dtype.kind not in "iu":
            raise ValueError(f"{name} must be integers")
        a = np.broadcast_to(a, (self.Q,)) if a.ndim == 0 else a
        if a.shape != (self.Q,):
            raise ValueError(f"{name} must be one integer, or one per query ({self.Q}), got shape {a.shape}")
        if self.Q and (int(a.min()) < lo or int(a.max()) >= hi):
            raise ValueError(f"{name} must lie in [{lo}, {hi})")
        return np.ascontiguousarray(a, dtype)


def _min_s(min_score) -> Optional[np.ndarray]:
    """A threshold on the score as one on ``s_int``: ``s_int / 2^31 >= min_score`` is ``s_int >= ceil(min_score * 2^31)``."""
    if min_score is None:
        return None
    a = np.asarray(min_score, np.float64)
    if not (a >= 0.0).all() or not (a <= 1.0).all():
        raise ValueError("min_score must lie in [0, 1]")
    return np.ceil(a * Q_ONE).astype(np.int64)


class LoopCandidates:
    """The result sets of Q queries: ``ids`` int32 and ``scores`` uint32 (``s_int``; the score is ``s_int / 2^31``) of query
    q in ``[offsets[q], offsets[q+1])``, ascending by id; ``skipped``: ids outside the tables that were met and passed over.
    ``candidates[q]`` is ``(ids, scores)`` of one query.  ``stages()``: ``acc`` uint64 [Q,E], ``gbest`` int32 [Q,E] and
    ``bitmap`` uint32 [Q, ceil(E/32)] where the call was asked to keep them."""

    def __init__(self, offsets, ids, scores, skipped: int, stages: Optional[dict] = None):
        self.offsets, self.ids, self.scores, self.skipped, self._stages = offsets, ids, scores, int(skipped), stages

    def __len__(self) -> int:
        return len(self.offsets) - 1

    def __getitem__(self, q: int) -> Tuple[np.ndarray, np.ndarray]:
        if not -len(self) <= q < len(self):
            raise IndexError(q)
        q %= len(self)
        return self.ids[self.offsets[q]:self.offsets[q + 1]], self.scores[self.offsets[q]:self.offsets[q + 1]]

    def stages(self) -> dict:
        if self._stages is None:
            raise ValueError("the stages were not kept: pass keep_stages=True")
        return self._stages


def _empty(Q: int, E: int, keep: bool) -> LoopCandidates:
    st = dict(acc=np.zeros((Q, E), np.uint64), gbest=np.full((Q, E), -1, np.int32), bitmap=np.zeros((Q, (E + 31) // 32), np.uint32)) if keep else None
    return LoopCandidates(np.zeros(Q + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.uint32), 0, st)


# ---- the numpy statement --------------------------------------------------------------------------------------------------------------
def loop_candidates_host(s, common, best_table, connected=None, own_ids=None, limit=None, min_s=None, nb: int = 10, mode: str = "loop",
                         keep_stages: bool = True) -> LoopCandidates:
    """``slam_loop_candidates`` / ``slam_loop_fill`` in numpy over downloaded tables ``s`` uint32 [Q,E] and ``common`` int32
    [Q,E]; the arguments of ``loop_candidates_tables``."""
    s, common = np.asarray(s), np.asarray(common)
    if s.ndim != 2 or s.shape != common.shape or s.dtype.kind not in "iu" or common.dtype.kind not in "iu":
        raise ValueError("s and common must be integer tables of one shape [Q, E]")
    Q, E = s.shape
    a = _Args(Q, E, best_table, connected, own_ids, limit, min_s, nb, mode)
    out = _empty(Q, E, True)
    st = out.stages()
    ids, scores, skipped = [], [], 0
    at = np.arange(E, dtype=np.int64)
    for q in range(Q):
        sq, cq = s[q].astype(np.int64), common[q].astype(np.int64)
        ex = a.excl[a.excl_off[q]:a.excl_off[q + 1]].astype(np.int64)
        inside = (ex >= 0) & (ex < E)
        skipped += int((~inside).sum())
        excluded = np.zeros(E, bool)
        excluded[ex[inside]] = True
        floor = int(a.min_s[q])
        if a.mode == 0 and floor == DERIVE:
            others = ex[inside & (ex != a.own[q])]
            floor = int(sq[others].min()) if len(others) else NO_CONNECTED
        shares = ~excluded & (at < a.limit[q]) & (cq > 0)
        cmax = int(cq[shares].max()) if shares.any() else 0
        words_ok = shares & (5 * cq > 4 * cmax)
        cand = np.flatnonzero(words_ok & (sq >= floor))
        if cmax == 0 or len(cand) == 0:
            ids.append(np.zeros(0, np.int32))
            scores.append(np.zeros(0, np.uint32))
            continue
        rows = a.best[cand].astype(np.int64)                                        # [C, nb]
        skipped += int((rows >= E).sum())
        valid = (rows >= 0) & (rows < E)
        j = np.where(valid, rows, 0)
        adds = valid & words_ok[j]
        acc = sq[cand] + np.where(adds, sq[j], 0).sum(1)
        group = np.concatenate([sq[cand][:, None], np.where(adds, sq[j], -1)], 1)       # the candidate first: argmax keeps the first of equals
        pick = group.argmax(1)
        gbest = np.concatenate([cand[:, None], j], 1)[np.arange(len(cand)), pick]
        st["acc"][q, cand], st["gbest"][q, cand] = acc.astype(np.uint64), gbest.astype(np.int32)
        members = np.unique(gbest[4 * acc > 3 * int(acc.max())])
        np.bitwise_or.at(st["bitmap"][q], members >> 5, (np.uint32(1) << (members & 31).astype(np.uint32)))
        ids.append(members.astype(np.int32))
        scores.append(s[q][members].astype(np.uint32))
    out.offsets[1:] = np.cumsum([len(x) for x in ids])
    out.ids, out.scores = np.concatenate(ids or [out.ids]), np.concatenate(scores or [out.scores])
    out.skipped = skipped
    if not keep_stages:
        out._stages = None
    return out


# ---- the device calls -----------------------------------------------------------------------------------------------------------------
def loop_candidates_tables(s, common, best_table, connected=None, own_ids=None, limit=None, min_s=None, nb: int = 10, mode: str = "loop",
                           keep_stages: bool = False, shape: Optional[Tuple[int, int]] = None, ctx: Optional[Context] = None) -> LoopCandidates:
    """The candidate stage over dense tables: ``s`` uint32 [Q,E] and ``common`` int32 [Q,E] as numpy arrays (uploaded), or as
    two ``DeviceBuffer`` with ``shape = (Q, E)`` (``BowDatabase.scores_dense_device``: nothing crosses PCIe but the results).

    ``best_table``: int [E,nb] (-1 = padding), a ``CovisibilityGraph`` (its ``best_table(nb)``) or a ``BestTable`` (resident:
    nothing is uploaded); ``connected``: one list of
    entry ids per query, to which a query's own id is added; ``own_ids``: the entry of each query, -1 (default) for a frame
    that is not in the database; ``limit``: entries with id >= limit are passed over (one value or one per query, default E);
    ``min_s``: a threshold on ``s_int`` per query, ``DERIVE`` (default) for the least ``s_int`` over the connected entries.
    ``mode``: "loop", or "relocalization" (no lists, no threshold).  Ids outside [0, E) in a connected list or in the row of
    a candidate are passed over and counted (``skipped``, and the context's ``index_errors``)."""
    resident = isinstance(s, DeviceBuffer)
    if resident:
        if not isinstance(common, DeviceBuffer) or shape is None:
            raise ValueError("resident tables are two DeviceBuffer and shape = (Q, E)")
        Q, E = int(shape[0]), int(shape[1])
        if s.nbytes < 4 * Q * E or common.nbytes < 4 * Q * E:
            raise ValueError(f"[{Q}, {E}] tables do not fit the device buffers")
        ctx = ctx or s.ctx
        if s.ctx is not ctx or common.ctx is not ctx:
            raise ValueError("the tables belong to another context")
    else:
        s, common = np.asarray(s), np.asarray(common)
        if s.ndim != 2 or s.shape != common.shape or s.dtype.kind not in "iu" or common.dtype.kind not in "iu":
            raise ValueError("s and common must be integer tables of one shape [Q, E]")
        if s.size and (s.min() < 0 or s.max() >= 1 << 32 or common.min() < -(1 << 31) or common.max() >= 1 << 31):
            raise ValueError("s must fit uint32 and common int32")
        Q, E = s.shape
    a = _Args(Q, E, best_table, connected, own_ids, limit, min_s, nb, mode)
    if Q == 0 or E == 0:
        return _empty(Q, E, keep_stages)
    ctx = ctx or default_context()
    W = (E + 31) // 32
    m = _Buffers(ctx)
    try:
        d_s, d_c = (s, common) if resident else (m.up(np.ascontiguousarray(s, np.uint32)), m.up(np.ascontiguousarray(common, np.int32)))
        if a.d_best is not None and a.d_best.ctx is not ctx:
            raise ValueError("the best table belongs to another context")
        d_best = a.d_best if a.d_best is not None else (m.up(a.best) if a.nb else None)
        d_excl = m.up(a.excl) if len(a.excl) else None
        ws = _new(ctx, m, workspace_bytes(Q, E), "ws")
        d_acc, d_gbest, d_bitmap = (_new(ctx, m, n, "out") for n in (8 * Q * E, 4 * Q * E, 4 * Q * W))
        counts, skipped = np.zeros(Q, np.int64), ctypes.c_int64(0)
        loop = a.mode == 0
        check(ctx.lib.slam_loop_candidates(ctx.handle, Q, E, d_s.ptr, d_c.ptr, a.nb, d_best.ptr if d_best is not None else None,
                                           d_excl.ptr if d_excl is not None else None,
                                           addr(a.excl_off) if loop else None, addr(a.own) if loop else None, addr(a.limit),
                                           addr(a.min_s) if loop else None, a.mode, ws.ptr, d_acc.ptr, d_gbest.ptr, d_bitmap.ptr, addr(counts),
                                           ctypes.byref(skipped)))
        off = np.zeros(Q + 1, np.int64)
        off[1:] = np.cumsum(counts)
        total = int(off[-1])
        d_ids, d_sc = _new(ctx, m, 4 * total, "out"), _new(ctx, m, 4 * total, "out")
        check(ctx.lib.slam_loop_fill(ctx.handle, Q, E, d_s.ptr, d_bitmap.ptr, ws.ptr, addr(off), d_ids.ptr, d_sc.ptr))
        ids = d_ids.download(np.int32, (total,)) if total else np.zeros(0, np.int32)
        scores = d_sc.download(np.uint32, (total,)) if total else np.zeros(0, np.uint32)
        st = None
        if keep_stages:
            st = dict(acc=d_acc.download(np.uint64, (Q, E)), gbest=d_gbest.download(np.int32, (Q, E)), bitmap=d_bitmap.download(np.uint32, (Q, W)))
        return LoopCandidates(off, ids, scores, int(skipped.value), st)
    finally:
        m.free()


def _query_tables(db: BowDatabase, vectors):
    if not isinstance(db, BowDatabase):
        raise ValueError("expected a BowDatabase")
    return db.scores_dense_device(_as_vectors(vectors))


def loop_candidates(db: BowDatabase, vectors, graph_or_best_table, connected=None, own_ids=None, limit=None, min_score=None, nb: int = 10,
                    keep_stages: bool = False) -> LoopCandidates:
    """``DetectLoopCandidates`` for the Q ``vectors`` at once against the entries of ``db`` (entry id = keyframe index): the
    dense query and the candidate stage, both on the device - the [Q,E] tables never leave it.  ``min_score``: None for
    ORB-SLAM's minScore (the lowest score against the ``connected`` keyframes, 1 without any), or a score in [0, 1] (one or one
    per query).  The other arguments as ``loop_candidates_tables`` takes them."""
    floor = _min_s(min_score)
    d_s, d_c, Q, E = _query_tables(db, vectors)
    try:
        if d_s is None:
            _Args(Q, E, graph_or_best_table if E else np.zeros((0, 0), np.int32), connected, own_ids, limit, floor, nb, "loop")
            return _empty(Q, E, keep_stages)
        return loop_candidates_tables(d_s, d_c, graph_or_best_table, connected, own_ids, limit, floor, nb, "loop", keep_stages, (Q, E), db.ctx)
    finally:
        for b in (d_s, d_c):
            if b is not None:
                b.free()


def relocalization_candidates(db: BowDatabase, vectors, best_table, nb: int = 10, keep_stages: bool = False) -> LoopCandidates:
    """``DetectRelocalizationCandidates`` for Q frames at once: every entry that shares a word takes part, there is no
    threshold on the score, the groups are summed and retained as for a loop."""
    d_s, d_c, Q, E = _query_tables(db, vectors)
    try:
        if d_s is None:
            return _empty(Q, E, keep_stages)
        return loop_candidates_tables(d_s, d_c, best_table, nb=nb, mode="relocalization", keep_stages=keep_stages, shape=(Q, E), ctx=db.ctx)
    finally:
        for b in (d_s, d_c):
            if b is not None:
                b.free()


# ---- host only ------------------------------------------------------------------------------------------------------------------------
class LoopConsistency:
    """``LoopClosing::DetectLoop``'s consistency check, carried from keyframe to keyframe (``mvConsistentGroups``); on the host
    by decision: a handful of candidates against a handful of groups, each keyframe after the one before.

    ``update(candidates, graph)`` expands each candidate c to ``{c} | graph.connected(c)`` and compares it with the groups of
    the keyframe before: a group that shares a member is met.  A previous group is continued (count + 1) by the first candidate
    that meets it only; a candidate is returned, once, when a count it meets has reached ``threshold`` (whether or not it was
    the one to continue that group - ORB-SLAM's rule); a candidate that meets no previous group starts a group at 0.  So a
    place is accepted at the keyframe that is the ``threshold``-th in a row consistent with the first detection.  An empty
    candidate list clears the state."""

    def __init__(self, threshold: int = 3):
        if isinstance(threshold, bool) or int(threshold) != threshold or threshold < 0:
            raise ValueError("threshold must be an integer >= 0")
        self.threshold = int(threshold)
        self.groups: List[Tuple[frozenset, int]] = []

    def reset(self) -> None:
        self.groups = []

    def update(self, candidates: Sequence[int], graph: CovisibilityGraph) -> List[int]:
        if not isinstance(graph, CovisibilityGraph):
            raise ValueError("update takes a CovisibilityGraph")
        cands = [int(c) for c in np.asarray(candidates).reshape(-1)]
        if any(not 0 <= c < graph.K for c in cands):
            raise ValueError(f"a candidate is not a keyframe in [0, {graph.K})")
        if not cands:
            self.groups = []
            return []
        current: List[Tuple[frozenset, int]] = []
        continued = [False] * len(self.groups)
        accepted: List[int] = []
        for c in cands:
            group = frozenset([c] + graph.connected(c).tolist())
            enough = met = False
            for g, (previous, count) in enumerate(self.groups):
                if group.isdisjoint(previous):
                    continue
                met = True
                if not continued[g]:
                    current.append((group, count + 1))
                    continued[g] = True
                if count + 1 >= self.threshold and not enough:
                    accepted.append(c)
                    enough = True
            if not met:
                current.append((group, 0))
        self.groups = current
        return accepted


class LoopDetector:
    """``LoopClosing::DetectLoop`` for one keyframe at a time: query -> candidates -> consistency, then the keyframe joins the
    database (its entry id is its keyframe index, so keyframes must arrive in order).  ``min_gap``: a keyframe whose id is
    less than ``min_gap`` past the last closed loop (``loop_closed(k)``) is added and nothing else - ORB-SLAM's 10, counted in
    keyframe ids."""

    def __init__(self, db: BowDatabase, threshold: int = 3, min_gap: int = 10, nb: int = 10):
        if not isinstance(db, BowDatabase):
            raise ValueError("expected a BowDatabase")
        if int(min_gap) != min_gap or min_gap < 0:
            raise ValueError("min_gap must be an integer >= 0")
        self.db, self.nb, self.min_gap = db, int(nb), int(min_gap)
        self.consistency = LoopConsistency(threshold)
        self.last_loop: Optional[int] = None
        self.last: Optional[LoopCandidates] = None

    def loop_closed(self, keyframe: int) -> None:
        """The loop found at ``keyframe`` was closed: the gate counts from here."""
        self.last_loop = int(keyframe)

    def step(self, vector, graph: CovisibilityGraph, min_score=None) -> List[int]:
        """Keyframe ``len(db)`` arrives with its BoW ``vector``; ``graph`` the covisibility graph as it stands (it may know
        later keyframes: only entries of the database are read).  Returns the accepted loop keyframes, usually none."""
        if not isinstance(graph, CovisibilityGraph):
            raise ValueError("step takes a CovisibilityGraph")
        v = _as_vectors(vector)
        if len(v) != 1:
            raise ValueError("step takes one vector")
        k = E = len(self.db)
        if graph.K < E:
            raise ValueError(f"the graph has {graph.K} keyframes, the database {E} entries")
        self.last = None
        try:
            if self.last_loop is not None and k < self.last_loop + self.min_gap:
                return []
            if E == 0:
                self.consistency.reset()
                return []
            table = graph.best_table(self.nb)[:E]
            table[table >= E] = -1                                  # keyframes that have not arrived are not in the database
            conn = graph.connected(k) if k < graph.K else np.zeros(0, np.int32)
            self.last = loop_candidates(self.db, v, table, [conn[conn < E]], None, None, min_score, self.nb)
            return self.consistency.update(self.last.ids, graph)
        finally:
            self.db.add(v)


__all__ = ["BestTable", "LoopCandidates", "LoopConsistency", "LoopDetector", "loop_candidates", "loop_candidates_host", "loop_candidates_tables",
           "relocalization_candidates"]
