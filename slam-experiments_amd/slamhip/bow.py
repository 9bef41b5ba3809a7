"""Bag-of-words place recognition on the GPU (``slam_bow_*``): DBoW2's vocabulary tree over 256-bit
descriptors, tf-idf BoW vectors (``TF_IDF``, ``L1_NORM``), and a keyframe database whose inverted index answers "have I been
here before?" with a ranked list of entries - the candidates ``solve_pnp_ransac_batch`` / ``estimate_sim3_batch`` take.

The reference has no call site (it detects no loops).  PARITY UNPINNED: no DBoW2 exists here; the tree descent, the weights
and the L1 score are restated from their definitions, the score in fixed point (``q = floor(v * 2^31)``, a sum of integer
minima, so that it is the same on every run), and training is a deterministic hierarchical k-majority with maximin seeding
(DBoW2's k-means++ draws are not reproduced).  The text form is ORB-SLAM2's ``loadFromTextFile``.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import threading
from typing import Optional, Sequence, Tuple

import numpy as np

from ._args import _Buffers, _device_rows, _offsets, _rows_arg
from ._lib import check, load
from .device import Context, DeviceBuffer, default_context
from .matching import as_descriptors

K_MAX, DEPTH_MAX, IMAGE_MAX, RESULTS_MAX = 32, 10, 8192, 64
WORDS_MAX = 1 << 24
Q_ONE = float(1 << 31)


def limits() -> dict:
    """The library's limits (``slam_bow_limits``); needs no GPU.  ``query_pass_entries``: database entries one LDS pass of the
    query kernel holds; ``lanes16_up_to``: descriptors up to which ``bow_transform(lanes=0)`` takes sixteen lanes each."""
    lim = (ctypes.c_int32 * 7)()
    check(load().slam_bow_limits(lim))
    assert (lim[0], lim[1], lim[2], lim[3]) == (K_MAX, DEPTH_MAX, IMAGE_MAX, RESULTS_MAX), "the library's limits are not this module's"
    return {"query_pass_entries": lim[4], "staged_nodes": lim[5], "lanes16_up_to": lim[6]}


# ----------------------------------------------------------------------------------------------------------------- vocabulary

class Vocabulary:
    """A rooted k-ary tree of 256-bit centres in flat arrays: ``node_desc`` u8 [n_nodes,32], ``child_begin`` / ``child_count``
    int32 (the children of a node are contiguous; count 0 = leaf), ``word_of_node`` int32 (-1 for inner nodes), ``idf`` f64
    [n_words].  Node 0 is the root; leaves may sit at any depth <= ``depth``.  Build one with ``from_arrays`` (validated),
    ``train_vocabulary``, ``load`` or ``read_dbow2_text``."""

    def __init__(self, k, depth, node_desc, child_begin, child_count, word_of_node, idf):
        self.k, self.depth = int(k), int(depth)
        self.node_desc, self.child_begin, self.child_count = node_desc, child_begin, child_count
        self.word_of_node, self.idf = word_of_node, idf
        self._lock = threading.Lock()
        self._device: dict = {}

    @property
    def n_nodes(self) -> int:
        return len(self.node_desc)

    @property
    def n_words(self) -> int:
        return len(self.idf)

    def arrays(self) -> dict:
        return {"k": self.k, "depth": self.depth, "node_desc": self.node_desc, "child_begin": self.child_begin,
                "child_count": self.child_count, "word_of_node": self.word_of_node, "idf": self.idf}

    @classmethod
    def from_arrays(cls, k, depth, node_desc, child_begin, child_count, word_of_node, idf) -> "Vocabulary":
        k, depth = int(k), int(depth)
        if not 2 <= k <= K_MAX or not 1 <= depth <= DEPTH_MAX:
            raise ValueError(f"k must lie in [2, {K_MAX}] and depth in [1, {DEPTH_MAX}], got k={k}, depth={depth}")
        nd = np.asarray(node_desc)
        if nd.dtype != np.uint8 or nd.ndim != 2 or nd.shape[1] != 32 or len(nd) < 1:
            raise ValueError(f"node_desc must be uint8 [n_nodes,32], got {nd.dtype} {nd.shape}")
        n = len(nd)
        ints = []
        for name, a in (("child_begin", child_begin), ("child_count", child_count), ("word_of_node", word_of_node)):
            a = np.asarray(a)
            if a.dtype.kind not in "iu" or a.shape != (n,):
                raise ValueError(f"{name} must be integers of shape [{n}], got {a.dtype} {a.shape}")
            ints.append(a.astype(np.int64))
        cb, cc, won = ints
        w = np.asarray(idf)
        if w.dtype.kind != "f" or w.ndim != 1:
            raise ValueError("idf must be floating point of shape [n_words]")
        w = np.ascontiguousarray(w, np.float64)
        if (cc < 0).any() or (cc > k).any():
            raise ValueError(f"child_count must lie in [0, {k}]")
        inner = np.flatnonzero(cc > 0)
        order = inner[np.argsort(cb[inner], kind="stable")]
        ends = cb[order] + cc[order]
        if n > 1 and (len(order) == 0 or cb[order[0]] != 1 or ends[-1] != n or (cb[order[1:]] != ends[:-1]).any()):
            raise ValueError("the children of the inner nodes must be contiguous and tile the nodes 1 .. n_nodes - 1, one parent each")
        if n == 1 and len(order):
            raise ValueError("child range out of bounds")
        level = np.full(n, -1, np.int64)
        level[0] = 0
        for d in range(depth):
            at = np.flatnonzero((level == d) & (cc > 0))
            if len(at) == 0:
                break
            kids = np.concatenate([np.arange(cb[v], cb[v] + cc[v]) for v in at])
            level[kids] = d + 1
        if (level < 0).any():
            raise ValueError(f"a node is deeper than depth={depth}, or not reachable from the root")
        if (cc[level == depth] > 0).any():
            raise ValueError(f"a node at depth {depth} has children")
        leaves = cc == 0
        if (won[~leaves] != -1).any():
            raise ValueError("word_of_node must be -1 for inner nodes (every inner node has at least one child)")
        nw = int(leaves.sum())
        if nw > WORDS_MAX:
            raise ValueError("more than 2^24 words")
        if len(w) != nw or not np.array_equal(np.sort(won[leaves]), np.arange(nw)):
            raise ValueError(f"the {nw} leaves must carry the word ids 0 .. {nw - 1}, one each, and idf must have that many entries")
        if not np.isfinite(w).all() or (w < 0).any():
            raise ValueError("idf must be finite and >= 0")
        return cls(k, depth, np.ascontiguousarray(nd), cb.astype(np.int32), cc.astype(np.int32), won.astype(np.int32), w)

    def save(self, path) -> None:
        np.savez_compressed(path, k=self.k, depth=self.depth, node_desc=self.node_desc, child_begin=self.child_begin,
                            child_count=self.child_count, word_of_node=self.word_of_node, idf=self.idf)

    @classmethod
    def load(cls, path) -> "Vocabulary":
        with np.load(path) as z:
            return cls.from_arrays(int(z["k"]), int(z["depth"]), z["node_desc"], z["child_begin"], z["child_count"],
                                   z["word_of_node"], z["idf"])

    def upload(self, ctx: Optional[Context] = None) -> "DeviceVocabulary":
        """The tree on the device of ``ctx`` (made once per context and kept until ``free``)."""
        ctx = ctx or default_context()
        with self._lock:
            dv = self._device.get(ctx)
            if dv is None:
                dv = self._device[ctx] = DeviceVocabulary(ctx, self)
            return dv

    def free(self) -> None:
        with self._lock:
            for dv in self._device.values():
                dv.free()
            self._device = {}


class DeviceVocabulary:
    """``Vocabulary.upload``: node rows, (first child, count) pairs, word ids and idf in device memory."""

    def __init__(self, ctx: Context, vocab: Vocabulary):
        self.ctx, self.vocab = ctx, vocab
        child = np.ascontiguousarray(np.stack([vocab.child_begin, vocab.child_count], axis=1), np.int32)
        self.node_desc, self.child = ctx.upload(vocab.node_desc), ctx.upload(child)
        self.word_of_node, self.idf = ctx.upload(vocab.word_of_node), ctx.upload(vocab.idf)

    def free(self) -> None:
        for b in (self.node_desc, self.child, self.word_of_node, self.idf):
            b.free()


def read_dbow2_text(path) -> Vocabulary:
    """A vocabulary in the text form ORB-SLAM2's ``loadFromTextFile`` reads (ORBvoc.txt): the header ``k L scoring
    weighting``, then one line per node in id order from 1, ``parent is_leaf b0 .. b31 weight``; word ids go to the leaves in
    file order.  Nodes are renumbered breadth first so that siblings are contiguous.  Only scoring 0 (L1) and weighting 0
    (TF-IDF) are supported."""
    with open(path, "r") as fh:
        head = fh.readline().split()
        if len(head) != 4:
            raise ValueError("the header must be 'k L scoring weighting'")
        k, depth, scoring, weighting = (int(x) for x in head)
        if scoring != 0 or weighting != 0:
            raise NotImplementedError(f"only L1 scoring (0) with TF-IDF weighting (0) is supported, got scoring={scoring}, weighting={weighting}")
        rows = [ln.split() for ln in fh if ln.strip()]
    if any(len(r) != 35 for r in rows):
        raise ValueError("every node line must be 'parent is_leaf b0 .. b31 weight'")
    n = len(rows) + 1
    parent = np.array([0] + [int(r[0]) for r in rows], np.int64)
    is_leaf = np.array([0] + [int(r[1]) for r in rows], np.int64) != 0
    desc = np.zeros((n, 32), np.uint8)
    if rows:
        b = np.array([[int(x) for x in r[2:34]] for r in rows], np.int64)
        if b.min() < 0 or b.max() > 255:
            raise ValueError("descriptor bytes must lie in [0, 255]")
        desc[1:] = b
    weight = np.array([0.0] + [float(r[34]) for r in rows])
    if n == 1:
        is_leaf[0] = True
    if (parent[1:] < 0).any() or (parent[1:] >= n).any():
        raise ValueError("a parent id is out of range")
    word = np.full(n, -1, np.int64)
    word[is_leaf] = np.arange(int(is_leaf.sum()))
    kids = [[] for _ in range(n)]
    for v in range(1, n):
        kids[parent[v]].append(v)
    order, begin, count = [0], [], []
    for v in order:                                     # breadth first; `order` grows while it is walked
        begin.append(len(order) if kids[v] else 0)
        count.append(len(kids[v]))
        order.extend(kids[v])
    if len(order) != n:
        raise ValueError("a node is not reachable from the root")
    order = np.asarray(order)
    if (np.asarray(count)[is_leaf[order]] != 0).any() or (np.asarray(count)[~is_leaf[order]] == 0).any():
        raise ValueError("is_leaf disagrees with the parent column")
    won = word[order]
    idf = np.zeros(int(is_leaf.sum()))
    idf[won[won >= 0]] = weight[order][won >= 0]
    return Vocabulary.from_arrays(k, depth, desc[order], begin, count, won, idf)


def write_dbow2_text(vocab: Vocabulary, path) -> None:
    """``vocab`` in the text form of ``read_dbow2_text``.  The reader gives word ids to the leaves in file order, so the word
    ids must ascend with the node id (as in every trained or read vocabulary)."""
    leaves = np.flatnonzero(vocab.child_count == 0)
    if not np.array_equal(vocab.word_of_node[leaves], np.arange(len(leaves))):
        raise ValueError("the text form carries word ids by file order: they must ascend with the node id")
    parent = np.zeros(vocab.n_nodes, np.int64)
    for v in np.flatnonzero(vocab.child_count > 0):
        parent[vocab.child_begin[v]:vocab.child_begin[v] + vocab.child_count[v]] = v
    with open(path, "w") as fh:
        fh.write(f"{vocab.k} {vocab.depth} 0 0\n")
        for v in range(1, vocab.n_nodes):
            leaf = vocab.child_count[v] == 0
            w = float(vocab.idf[vocab.word_of_node[v]]) if leaf else 0.0
            fh.write(f"{parent[v]} {int(leaf)} {' '.join(str(int(x)) for x in vocab.node_desc[v])} {w!r}\n")


# ------------------------------------------------------------------------------------------------------------------ transform

def _transform_device(dv: DeviceVocabulary, m: _Buffers, rows: DeviceBuffer, n: int, levels_up: int, lanes: int = 0):
    ctx, v = dv.ctx, dv.vocab
    dw, dn = m.new(4 * n), m.new(4 * n)
    check(ctx.lib.slam_bow_transform(ctx.handle, rows.ptr, n, dv.node_desc.ptr, dv.child.ptr, dv.word_of_node.ptr, v.n_nodes, v.depth,
                                     levels_up, lanes, dw.ptr, dn.ptr))
    return dw, dn


def _levels_up(levels_up) -> int:
    if int(levels_up) != levels_up or levels_up < 0:
        raise ValueError("levels_up must be an integer >= 0")
    return min(int(levels_up), 1 << 20)


def bow_transform(vocab: Vocabulary, descriptors, offsets=None, levels_up: int = 0, ctx: Optional[Context] = None, lanes: int = 0):
    """DBoW2's ``transform`` per feature: (words int32 [n], nodes int32 [n]) of descriptors u8 [n,32] - the leaf's word id, and
    the node of the path at depth ``min(leaf depth, max(0, depth - levels_up))`` (the direct index ORB-SLAM's ``SearchByBoW``
    groups features by).  ``descriptors`` may be a ``(DeviceBuffer, n)`` pair as ``OrbResult.device_descriptors(b)`` returns
    it: resident rows never cross PCIe.  ``offsets`` (int [B+1], optional) is only checked against n.  ``lanes``: 1 or 16 lanes
    per descriptor (two kernels, the same results), 0 = the library chooses by n."""
    levels_up = _levels_up(levels_up)
    if lanes not in (0, 1, 16):
        raise ValueError("lanes must be 0, 1 or 16")
    rows, n = _rows_arg(descriptors)
    if offsets is not None:
        _offsets(offsets, n)
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    ctx = ctx or default_context()
    m = _Buffers(ctx)
    try:
        rows = _device_rows(ctx, m, rows)
        dw, dn = _transform_device(vocab.upload(ctx), m, rows, n, levels_up, lanes)
        return dw.download(np.int32, (n,)), dn.download(np.int32, (n,))
    finally:
        m.free()


# -------------------------------------------------------------------------------------------------------------------- vectors

class BowVectors:
    """The BoW vectors of B images as compressed rows: ``offsets`` int64 [B+1], and per kept word (ascending id inside a row)
    ``words`` int32, ``values`` f64 (L1-normalised tf-idf) and ``q`` uint32 (``floor(value * 2^31)``, what the database
    scores with).  ``vectors[b]`` is the row of image b as a one-row ``BowVectors``.  With ``keep_on_device`` the four arrays
    also stay resident (``device``: buffers in that order) until ``free``."""

    def __init__(self, offsets, words, values, q, device: Optional[Tuple[DeviceBuffer, ...]] = None):
        self.offsets, self.words, self.values, self.q, self.device = offsets, words, values, q, device

    def __len__(self) -> int:
        return len(self.offsets) - 1

    def __getitem__(self, b: int) -> "BowVectors":
        if not -len(self) <= b < len(self):
            raise IndexError(b)
        b %= len(self)
        lo, hi = int(self.offsets[b]), int(self.offsets[b + 1])
        return BowVectors(np.array([0, hi - lo], np.int64), self.words[lo:hi].copy(), self.values[lo:hi].copy(), self.q[lo:hi].copy())

    def free(self) -> None:
        if self.device is not None:
            for b in self.device:
                b.free()
            self.device = None


def _as_vectors(v) -> BowVectors:
    if isinstance(v, BowVectors):
        return v
    if isinstance(v, (list, tuple)) and all(isinstance(x, BowVectors) for x in v):
        off = np.zeros(1 + sum(len(x) for x in v), np.int64)
        np.cumsum(np.concatenate([np.diff(x.offsets) for x in v] or [np.zeros(0, np.int64)]), out=off[1:])
        cat = lambda name, dt: np.concatenate([getattr(x, name) for x in v]).astype(dt) if len(v) else np.zeros(0, dt)
        return BowVectors(off, cat("words", np.int32), cat("values", np.float64), cat("q", np.uint32))
    raise ValueError("expected BowVectors (or a list of them)")


def bow_vectors(vocab: Vocabulary, descriptors, offsets, keep_on_device: bool = False, ctx: Optional[Context] = None) -> BowVectors:
    """DBoW2's ``transform`` per image: the tf-idf vectors of B images, image b owning the descriptor rows
    ``[offsets[b], offsets[b+1])`` (at most 8192 each).  Descriptors as in ``bow_transform``."""
    rows, n = _rows_arg(descriptors)
    off = _offsets(offsets, n)
    if len(off) > 1 and np.diff(off).max() > IMAGE_MAX:
        raise ValueError(f"at most {IMAGE_MAX} descriptors per image")
    ctx = ctx or default_context()
    m = _Buffers(ctx)
    try:
        rows = _device_rows(ctx, m, rows)
        dv = vocab.upload(ctx)
        dw = _transform_device(dv, m, rows, n, 0)[0] if n else m.new(16)
        return _vectors_device(dv, m, dw, off, n, dv.idf, keep_on_device)
    finally:
        m.free()


def _vectors_device(dv: DeviceVocabulary, m: _Buffers, dw: DeviceBuffer, off: np.ndarray, n: int, d_idf: DeviceBuffer, keep: bool) -> BowVectors:
    ctx, B = dv.ctx, len(off) - 1
    need = ctypes.c_uint64(0)
    check(ctx.lib.slam_bow_vectors_workspace(B, n, ctypes.byref(need)))
    out = [ctx.malloc(max(8 * (B + 1), 16)), ctx.malloc(max(4 * n, 16)), ctx.malloc(max(8 * n, 16)), ctx.malloc(max(4 * n, 16))]
    try:
        ws, do = m.new(need.value), m.up(off)
        check(ctx.lib.slam_bow_vectors(ctx.handle, dw.ptr, do.ptr, B, n, d_idf.ptr, dv.vocab.n_words, ws.ptr, ws.nbytes, out[0].ptr,
                                       out[1].ptr, out[2].ptr, out[3].ptr))
        o = out[0].download(np.int64, (B + 1,))
        t = int(o[-1])
        res = BowVectors(o, out[1].download(np.int32, (t,)), out[2].download(np.float64, (t,)), out[3].download(np.uint32, (t,)),
                         tuple(out) if keep else None)
    except BaseException:
        keep = False
        raise
    finally:
        if not keep:
            for b in out:
                b.free()
    return res


# ------------------------------------------------------------------------------------------------------------------- database

class BowDatabase:
    """DBoW2's ``TemplatedDatabase`` on the device: a growing forward store (per entry its sorted words and q values) and an
    inverted index (per word the postings (entry, q)), rebuilt by a counting sort at the first query after an ``add``.
    Scores are ``s_int / 2^31`` with ``s_int = sum over the shared words of min(q, p)``: for L1-normalised non-negative vectors
    DBoW2's L1 score ``1 - |v - w|_1 / 2`` is that sum of minima, and in integers it does not depend on the order of the
    postings or of the atomic adds.  ``add`` and the queries may be called from several threads: the object's own lock covers
    its store and index; the library calls themselves keep no state."""

    def __init__(self, vocab: Vocabulary, ctx: Optional[Context] = None, capacity: int = 1 << 16):
        self.vocab, self.ctx = vocab, ctx or default_context()
        self._lock = threading.Lock()
        self._cap = max(int(capacity), 16)
        self._store = self.ctx.malloc(12 * self._cap)           # words int32 | entry ids int32 | q uint32, `cap` slots each
        self._counts: list = []
        self._total = 0
        self._index: Optional[Tuple[DeviceBuffer, DeviceBuffer, int]] = None      # (word offsets, postings, entries covered)

    def __len__(self) -> int:
        return len(self._counts)

    def _parts(self, store: DeviceBuffer, cap: int):
        return [store.view(i * 4 * cap, 4 * cap) for i in range(3)]

    def add(self, vector_or_descriptors) -> int:
        """Append one entry: a one-row ``BowVectors``, or the descriptors of one image; returns the entry's id."""
        v = vector_or_descriptors
        if not isinstance(v, BowVectors):
            v = bow_vectors(self.vocab, v, [0, _rows_arg(v)[1]], ctx=self.ctx)
        if len(v) != 1:
            raise ValueError("add takes one vector at a time")
        return self.add_vectors(v)[0]

    def add_vectors(self, vectors: BowVectors) -> range:
        """Append every row of ``vectors`` as an entry of its own, in one upload; returns the range of their ids."""
        v = _as_vectors(vectors)
        words, off = np.ascontiguousarray(v.words, np.int32), np.asarray(v.offsets, np.int64)
        t = len(words)
        if t:
            inside = np.ones(t, bool)
            inside[off[1:-1][off[1:-1] < t]] = False                # a row's first word is not compared with the row before
            if words.min() < 0 or words.max() >= self.vocab.n_words or (np.diff(words) <= 0)[inside[1:]].any():
                raise ValueError("the words of a vector must ascend and lie inside the vocabulary")
        with self._lock:
            if self._total + t > self._cap:
                cap = self._cap
                while cap < self._total + t:
                    cap *= 2
                grown = self.ctx.malloc(12 * cap)
                for src, dst in zip(self._parts(self._store, self._cap), self._parts(grown, cap)):
                    if self._total:
                        check(self.ctx.lib.slam_copy(self.ctx.handle, dst.ptr, src.ptr, 4 * self._total))
                self.ctx.sync()
                self._store.free()
                self._store, self._cap = grown, cap
            first = len(self._counts)
            if t:
                pw, pe, pq = self._parts(self._store, self._cap)
                ids = np.repeat(np.arange(first, first + len(v), dtype=np.int32), np.diff(off))
                pw.view(4 * self._total, 4 * t).upload(words)
                pe.view(4 * self._total, 4 * t).upload(ids)
                pq.view(4 * self._total, 4 * t).upload(np.ascontiguousarray(v.q, np.uint32))
            self._counts.extend(np.diff(off).tolist())
            self._total += t
            return range(first, first + len(v))

    def _ensure_index(self):
        """(word offsets, postings, entries) of the current store; called with the lock held."""
        E = len(self._counts)
        if self._index is not None and self._index[2] == E:
            return self._index
        self._drop_index()
        nw, T, ctx = self.vocab.n_words, self._total, self.ctx
        off, post = ctx.malloc(4 * (nw + 1)), ctx.malloc(max(8 * T, 16))
        m = _Buffers(ctx)
        try:
            cursor, perm = m.new(4 * nw), m.new(4 * T)
            pw, pe, pq = self._parts(self._store, self._cap)
            check(ctx.lib.slam_bow_index_build(ctx.handle, pw.ptr, pe.ptr, pq.ptr, T, nw, off.ptr, cursor.ptr, perm.ptr, post.ptr))
            ctx.sync()
        except BaseException:
            off.free()
            post.free()
            raise
        finally:
            m.free()
        self._index = (off, post, E)
        return self._index

    def rebuild_index(self) -> None:
        """Rebuild the inverted index now (otherwise the next query does it)."""
        with self._lock:
            self._drop_index()
            self._ensure_index()

    def _drop_index(self) -> None:
        if self._index is not None:
            self._index[0].free()
            self._index[1].free()
            self._index = None

    def _run(self, vectors, max_results: int, max_id, dense: bool, resident: bool = False):
        v = _as_vectors(vectors)
        Q = len(v)
        with self._lock:
            E = len(self._counts)
            limit = E if max_id is None else int(max_id)
            if limit < 0:
                raise ValueError("max_id must be >= 0")
            R = max_results
            if dense:
                shape = (Q, E)
                if Q == 0 or E == 0:
                    return (None, None, Q, E) if resident else (np.zeros(shape, np.uint32), np.zeros(shape, np.int32))
            elif Q == 0:
                return np.zeros((0, R), np.int32), np.zeros((0, R)), np.zeros((0, R), np.int32)
            off, post, _ = self._ensure_index()
            ctx = self.ctx
            m = _Buffers(ctx)
            try:
                if v.device is not None and v.device[0].ctx is ctx:
                    qo, qw, qq = v.device[0], v.device[1], v.device[3]
                else:
                    qo, qw, qq = m.up(np.ascontiguousarray(v.offsets, np.int64)), m.up(np.ascontiguousarray(v.words, np.int32)), \
                        m.up(np.ascontiguousarray(v.q, np.uint32))
                if dense:
                    ds, dc = (ctx.malloc(4 * Q * E), ctx.malloc(4 * Q * E)) if resident else (m.new(4 * Q * E), m.new(4 * Q * E))
                    try:
                        check(ctx.lib.slam_bow_query(ctx.handle, qo.ptr, qw.ptr, qq.ptr, Q, off.ptr, post.ptr, self.vocab.n_words, E, E, 1,
                                                     None, None, None, ds.ptr, dc.ptr))
                        if resident:
                            return ds, dc, Q, E
                    except BaseException:
                        if resident:
                            ds.free()
                            dc.free()
                        raise
                    return ds.download(np.uint32, shape), dc.download(np.int32, shape)
                di, ds, dc = m.new(4 * Q * R), m.new(4 * Q * R), m.new(4 * Q * R)
                check(ctx.lib.slam_bow_query(ctx.handle, qo.ptr, qw.ptr, qq.ptr, Q, off.ptr, post.ptr, self.vocab.n_words, E, limit, R,
                                             di.ptr, ds.ptr, dc.ptr, None, None))
                return (di.download(np.int32, (Q, R)), ds.download(np.uint32, (Q, R)).astype(np.float64) / Q_ONE,
                        dc.download(np.int32, (Q, R)))
            finally:
                m.free()

    def query(self, vectors, max_results: int = 10, max_id=None):
        """DBoW2's ``query`` (L1) for Q vectors at once: per query the entries with id < ``max_id`` (None: all) that share a
        word with it, by (score descending, id ascending): (ids int32 [Q,R], scores f64 [Q,R], common int32 [Q,R]) with
        R = ``max_results`` <= 64, fillers (-1, 0.0, 0).  ``common`` is the number of shared words."""
        if int(max_results) != max_results or not 1 <= max_results <= RESULTS_MAX:
            raise ValueError(f"max_results must lie in [1, {RESULTS_MAX}]")
        return self._run(vectors, int(max_results), max_id, False)

    def scores_dense(self, vectors):
        """(s_int uint32 [Q,E], common int32 [Q,E]) of every query against every entry; the score is ``s_int / 2^31``."""
        return self._run(vectors, 1, None, True)

    def scores_dense_device(self, vectors):
        """``scores_dense`` without the download: (d_s, d_common, Q, E), two ``DeviceBuffer`` the caller frees, holding the
        tables uint32 / int32 [Q,E] - what ``loop_candidates`` reads.  (None, None, Q, E) where Q or E is 0."""
        return self._run(vectors, 1, None, True, True)

    def free(self) -> None:
        with self._lock:
            self._drop_index()
            if self._store is not None:
                self._store.free()
                self._store = None
            self._counts, self._total = [], 0


# ------------------------------------------------------------------------------------------------------------------- training

def train_vocabulary(descriptors, image_offsets, k: int = 10, depth: int = 6, max_iters: int = 16, ctx: Optional[Context] = None) -> Vocabulary:
    """A vocabulary from the descriptors u8 [n,32] of N images (image b owns rows ``[image_offsets[b], image_offsets[b+1])``, at
    most 8192 each): hierarchical k-majority, one depth of the tree per round of kernels, deterministic.  Every node is seeded
    by maximin (first row, then the row farthest from the centres so far, until k centres or distance 0; one centre = a
    leaf), iterated at most ``max_iters`` times (nearest centre, lowest on ties; bitwise majority with ``2 * count >= rows``),
    and the centres that own rows after a final assignment become its children.  Node ids are breadth first, words the leaves
    in id order, ``idf = ln(N / N_i)`` from the device's per-word image counts."""
    d = as_descriptors(descriptors)
    n = len(d)
    off = _offsets(image_offsets, n, "image_offsets")
    k, depth, max_iters = int(k), int(depth), int(max_iters)
    if not 2 <= k <= K_MAX or not 1 <= depth <= DEPTH_MAX or max_iters < 1:
        raise ValueError(f"k must lie in [2, {K_MAX}], depth in [1, {DEPTH_MAX}] and max_iters >= 1")
    if n == 0 or len(off) < 2:
        raise ValueError("no descriptors to train on")
    if n >= 1 << 31:
        raise ValueError("more than 2^31 descriptors")
    if np.diff(off).max() > IMAGE_MAX:
        raise ValueError(f"at most {IMAGE_MAX} descriptors per image")
    ctx = ctx or default_context()
    lib, h = ctx.lib, ctx.handle
    node_desc, child_begin, child_count = [np.zeros((1, 32), np.uint8)], [0], [0]
    n_nodes = 1
    frontier = np.zeros(1, np.int64)                    # node ids of the current depth
    m = _Buffers(ctx)
    try:
        rows = m.up(d)
        row_node, assign, changed = m.up(np.zeros(n, np.int32)), m.new(4 * n), m.new(16)
        perm = m.new(4 * n)
        n_live = n
        for _ in range(depth):
            F = len(frontier)
            if F == 0 or n_live == 0:
                break
            lv = _Buffers(ctx)
            try:
                need = ctypes.c_uint64(0)
                check(lib.slam_bow_train_seed_workspace(n, F, ctypes.byref(need)))
                cent, cc, ws = lv.new(32 * F * k), lv.new(4 * F), lv.new(need.value)
                check(lib.slam_bow_train_seed(h, rows.ptr, n, row_node.ptr, F, k, cent.ptr, cc.ptr, ws.ptr, ws.nbytes))
                key_off, cursor = lv.new(4 * (F + 1)), lv.new(4 * F)
                check(lib.slam_bow_group_keys(h, row_node.ptr, n, F, key_off.ptr, cursor.ptr, perm.ptr))
                bits, rows_of = lv.new(4 * 256 * F * k), lv.new(4 * F * k)
                check(lib.slam_memset(h, assign.ptr, 0xFF, 4 * n))
                moved = ctypes.c_int64(0)
                for _it in range(max_iters):
                    check(lib.slam_bow_train_step(h, rows.ptr, n, row_node.ptr, F, k, cent.ptr, cc.ptr, assign.ptr, perm.ptr, n_live,
                                                  bits.ptr, rows_of.ptr, changed.ptr, 1, ctypes.byref(moved)))
                    if moved.value == 0:
                        break
                check(lib.slam_bow_train_step(h, rows.ptr, n, row_node.ptr, F, k, cent.ptr, cc.ptr, assign.ptr, None, 0, None, None,
                                              changed.ptr, 0, ctypes.byref(moved)))
                own_d = lv.new(4 * F * k)
                check(lib.slam_bow_train_descend(h, row_node.ptr, assign.ptr, n, F, k, own_d.ptr, None))
                own = own_d.download(np.uint32, (F, k))
                count = cc.download(np.int32, (F,))
                centres = cent.download(np.uint8, (F, k, 32))
                # the centres that own rows become children, in centre order; a node of one centre is a leaf
                child = (own > 0) & (count > 1)[:, None]
                kids = child.sum(1)
                nxt = np.full((F, k), -1, np.int32)
                nxt[child] = np.arange(int(kids.sum()), dtype=np.int32)
                begin = n_nodes + np.concatenate([[0], np.cumsum(kids)[:-1]])
                for f in np.flatnonzero(kids):
                    child_begin[frontier[f]], child_count[frontier[f]] = int(begin[f]), int(kids[f])
                node_desc.append(centres[child])
                child_begin.extend([0] * int(kids.sum()))
                child_count.extend([0] * int(kids.sum()))
                frontier = n_nodes + np.arange(int(kids.sum()), dtype=np.int64)
                n_nodes += int(kids.sum())
                n_live = int(own[child].sum())
                nd = lv.up(nxt)
                check(lib.slam_bow_train_descend(h, row_node.ptr, assign.ptr, n, F, k, None, nd.ptr))
                ctx.sync()
            finally:
                lv.free()
        cc_all = np.asarray(child_count, np.int32)
        won = np.full(n_nodes, -1, np.int32)
        leaves = np.flatnonzero(cc_all == 0)
        won[leaves] = np.arange(len(leaves), dtype=np.int32)
        vocab = Vocabulary.from_arrays(k, depth, np.concatenate(node_desc), np.asarray(child_begin, np.int32), cc_all, won, np.ones(len(leaves)))
        # N_i: the distinct (image, word) pairs through the vector kernel with unit weights, counted per word on the device
        dv = vocab.upload(ctx)
        try:
            dw, _ = _transform_device(dv, m, rows, n, 0)
            pairs = _vectors_device(dv, m, dw, off, n, dv.idf, True)
            try:
                t, nw = int(pairs.offsets[-1]), len(leaves)
                key_off, cursor, scratch = m.new(4 * (nw + 1)), m.new(4 * nw), m.new(4 * t)
                check(lib.slam_bow_group_keys(h, pairs.device[1].ptr, t, nw, key_off.ptr, cursor.ptr, scratch.ptr))
                images_with = np.diff(key_off.download(np.int32, (nw + 1,))).astype(np.float64)
            finally:
                pairs.free()
        finally:
            vocab.free()
        vocab.idf = np.log(float(len(off) - 1) / images_with)
        return Vocabulary.from_arrays(k, depth, vocab.node_desc, vocab.child_begin, vocab.child_count, vocab.word_of_node, vocab.idf)
    finally:
        m.free()


# ------------------------------------------------------------------------------------------------------------ loop candidates

def detect_loop_candidates(db: BowDatabase, vector, connected: Sequence[int] = (), min_score: float = 0.0):
    """The first stage of ORB-SLAM's ``DetectLoopCandidates``: the database entries that share words with ``vector`` (one
    BoW vector), without the ``connected`` ids (the keyframe's covisibility neighbours), kept when they share more than 0.8 of
    the largest shared-word count and score at least ``min_score`` -> (ids int32, scores f64) by (score descending, id
    ascending).  The covisibility-group accumulation and the consistency check over consecutive keyframes are
    ``slamhip.loop_detect``'s (``loop_candidates``, ``LoopConsistency``); this function stays the first stage alone."""
    v = _as_vectors(vector)
    if len(v) != 1:
        raise ValueError("detect_loop_candidates takes one vector")
    if not min_score >= 0.0:
        raise ValueError("min_score must be >= 0")
    s, c = db.scores_dense(v)
    s, c = s[0], c[0].copy()
    conn = np.asarray(list(connected), np.int64).reshape(-1)
    if len(conn) and (conn.min() < 0 or conn.max() >= len(c)):
        raise ValueError("a connected id is not in the database")
    c[conn] = 0
    if len(c) == 0 or c.max() == 0:
        return np.zeros(0, np.int32), np.zeros(0)
    score = s.astype(np.float64) / Q_ONE
    ids = np.flatnonzero((c > 0.8 * c.max()) & (score >= min_score))
    ids = ids[np.lexsort((ids, -s[ids].astype(np.int64)))]
    return ids.astype(np.int32), score[ids]
