"""Node-constrained matching over the BoW direct index (``slam_bow_match_*``): ORB-SLAM's
``ORBmatcher::SearchByBoW`` - the correspondences of candidate image pairs, comparing only the features that
``bow_transform(..., levels_up)`` put into the same vocabulary node - as the step between ``detect_loop_candidates`` and
``solve_pnp_ransac_batch`` / ``estimate_sim3_batch``.

The reference has no call site (it detects no loops).  PARITY UNPINNED: the one-to-one step keeps, among the rows that name
one side-2 row, the smallest (distance, side-1 row) where ORB-SLAM's sequential loop depends on its iteration order, and the
rotation check is stated on this project's 32 integer orientation bins.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Tuple

import numpy as np

from ._args import N_BINS, PAIRS_MAX, _Buffers, _bins_arg, _device_rows, _down_split, _offsets, _pairs_arg, _rows_arg
from ._lib import BowGroups, addr, check, load
from .bow import _levels_up, _transform_device
from .device import Context, DeviceBuffer, default_context
from .matching import as_descriptors

ROWS_MAX, NO_SECOND = 8192, 256
TH_LOW, RATIO = 50, 0.75           # ORBmatcher::TH_LOW and the nnratio of the loop-closing and relocalisation calls
LEVELS_UP = 4


def limits() -> dict:
    """The library's limits (``slam_bow_match_limits``); needs no GPU."""
    lim = (ctypes.c_int32 * 6)()
    check(load().slam_bow_match_limits(lim))
    assert (lim[0], lim[1], lim[4], lim[5]) == (ROWS_MAX, PAIRS_MAX, N_BINS, NO_SECOND), "the library's limits are not this module's"
    return {"rows_per_image": lim[0], "pairs_per_call": lim[1], "group_threads": lim[2], "scan_lanes": lim[3], "bins": lim[4],
            "no_second": lim[5]}


def plan_describe(B: int, n: int) -> dict:
    """The launch plan for ``B`` images or pairs of ``n`` rows per image, WITHOUT a device (``slam_bow_match_plan_describe``)."""
    plan = (ctypes.c_int64 * 8)()
    check(load().slam_bow_match_plan_describe(int(B), int(n), plan))
    names = ("sort_length", "group_lds_bytes", "group_blocks", "scan_blocks", "finish_blocks", "workspace_bytes", "finish_lds_bytes",
             "group_workspace_bytes")
    return dict(zip(names, plan))


def _nodes_arg(nodes, n: int, name: str) -> np.ndarray:
    a = np.asarray(nodes)
    if a.dtype.kind not in "iu" or a.shape != (n,):
        raise ValueError(f"{name} must be integers of shape [{n}], got {a.dtype} {a.shape}")
    if n and (a.min() < -(1 << 31) or a.max() >= 1 << 31):
        raise ValueError(f"{name} must fit 32 bits")
    return np.ascontiguousarray(a, np.int32)


def _image_offsets(offsets, n: int) -> np.ndarray:
    off = _offsets(offsets, n)
    if len(off) > 1 and np.diff(off).max() > ROWS_MAX:
        raise ValueError(f"at most {ROWS_MAX} rows per image")
    return off


class FeatureVectors:
    """DBoW2's ``FeatureVector`` of B images in grouped form: image b owns the positions ``[offsets[b], offsets[b+1])``; inside
    an image the rows are sorted by (node id as unsigned 32-bit, row) - node -> ascending feature indices, masked (negative)
    ids last.  ``order`` int32 [n] is the row (local to its image) at each position and ``nodes_sorted`` int32 [n] its node
    id; both are read from the device when asked for.  The grouped descriptors, the two arrays and the inverse of ``order``
    stay resident until ``free`` (``keep_on_device=False``: on the host, uploaded again by every search)."""

    def __init__(self, ctx: Context, offsets: np.ndarray, device: Tuple[DeviceBuffer, ...]):
        self.ctx, self.offsets = ctx, offsets
        self.device: Optional[Tuple[DeviceBuffer, ...]] = device     # (descriptors, nodes, order, inverse) in grouped order
        self._host = None

    def __len__(self) -> int:
        return len(self.offsets) - 1

    @property
    def n(self) -> int:
        return int(self.offsets[-1])

    def _read(self, which: int, dtype, shape) -> np.ndarray:
        if self._host is not None:
            return self._host[which].copy()
        if self.device is None:
            raise ValueError("these feature vectors have been freed")
        return self.device[which].download(dtype, shape) if self.n else np.zeros(shape, dtype)

    @property
    def descriptors_sorted(self) -> np.ndarray:
        return self._read(0, np.uint8, (self.n, 32))

    @property
    def nodes_sorted(self) -> np.ndarray:
        return self._read(1, np.int32, (self.n,))

    @property
    def order(self) -> np.ndarray:
        return self._read(2, np.int32, (self.n,))

    def to_host(self) -> "FeatureVectors":
        """Move the grouped form to the host and release the device memory."""
        if self.device is not None:
            self._host = tuple(self._read(i, dt, sh) for i, (dt, sh) in enumerate(
                ((np.uint8, (self.n, 32)), (np.int32, (self.n,)), (np.int32, (self.n,)), (np.int32, (self.n,)))))
            self.free()
        return self

    def _resident(self, ctx: Context, m: _Buffers) -> Tuple[DeviceBuffer, ...]:
        if self.device is not None:
            if self.ctx is not ctx:
                raise ValueError("the feature vectors belong to another context")
            return self.device
        if self._host is None:
            raise ValueError("these feature vectors have been freed")
        return tuple(m.up(a) for a in self._host)

    def free(self) -> None:
        if self.device is not None:
            for b in self.device:
                b.free()
            self.device = None

    @classmethod
    def from_nodes(cls, descriptors, nodes, offsets=None, keep_on_device: bool = True, ctx: Optional[Context] = None) -> "FeatureVectors":
        """Group B images by plain node ids (int [n], one per descriptor row; negative = masked): what
        ``bow_feature_vectors`` does behind the vocabulary's descent.  ``descriptors``: u8 [n,32] or ``(DeviceBuffer, n)``;
        ``nodes``: a host array or a ``DeviceBuffer`` of int32 [n]; ``offsets`` int [B+1] (None: one image)."""
        rows, n = _rows_arg(descriptors)
        off = _image_offsets([0, n] if offsets is None else offsets, n)
        host_nodes = None if isinstance(nodes, DeviceBuffer) else _nodes_arg(nodes, n, "nodes")
        if host_nodes is None and nodes.nbytes < 4 * n:
            raise ValueError(f"{n} node ids do not fit a device buffer of {nodes.nbytes} bytes")
        ctx = ctx or default_context()
        m = _Buffers(ctx)
        try:
            d_rows = _device_rows(ctx, m, rows) if n else None
            d_nodes = (nodes if host_nodes is None else m.up(host_nodes)) if n else None
            return _group(ctx, d_rows, d_nodes, off, keep_on_device)
        finally:
            m.free()


def _group(ctx: Context, d_rows: Optional[DeviceBuffer], d_nodes: Optional[DeviceBuffer], off: np.ndarray, keep: bool) -> FeatureVectors:
    n, B = int(off[-1]), len(off) - 1
    out = tuple(ctx.malloc(max(sz * n, 16)) for sz in (32, 4, 4, 4))
    try:
        if n:
            check(ctx.lib.slam_bow_match_group(ctx.handle, d_rows.ptr, d_nodes.ptr, addr(off), B, out[0].ptr, out[1].ptr, out[2].ptr,
                                               out[3].ptr))
            ctx.sync()                                   # the inputs may be the caller's temporaries
    except BaseException:
        for b in out:
            b.free()
        raise
    fv = FeatureVectors(ctx, off, out)
    return fv if keep else fv.to_host()


def bow_feature_vectors(vocab, descriptors, offsets, levels_up: int = LEVELS_UP, keep_on_device: bool = True,
                        ctx: Optional[Context] = None) -> FeatureVectors:
    """DBoW2's ``transform(features, BowVector, FeatureVector, levelsup)`` for B images, the FeatureVector half:
    ``bow_transform``'s descent (the node of every descriptor ``levels_up`` levels above the leaves) and the group step,
    kept resident.  Image b owns the descriptor rows ``[offsets[b], offsets[b+1])`` (at most 8192 each); ``descriptors`` may
    be a ``(DeviceBuffer, n)`` pair as ``OrbResult.device_descriptors(b)`` returns it: resident rows never cross PCIe."""
    levels_up = _levels_up(levels_up)
    rows, n = _rows_arg(descriptors)
    off = _image_offsets(offsets, n)
    ctx = ctx or default_context()
    m = _Buffers(ctx)
    try:
        if n == 0:
            return _group(ctx, None, None, off, keep_on_device)
        d_rows = _device_rows(ctx, m, rows)
        _, d_nodes = _transform_device(vocab.upload(ctx), m, d_rows, n, levels_up)
        return _group(ctx, d_rows, d_nodes, off, keep_on_device)
    finally:
        m.free()


def _scan_order(scan_order) -> int:
    if scan_order not in (0, 1):
        raise ValueError("scan_order must be 0 (a lane per grouped position) or 1 (a lane per row)")
    return int(scan_order)


def _groups(fv: FeatureVectors, dev, d_bins) -> BowGroups:
    return BowGroups(dev[0].ptr, dev[1].ptr, dev[2].ptr, dev[3].ptr, d_bins.ptr if d_bins is not None else None, addr(fv.offsets), len(fv))


def search_by_bow(fv1: FeatureVectors, fv2: FeatureVectors, pairs, bins1=None, bins2=None, th_low: int = TH_LOW, ratio: float = RATIO,
                  return_tables: bool = False, ctx: Optional[Context] = None, scan_order: int = 0):
    """``ORBmatcher::SearchByBoW`` for P image pairs in one chain of launches.  ``pairs`` int [P, 2] holds
    (image of ``fv1`` = the keyframe side, image of ``fv2`` = the frame side); one frame against its candidates is
    ``[(b, 0) for b in candidates]``.  Per pair: the two nearest same-node rows of every side-1 row, the selection
    ``d0 <= th_low and d0 < ratio * d1`` (a lone candidate: d1 = 256), the one-to-one step (among the rows that name one
    side-2 row the smallest (d0, row) keeps it) and, when ``bins1`` and ``bins2`` are given (orientation bins in [0, 32) of
    every row of the two sets in row order, ``OrbResult.bin``), the rotation histogram with its three maxima.
    Returns (matches12: list of int32 [n1] holding the side-2 row or -1, counts int32 [P]), and with ``return_tables`` also
    the list of the top-2 tables (idx, dist) int32 [n1, 2].  ``scan_order`` is an experiment knob; the result does not
    depend on it."""
    if not isinstance(fv1, FeatureVectors) or not isinstance(fv2, FeatureVectors):
        raise ValueError("search_by_bow takes two FeatureVectors (see bow_feature_vectors, FeatureVectors.from_nodes)")
    p = _pairs_arg(pairs, len(fv1), len(fv2))
    b1, b2 = _bins_arg(bins1, fv1.n, "bins1"), _bins_arg(bins2, fv2.n, "bins2")
    if (b1 is None) != (b2 is None):
        raise ValueError("bins1 and bins2 come together or not at all")
    if isinstance(th_low, bool) or int(th_low) != th_low or not -(1 << 31) <= th_low < 1 << 31:
        raise ValueError("th_low must be an integer")
    ratio = float(ratio)
    if ratio != ratio:
        raise ValueError("ratio is not a number")
    scan_order = _scan_order(scan_order)
    P = len(p)
    sizes = np.diff(fv1.offsets)[p[:, 0]] if P else np.zeros(0, np.int64)
    total = int(sizes.sum())
    if P == 0:
        return ([], np.zeros(0, np.int32), []) if return_tables else ([], np.zeros(0, np.int32))
    ctx = ctx or fv1.ctx
    m = _Buffers(ctx)
    try:
        g1 = _groups(fv1, fv1._resident(ctx, m), m.up(b1) if b1 is not None else None)
        g2 = _groups(fv2, fv2._resident(ctx, m), m.up(b2) if b2 is not None else None)
        d_m, d_c = m.new(4 * total), m.new(4 * P)
        d_i, d_d = (m.new(8 * total), m.new(8 * total)) if return_tables else (None, None)
        check(ctx.lib.slam_bow_match_search(ctx.handle, ctypes.byref(g1), ctypes.byref(g2), addr(p), P, int(th_low), ratio, scan_order,
                                            d_m.ptr, d_c.ptr, d_i.ptr if d_i else None, d_d.ptr if d_d else None))
        counts = d_c.download(np.int32, (P,))
        matches = _down_split(d_m, np.int32, (), total, sizes)
        if not return_tables:
            return matches, counts
        return matches, counts, list(zip(_down_split(d_i, np.int32, (2,), total, sizes), _down_split(d_d, np.int32, (2,), total, sizes)))
    finally:
        m.free()


def node_top2(fv1: FeatureVectors, fv2: FeatureVectors, pairs, ctx: Optional[Context] = None, scan_order: int = 0):
    """The node top-2 alone (``slam_bow_match_top2``): the list of (idx, dist) int32 [n1, 2] of ``search_by_bow``'s pairs."""
    p = _pairs_arg(pairs, len(fv1), len(fv2))
    scan_order = _scan_order(scan_order)
    P = len(p)
    if P == 0:
        return []
    sizes = np.diff(fv1.offsets)[p[:, 0]]
    total = int(sizes.sum())
    ctx = ctx or fv1.ctx
    m = _Buffers(ctx)
    try:
        g1, g2 = _groups(fv1, fv1._resident(ctx, m), None), _groups(fv2, fv2._resident(ctx, m), None)
        d_i, d_d = m.new(8 * total), m.new(8 * total)
        check(ctx.lib.slam_bow_match_top2(ctx.handle, ctypes.byref(g1), ctypes.byref(g2), addr(p), P, scan_order, d_i.ptr, d_d.ptr))
        return list(zip(_down_split(d_i, np.int32, (2,), total, sizes), _down_split(d_d, np.int32, (2,), total, sizes)))
    finally:
        m.free()


def node_match_arrays(query, train, query_nodes, train_nodes, k: int = 2, ctx: Optional[Context] = None,
                      scan_order: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """``knnMatch(query, train, k, mask=W)`` for the node mask W: train row j is a candidate for query row i iff
    ``query_nodes[i] == train_nodes[j] >= 0``.  Returns (idx, dist) int32 [N, k], k in {1, 2}, ordered by (distance, train
    index); missing neighbours (-1, INT32_MAX).  One pair of at most 8192 rows a side; with all node ids equal this is
    ``knn_match_arrays``."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or int(k) not in (1, 2):
        raise ValueError(f"k must be 1 or 2, got {k!r}")
    q, t = as_descriptors(query), as_descriptors(train)
    qn, tn = _nodes_arg(query_nodes, len(q), "query_nodes"), _nodes_arg(train_nodes, len(t), "train_nodes")
    if max(len(q), len(t)) > ROWS_MAX:
        raise ValueError(f"at most {ROWS_MAX} rows per image")
    _scan_order(scan_order)
    ctx = ctx or default_context()
    fq = FeatureVectors.from_nodes(q, qn, ctx=ctx)
    try:
        ft = FeatureVectors.from_nodes(t, tn, ctx=ctx)
        try:
            idx, dist = node_top2(fq, ft, [(0, 0)], ctx, scan_order)[0]
        finally:
            ft.free()
    finally:
        fq.free()
    return np.ascontiguousarray(idx[:, :int(k)]), np.ascontiguousarray(dist[:, :int(k)])


def search_by_bow_descriptors(vocab, descriptors1, descriptors2, bins1=None, bins2=None, levels_up: int = LEVELS_UP, th_low: int = TH_LOW,
                              ratio: float = RATIO, ctx: Optional[Context] = None):
    """``search_by_bow`` for one pair given as descriptors (u8 [n,32] or ``(DeviceBuffer, n)``) and a vocabulary: the descent,
    the group step and the search -> (matches12 int32 [n1], number of matches)."""
    ctx = ctx or default_context()
    n1, n2 = _rows_arg(descriptors1)[1], _rows_arg(descriptors2)[1]
    f1 = bow_feature_vectors(vocab, descriptors1, [0, n1], levels_up, ctx=ctx)
    try:
        f2 = bow_feature_vectors(vocab, descriptors2, [0, n2], levels_up, ctx=ctx)
        try:
            matches, counts = search_by_bow(f1, f2, [(0, 0)], bins1, bins2, th_low, ratio, ctx=ctx)
        finally:
            f2.free()
    finally:
        f1.free()
    return matches[0], int(counts[0])


def match_index_pairs(matches12) -> List[Tuple[np.ndarray, np.ndarray]]:
    """Per pair the (side-1 rows, side-2 rows) int32 arrays of its matches, side-1 ascending: what slices the map points of a
    keyframe and the pixels of the frame into one candidate of ``solve_pnp_ransac_batch`` or ``estimate_sim3_batch``."""
    out = []
    for m12 in matches12:
        i1 = np.flatnonzero(np.asarray(m12) >= 0).astype(np.int32)
        out.append((i1, np.asarray(m12, np.int32)[i1]))
    return out
