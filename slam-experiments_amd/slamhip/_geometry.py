"""What the wrappers of the batched RANSAC estimators (``two_view``, ``pnp``, ``homography``, ``sim3``, ``sim3_opt``) share in
front of and behind a call: the checks of intrinsics, RANSAC arguments, point arrays and candidate offsets, the concatenation
of a list of candidates, one RANSAC call from upload to download, the mask of a call and its split - and the pieces of the
loop-edge builders (``pose_graph``, ``pnp``, ``sim3``, ``sim3_graph``).  Private; the modules import what they use from here."""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

from ._args import _Buffers
from ._lib import check
from .device import default_context

MAX_HYPOTHESES = 1 << 20
MAX_PAIRS = 65535
MAX_TOTAL = 1 << 28             # correspondences of one call


def _intrinsics(K) -> Tuple[float, float, float, float]:
    """(fx, fy, cx, cy) from a 3x3 camera matrix or a 4-sequence."""
    A = np.asarray(K, np.float64)
    if A.shape == (3, 3):
        vals = (A[0, 0], A[1, 1], A[0, 2], A[1, 2])
    elif A.shape == (4,):
        vals = tuple(A)
    else:
        raise ValueError(f"intrinsics must be a 3x3 camera matrix or (fx, fy, cx, cy), got shape {A.shape}")
    fx, fy, cx, cy = (float(v) for v in vals)
    if not (np.isfinite([fx, fy, cx, cy]).all() and fx > 0 and fy > 0):
        raise ValueError("focal lengths must be positive and intrinsics finite")
    return fx, fy, cx, cy


def _check_ransac_args(hypotheses, threshold, seed):
    if not isinstance(hypotheses, (int, np.integer)) or isinstance(hypotheses, bool):
        raise TypeError("hypotheses must be an integer")
    if not 1 <= int(hypotheses) <= MAX_HYPOTHESES:
        raise ValueError(f"hypotheses must be in [1, {MAX_HYPOTHESES}]")
    if not (np.isfinite(threshold) and threshold > 0):
        raise ValueError("threshold must be positive")
    if not isinstance(seed, (int, np.integer)) or isinstance(seed, bool):
        raise TypeError("seed must be an integer")
    return int(hypotheses), float(threshold), int(seed) & ((1 << 64) - 1)


def _numeric(a, name: str) -> np.ndarray:
    try:
        return np.asarray(a, np.float64)
    except (TypeError, ValueError) as exc:
        raise TypeError(f"{name} must be numeric") from exc


def _points(a, name: str, k: int = 2) -> np.ndarray:
    """f64 [N,k] of any N (nothing of any shape is no points)."""
    a = _numeric(a, name)
    if a.size == 0:
        return np.zeros((0, k))
    if a.ndim != 2 or a.shape[1] != k:
        raise ValueError(f"{name} must have shape [N,{k}], got {a.shape}")
    return np.ascontiguousarray(a)


def _rows(a, N: int, name: str, k: int = 2) -> np.ndarray:
    """f64 [N,k] of the N rows another array has (pixels, squared sigmas)."""
    a = _numeric(a, name)
    if a.size == 0 and N == 0:
        return np.zeros((0, k))
    if a.shape != (N, k):
        raise ValueError(f"{name} must have shape [{N},{k}], got {a.shape}")
    return np.ascontiguousarray(a)


def _pair(a, b, name_a: str, name_b: str, k: int, total: str = ""):
    """Two [N,k] arrays of one length; ``total``: what the 2^28 limit counts, where the wrapper has one of its own."""
    a, b = _points(a, name_a, k), _points(b, name_b, k)
    if len(a) != len(b):
        raise ValueError(f"{len(a)} points in frame 1 but {len(b)} in frame 2")
    if total and len(a) >= MAX_TOTAL:
        raise ValueError(f"more than 2^28 {total} in one call")
    return a, b


def _check_cap(B: int, cap: int, what: str):
    if B > cap:
        raise ValueError(f"at most {cap} {what} per call")


def _cand_offsets(offsets, cap: int, what: str):
    """(int32 offsets [B + 1], B) of a call of at most ``cap`` candidates; ``what`` is how the wrapper calls them."""
    offsets = np.ascontiguousarray(offsets, np.int32).reshape(-1)
    B = len(offsets) - 1
    if B < 0:
        raise ValueError("offsets must have B + 1 entries")
    _check_cap(B, cap, what)
    return offsets, B


def _concat(cands, what: str, fields, total: str, mismatch: str = "{} points in frame 1 but {} in frame 2", sigma2: bool = False):
    """A list of candidates as concatenated arrays and int32 offsets [B + 1]: ``(*arrays, offsets)``.

    ``fields``: (name, width) of every array of a candidate.  The first two are [N,k] of one length N, or ``mismatch`` says so;
    the others must have exactly N rows.  With ``sigma2`` a candidate may end in an [N,2] of squared sigmas (ones where it has
    none), returned in front of the offsets - as None when no candidate has any.  ``what`` is how the wrapper calls a candidate,
    ``total`` what its 2^28 limit counts."""
    names = ", ".join(n for n, _ in fields)
    expected = f"({names}) or ({names}, sigma2)" if sigma2 else f"({names})"
    widths = [k for _, k in fields] + [2] * sigma2
    cols, off, any_sigma = [[] for _ in widths], [0], False
    for i, c in enumerate(cands):
        if not len(fields) <= len(c) <= len(widths):
            raise ValueError(f"{what} {i}: expected {expected}")
        row = [_points(c[j], f"{what} {i} {n}", k) for j, (n, k) in enumerate(fields[:2])]
        N = len(row[0])
        if N != len(row[1]):
            raise ValueError(f"{what} {i}: " + mismatch.format(N, len(row[1])))
        row += [_rows(c[j], N, f"{what} {i} {n}", k) for j, (n, k) in enumerate(fields) if j >= 2]
        if sigma2:
            has = len(c) == len(widths) and c[-1] is not None
            any_sigma = any_sigma or has
            row.append(_rows(c[-1], N, "sigma2") if has else np.ones((N, 2)))
        for col, a in zip(cols, row):
            col.append(a)
        off.append(off[-1] + N)
    if off[-1] >= MAX_TOTAL:
        raise ValueError(f"more than 2^28 {total} in one call")
    out = [np.concatenate(v) if v else np.zeros((0, k)) for v, k in zip(cols, widths)]
    if sigma2 and not any_sigma:
        out[-1] = None
    return (*out, np.asarray(off, np.int32))


def _pair_arrays(pairs):
    """(px1 [M,2], px2 [M,2], int32 offsets [B + 1]) of a list of ``(px1, px2)`` pairs of matched pixels."""
    return _concat(pairs, "pair", (("px1", 2), ("px2", 2)), "matches")


def _concat_flags(flags, B: int):
    """One uint8 array of a list of per-candidate masks, or None."""
    if flags is None:
        return None
    if len(flags) != B:
        raise ValueError("one inlier mask per pair")
    return np.concatenate([np.asarray(v).astype(np.uint8).reshape(-1) for v in flags]) if len(flags) else np.zeros(0, np.uint8)


def _flags(flags, M: int):
    """uint8 [M] of one flag per correspondence, or None."""
    if flags is None:
        return None
    flags = np.ascontiguousarray(flags).astype(np.uint8).reshape(-1)
    if len(flags) != M:
        raise ValueError("one inlier flag per match")
    return flags


def _mask_down(buf, M: int) -> np.ndarray:
    """The M bytes of a call's mask as bool (nothing is read for M == 0)."""
    return buf.download(np.uint8, (M,)).astype(bool) if M else np.zeros(0, bool)


def _split_mask(mask: np.ndarray, off) -> List[np.ndarray]:
    return [mask[off[b]:off[b + 1]].copy() for b in range(len(off) - 1)]


def _solve_samples(ctx, name: str, a, b, shape: tuple, *extra):
    """One minimal-solver call ``name(handle, S, a, b, *extra, models, counts)`` on S > 0 samples:
    (models f64 [S, *shape], counts int32 [S])."""
    S = len(a)
    m = _Buffers(ctx or default_context())
    try:
        da, db = m.up(a), m.up(b)
        dm, dn = m.new(S * int(np.prod(shape)) * 8), m.new(S * 4)
        check(getattr(m.ctx.lib, name)(m.ctx.handle, S, da.ptr, db.ptr, *extra, dm.ptr, dn.ptr))
        return dm.download(np.float64, (S,) + shape), dn.download(np.int32, (S,))
    finally:
        m.free()


class _Vote:
    """One RANSAC call ``fn(handle, B, offsets, *arrays, M, *tail, *params, model, mask, stats)`` under the caller's ``_Buffers``:
    the arrays and the offsets uploaded (then ``tail``: arrays that may be None, passed as null), model (``width`` doubles per
    candidate), mask and stats allocated, the call made.  The buffers stay live for a call that follows; ``download`` reads
    model, stats and mask."""

    def __init__(self, m: _Buffers, fn, arrays, offsets, params, width: int, tail=()):
        self.B, self.M, self.width = len(offsets) - 1, len(arrays[0]), width
        self.arrays, self.offsets = [m.up(a) for a in arrays], m.up(offsets)
        tail = [m.up(a) if a is not None else None for a in tail]
        self.model, self.mask, self.stats = m.new(self.B * width * 8), m.new(self.M), m.new(self.B * 16)
        check(fn(m.ctx.handle, self.B, self.offsets.ptr, *(d.ptr for d in self.arrays), self.M, *(d.ptr if d is not None else None for d in tail),
                 *params, self.model.ptr, self.mask.ptr, self.stats.ptr))

    def download(self, *shape):
        """(model f64 [B, *shape], inlier bool [M], stats int32 [B,4])"""
        model, st = self.model.download(np.float64, (self.B,) + (shape or (self.width,))), self.stats.download(np.int32, (self.B, 4))
        return model, _mask_down(self.mask, self.M), st


def _model_srt(model: np.ndarray):
    """(s [B], R [B,3,3], t [B,3]) of Sim(3) models [B,13]."""
    T = model[:, :12].reshape(-1, 3, 4)
    return model[:, 12].copy(), np.ascontiguousarray(T[:, :, :3]), np.ascontiguousarray(T[:, :, 3])


# ---------------------------------------------------------------- loop closures -> edges -------------------------------------
def _edge_pairs(pairs) -> np.ndarray:
    """``pairs`` of a loop-edge builder as integers [B,2]."""
    pairs = np.asarray(pairs)
    if pairs.size == 0:
        pairs = np.zeros((0, 2), np.int64)
    if pairs.dtype.kind not in "iu" or pairs.ndim != 2 or pairs.shape[1] != 2:
        raise ValueError(f"pairs must be integers of shape [B,2], got {pairs.dtype} {pairs.shape}")
    return pairs


def _check_edge_args(min_inliers, *sigmas):
    if min_inliers < 1 or any(s <= 0 for s in sigmas):
        raise ValueError("min_inliers >= 1 and positive sigmas")


def _edge_info(weight: np.ndarray, *sigmas) -> np.ndarray:
    """Diagonal information [E,D,D] of edges weighted ``inliers / min_inliers``: ``weight / sigma^2`` on the three entries of the
    rotation, the three of the translation (sigma None: left zero) and, with a third sigma, the seventh entry of the scale."""
    D = 6 + (len(sigmas) == 3)
    info = np.zeros((len(weight), D, D))
    for block, sigma in enumerate(sigmas):
        for a in range(3 * block, min(3 * block + 3, D)):
            if sigma is not None:
                info[:, a, a] = weight / sigma ** 2
    return info
