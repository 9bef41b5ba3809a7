"""What the wrappers of the pair-table searches (``bow_match``, ``proj_match``, ``tri_match``, ``fuse``) share in front of and
behind a call: the temporaries of a call, the checks of offsets, descriptor rows, pairs, integer and f64 rows and poses, and the
download of a per-pair table.  Private; the modules import what they use from here."""
from __future__ import annotations

from typing import List, Optional

import numpy as np

from .device import Context, DeviceBuffer
from .matching import as_descriptors

PAIRS_MAX, N_BINS = 4096, 32


class _Buffers:
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


def _offsets(offsets, n: int, name: str = "offsets") -> np.ndarray:
    off = np.asarray(offsets)
    if off.dtype.kind not in "iu" or off.ndim != 1 or len(off) < 1:
        raise ValueError(f"{name} must be integers of shape [B + 1]")
    off = np.ascontiguousarray(off, np.int64)
    if off[0] != 0 or off[-1] != n or (np.diff(off) < 0).any():
        raise ValueError(f"{name} must ascend from 0 to {n}")
    return off


def _rows_arg(descriptors):
    """(rows, n) of a descriptor argument, checked: host rows u8 [n,32], or a ``(DeviceBuffer, n)`` pair as it is."""
    if isinstance(descriptors, tuple) and len(descriptors) == 2 and isinstance(descriptors[0], DeviceBuffer):
        buf, n = descriptors[0], int(descriptors[1])
        if n < 0 or n * 32 > buf.nbytes:
            raise ValueError(f"{n} rows do not fit a device buffer of {buf.nbytes} bytes")
        return buf, n
    d = as_descriptors(descriptors)
    return d, len(d)


def _device_rows(ctx: Context, m: _Buffers, rows) -> DeviceBuffer:
    """The rows of ``_rows_arg`` on the device of ``ctx``: host rows are uploaded."""
    if isinstance(rows, DeviceBuffer):
        if rows.ctx is not ctx:
            raise ValueError("the device rows belong to another context")
        return rows
    return m.up(rows)


def _pairs_arg(pairs, B1: int, B2: int) -> np.ndarray:
    p = np.asarray(pairs)
    if p.size == 0:
        return np.zeros((0, 2), np.int32)
    if p.dtype.kind not in "iu" or p.ndim != 2 or p.shape[1] != 2:
        raise ValueError(f"pairs must be integers of shape [P, 2], got {p.dtype} {p.shape}")
    if len(p) > PAIRS_MAX:
        raise ValueError(f"at most {PAIRS_MAX} pairs per call")
    if p.min() < 0 or p[:, 0].max() >= B1 or p[:, 1].max() >= B2:
        raise ValueError(f"pairs name images outside the two sets ({B1} and {B2} images)")
    return np.ascontiguousarray(p, np.int32)


def _int_rows(a, n: int, name: str, lo: int, hi: int, kinds: str = "iub", must: Optional[str] = None) -> np.ndarray:
    """One integer in [lo, hi) per row of a whole set, in row order: one array, or a list of one array per image.  ``kinds``:
    the dtype kinds taken (levels and marks may be booleans, bins and ids not); ``must``: how the range reads in the error."""
    if isinstance(a, (list, tuple)) and len(a) and not np.isscalar(a[0]):
        a = np.concatenate([np.asarray(x).reshape(-1) for x in a])
    a = np.asarray(a)
    if a.size == 0:
        a = np.zeros(0, np.int64)
    if a.dtype.kind not in kinds or a.shape != (n,):
        raise ValueError(f"{name} must be integers of shape [{n}], got {a.dtype} {a.shape}")
    if n and (a.min() < lo or a.max() >= hi):
        raise ValueError(f"{name} must {must or f'lie in [{lo}, {hi})'}")
    return a


def _bins_arg(bins, n: int, name: str) -> Optional[np.ndarray]:
    """Orientation bins of a whole set in row order as uint8 [n], or None."""
    return None if bins is None else np.ascontiguousarray(_int_rows(bins, n, name, 0, N_BINS, "iu"), np.uint8)


def _f64_rows(a, n: int, k: int, name: str) -> np.ndarray:
    a = np.asarray(a, np.float64)
    if a.size == 0 and n == 0:
        return np.zeros((0, k))
    if a.shape != (n, k) and not (k == 1 and a.shape == (n,)):
        raise ValueError(f"{name} must have shape [{n}, {k}], got {a.shape}")
    return np.ascontiguousarray(a.reshape(n, k))


def _poses_arg(poses, P: int) -> np.ndarray:
    a = np.asarray(poses, np.float64)
    if P == 0:
        return np.zeros((0, 3, 4))
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or a.shape[0] != P or a.shape[1:] not in ((3, 4), (4, 4)):
        raise ValueError(f"poses must have shape [{P},3,4] or [{P},4,4], got {a.shape}")
    return np.ascontiguousarray(a[:, :3, :])


def _split(flat: np.ndarray, sizes: np.ndarray) -> List[np.ndarray]:
    ends = np.cumsum(sizes)
    return [flat[e - s:e].copy() for s, e in zip(sizes, ends)]


def _down(buf, dtype, shape: tuple, total: int) -> np.ndarray:
    """A device table of ``total`` rows of ``shape`` on the host (nothing is read for no rows)."""
    return buf.download(dtype, (total,) + shape) if total else np.zeros((0,) + shape, dtype)


def _down_split(buf, dtype, shape: tuple, total: int, sizes) -> List[np.ndarray]:
    """The table of ``_down`` as one array per pair."""
    return _split(_down(buf, dtype, shape, total), sizes)
