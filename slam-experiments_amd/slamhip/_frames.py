"""The host side that the one-launch refinements of a batch of frames share (``optimize_poses_batch``,
``optimize_poses_stereo``): poses to rows, per-frame arrays to one array with an offsets table, the device buffers of one call
with a guaranteed free, and the download split into one ``PoseOptResult`` per frame.  Argument checks, error messages and the
library call stay with each function."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np


@dataclass
class PoseOptResult:
    pose: np.ndarray          # 4x4 Tcw after the last round
    inliers: np.ndarray       # bool [O]: chi2 <= threshold after the last round
    chi2: np.ndarray          # [O] at the returned pose
    n_inliers: int            # what _correct_current_pose returns (frontend.py:393)
    iterations: int           # accepted LM steps over all rounds


def pose_rows(poses) -> np.ndarray:
    """``poses`` [B,4,4] (or [B,3,4]) as contiguous f64 [B,12] rows (3x4, row-major)."""
    P = np.asarray(poses, np.float64)
    B = P.shape[0]
    return np.ascontiguousarray(P.reshape(B, -1, 4)[:, :3, :4].reshape(B, 12))


def refine_frames(ctx, pin, counts, columns, stats_cols: int, call):
    """One launch over B frames.  ``pin`` [B,12]; ``counts[b]`` the edges of frame b; ``columns`` a list of (the B per-frame
    arrays [O_b, w], w), uploaded concatenated in this order; ``call(d_pose, d_columns, d_off, O, d_out, d_inl, d_chi, d_st)``
    makes the library call on the device buffers (``d_st`` holds ``stats_cols`` int32 per frame, of which the first two are
    the inlier count and the accepted steps).  Returns (list of ``PoseOptResult``, stats int32 [B, stats_cols])."""
    B = len(pin)
    off = np.zeros(B + 1, np.int32)
    off[1:] = np.cumsum(counts)
    O = int(off[-1])
    bufs = []
    try:
        up = lambda a: bufs.append(ctx.upload(a)) or bufs[-1]          # noqa: E731
        new = lambda n: bufs.append(ctx.malloc(n)) or bufs[-1]         # noqa: E731
        d_pose, d_off = up(pin), up(off)
        d_cols = [up(np.concatenate(arrays) if O else np.zeros((1, w))) for arrays, w in columns]
        d_out, d_inl, d_chi, d_st = new(B * 96), new(max(O, 1)), new(max(O, 1) * 8), new(B * 4 * stats_cols)
        call(d_pose, d_cols, d_off, O, d_out, d_inl, d_chi, d_st)
        out = d_out.download(np.float64, (B, 3, 4))
        inl = d_inl.download(np.uint8, (max(O, 1),)).astype(bool)
        chi = d_chi.download(np.float64, (max(O, 1),))
        st = d_st.download(np.int32, (B, stats_cols))
    finally:
        for b in bufs:
            b.free()
    res = []
    for b in range(B):
        T = np.eye(4)
        T[:3, :4] = out[b]
        a, e = int(off[b]), int(off[b + 1])
        res.append(PoseOptResult(pose=T, inliers=inl[a:e].copy(), chi2=chi[a:e].copy(), n_inliers=int(st[b, 0]), iterations=int(st[b, 1])))
    return res, st
