"""The numpy statement of stereo matching (``slam_stereo_match``; ORB-SLAM's ``Frame::ComputeStereoMatches``), by
another route than the kernels: every right row against every left row as one boolean matrix (no tiles, no early exits), the
SAD by slicing the planes, the best (SAD, inc) by ``argmin`` over the whole profile, the median by ``np.lexsort``.

A block is a dict: ``count`` int32 [B], ``kp`` int32 [B, N_max, 4] = (x, y, level, bin) in level coordinates, ``desc`` u8
[B, N_max, 32] and ``planes[b][l]`` u8 [h_l, w_l], the pyramid of image ``b``."""
from __future__ import annotations

import numpy as np

MATCHED, NO_CANDIDATE, ORB_DISTANCE, WINDOW, SLIDE_BORDER, DISPARITY, MEDIAN = range(7)
NO_DIST = 256
DEFAULTS = dict(min_d=0.0, th_orb=75, w=5, Ls=5, reject=True)
_POP = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1).astype(np.int32)


def scale_table(scale: float, L: int) -> np.ndarray:
    """h_scale as ``OrbResult`` makes it."""
    return np.float32(scale) ** np.arange(L, dtype=np.float32)


def level0(c, s):
    """The level-0 pixel: one f32 product, promoted."""
    return (np.asarray(c).astype(np.float32) * np.asarray(s, np.float32)).astype(np.float64)


def empty(n):
    return dict(right=np.full(n, -1, np.int32), u_right=np.full(n, np.nan), depth=np.full(n, np.nan), orb_dist=np.full(n, NO_DIST, np.int32),
                sad=np.full(n, -1, np.int32), status=np.full(n, NO_CANDIDATE, np.uint8))


def sad_profile(IL, IR, x, y, c0, w, Ls):
    """SAD(inc) for inc in [-Ls, Ls], int64 [2 Ls + 1]: the caller has made the window test."""
    A = IL[y - w:y + w + 1, x - w:x + w + 1].astype(np.int64) - int(IL[y, x])
    out = np.zeros(2 * Ls + 1, np.int64)
    for k, inc in enumerate(range(-Ls, Ls + 1)):
        c = c0 + inc
        Bm = IR[y - w:y + w + 1, c - w:c + w + 1].astype(np.int64) - int(IR[y, c])
        out[k] = np.abs(A - Bm).sum()
    return out


def match_pair(kpL, descL, planesL, kpR, descR, planesR, scale, bf, max_d, min_d=0.0, th_orb=75, w=5, Ls=5, reject=True, chunk=256):
    """One pair: dict of arrays [nL] (right, u_right, depth, orb_dist, sad, status) and ``counts`` = (status 0, accepted)."""
    kpL, kpR = np.asarray(kpL, np.int64).reshape(-1, 4), np.asarray(kpR, np.int64).reshape(-1, 4)
    descL, descR = np.asarray(descL, np.uint8).reshape(-1, 32), np.asarray(descR, np.uint8).reshape(-1, 32)
    scale = np.asarray(scale, np.float32)
    L, nL, nR = len(scale), len(kpL), len(kpR)
    o = empty(nL)
    bf, min_d, max_d = np.float64(bf), np.float64(min_d), np.float64(max_d)
    okL, okR = (kpL[:, 2] >= 0) & (kpL[:, 2] < L), (kpR[:, 2] >= 0) & (kpR[:, 2] < L)
    lL, lR = np.where(okL, kpL[:, 2], 0), np.where(okR, kpR[:, 2], 0)
    sL, sR = scale[lL], scale[lR]
    uL, vL, uR, vR = level0(kpL[:, 0], sL), level0(kpL[:, 1], sL), level0(kpR[:, 0], sR), level0(kpR[:, 1], sR)
    r = 2.0 * sR.astype(np.float64)
    lo, hi, tv = np.floor(vR - r), np.ceil(vR + r), np.trunc(vL)
    best = np.full(nL, -1, np.int64)
    for i0 in range(0, nL, chunk):                                       # (chunks bound the memory of the distance matrix only)
        s = slice(i0, min(i0 + chunk, nL))
        cand = okL[s, None] & okR[None, :] & (lo[None, :] <= tv[s, None]) & (tv[s, None] <= hi[None, :])
        cand &= (lR[None, :] >= lL[s, None] - 1) & (lR[None, :] <= lL[s, None] + 1)
        cand &= (uR[None, :] >= (uL[s] - max_d)[:, None]) & (uR[None, :] <= (uL[s] - min_d)[:, None]) & ((uL[s] - min_d) >= 0)[:, None]
        if nR == 0:
            continue
        dist = _POP[descL[s, None, :] ^ descR[None, :, :]].sum(-1)
        dist = np.where(cand, dist, NO_DIST + 1)
        j = dist.argmin(1)                                               # the first minimum: the lowest row
        d = dist[np.arange(len(j)), j]
        has = d <= NO_DIST
        best[s] = np.where(has, j, -1)
        o["right"][s] = np.where(has, j, -1)
        o["orb_dist"][s] = np.where(has, d, NO_DIST)
    for i in range(nL):
        j = int(best[i])
        if j < 0:
            continue
        if o["orb_dist"][i] >= th_orb:
            o["status"][i] = ORB_DISTANCE
            continue
        l = int(lL[i])
        IL, IR = planesL[l], planesR[l]
        x, y = int(kpL[i, 0]), int(kpL[i, 1])
        c0 = int(np.floor(uR[j] / np.float64(scale[l]) + np.float64(0.5)))
        h_l, w_l = IL.shape
        if not (c0 - Ls - w >= 0 and c0 + Ls + w + 1 < w_l and x - w >= 0 and x + w < w_l and y - w >= 0 and y + w < h_l):
            o["status"][i] = WINDOW
            continue
        prof = sad_profile(IL, IR, x, y, c0, w, Ls)
        k = int(prof.argmin())                                           # the first minimum: the lowest inc
        o["sad"][i] = prof[k]
        if k == 0 or k == 2 * Ls:
            o["status"][i] = SLIDE_BORDER
            continue
        d1, d2, d3 = int(prof[k - 1]), int(prof[k]), int(prof[k + 1])
        den = d1 + d3 - 2 * d2
        delta = np.float64(0.0) if den == 0 else np.float64(d1 - d3) / np.float64(2 * den)
        u_right = np.float64(scale[l]) * (np.float64(c0 + (k - Ls)) + delta)
        disp = uL[i] - u_right
        if not (disp >= min_d and disp < max_d):
            o["status"][i] = DISPARITY
            continue
        if disp <= 0:
            disp, u_right = np.float64(0.01), uL[i] - np.float64(0.01)
        o["u_right"][i], o["depth"][i], o["status"][i] = u_right, bf / disp, MATCHED
    acc = np.flatnonzero(o["status"] == MATCHED)
    n = len(acc)
    if reject and n:
        order = np.lexsort((acc, o["sad"][acc]))
        m = int(o["sad"][acc][order[n // 2]])
        out = acc[10 * o["sad"][acc].astype(np.int64) >= 21 * m]
        o["status"][out] = MEDIAN
        o["u_right"][out] = np.nan
        o["depth"][out] = np.nan
    o["counts"] = np.asarray([(o["status"] == MATCHED).sum(), n], np.int32)
    return o


KEYS = ("right", "u_right", "depth", "orb_dist", "sad", "status")


def match(pairs, left, right, scale, **params):
    """``slam_stereo_match``: every output as [P, N_max] (slots past the left count are status 1 rows) and ``counts`` [P, 2]."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    n_max = left["kp"].shape[1]
    out = {k: np.stack([empty(n_max)[k] for _ in range(len(pairs))]) if len(pairs) else empty(0)[k].reshape(0, n_max) for k in KEYS}
    out["counts"] = np.zeros((len(pairs), 2), np.int32)
    for p, (a, b) in enumerate(pairs):
        nL, nR = (int(np.clip(blk["count"][i], 0, n_max)) for blk, i in ((left, a), (right, b)))
        o = match_pair(left["kp"][a, :nL], left["desc"][a, :nL], left["planes"][a], right["kp"][b, :nR], right["desc"][b, :nR],
                       right["planes"][b], scale, **params)
        for k in KEYS:
            out[k][p, :nL] = o[k]
        out["counts"][p] = o["counts"]
    return out
