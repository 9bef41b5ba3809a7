"""Integer numpy restatement of the ORB specification of DESIGN.md §4d, one function per stage, plus the procedural test images.

Test infrastructure (in the manner of two_view_ref.py): slow, direct, and the truth the device is compared with bit for bit.
Everything is integer arithmetic in int64 except where §4d says otherwise (the level sizes, the quotas and the rounding of the
rotated pattern, which are computed once on the host in float64 and handed to the device and to this file alike).
"""
from __future__ import annotations

import numpy as np

BORDER = 16
RADIUS = 15
N_BINS = 32
# radius-3 Bresenham ring, clockwise on the screen (y down) from 12 o'clock: (dx, dy)
RING = ((0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3),
        (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1), (-2, -2), (-1, -3))
BLUR_TAPS = (1, 6, 15, 20, 15, 6, 1)


# ------------------------------------------------------------------------------------------------ host-side parameters
def level_sizes(H, W, n_levels=8, scale=1.2):
    """(heights, widths) int32 [L]: round(H / s^l), round(W / s^l)."""
    lh = [int(np.rint(H / scale ** l)) for l in range(n_levels)]
    lw = [int(np.rint(W / scale ** l)) for l in range(n_levels)]
    return np.asarray(lh, np.int32), np.asarray(lw, np.int32)


def quotas(n_features, n_levels=8, scale=1.2):
    """ORB's geometric split: n (1 - f) / (1 - f^L) f^l rounded, the last level takes the remainder."""
    if n_levels == 1:
        return np.asarray([n_features], np.int32)
    f = 1.0 / scale
    want = n_features * (1.0 - f) / (1.0 - f ** n_levels)
    q, total = [], 0
    for _ in range(n_levels - 1):
        q.append(int(np.rint(want)))
        total += q[-1]
        want *= f
    q.append(max(n_features - total, 0))
    return np.asarray(q, np.int32)


def angle_boundaries():
    """int64 [32, 2]: direction (x, y) of the boundary at (k + 1/2) 11.25 degrees, scaled by 2^14; the first quadrant is rounded,
    the other three are its exact rotations (x, y) -> (-y, x)."""
    a = np.deg2rad((np.arange(8) + 0.5) * 11.25)
    d = np.zeros((32, 2), np.int64)
    d[:8, 0] = np.rint(16384 * np.cos(a))
    d[:8, 1] = np.rint(16384 * np.sin(a))
    for k in range(8, 32):
        d[k] = (-d[k - 8, 1], d[k - 8, 0])
    return d


def steered_table(pattern):
    """int8 [32, 256, 4]: bins 0..7 are rint of the pattern turned by bin * 11.25 degrees, bins 8..31 exact quarter turns of those."""
    p = np.asarray(pattern, np.float64).reshape(256, 2, 2)
    t = np.zeros((32, 256, 2, 2), np.int64)
    for b in range(8):
        c, s = np.cos(np.deg2rad(b * 11.25)), np.sin(np.deg2rad(b * 11.25))
        t[b, :, :, 0] = np.rint(c * p[:, :, 0] - s * p[:, :, 1])
        t[b, :, :, 1] = np.rint(s * p[:, :, 0] + c * p[:, :, 1])
    for b in range(8, 32):
        t[b, :, :, 0] = -t[b - 8, :, :, 1]
        t[b, :, :, 1] = t[b - 8, :, :, 0]
    return t.reshape(32, 256, 4).astype(np.int8)


# ------------------------------------------------------------------------------------------------------------- stages
def _axis_map(n_dst, n_src):
    """Pixel-centre bilinear source coordinate in 16.16, clamped: (index of the left tap, index of the right tap, 11-bit weight)."""
    i = np.arange(n_dst, dtype=np.int64)
    f = ((2 * i + 1) * n_src * 32768) // n_dst - 32768
    f = np.clip(f, 0, (n_src - 1) << 16)
    i0 = f >> 16
    return i0, np.minimum(i0 + 1, n_src - 1), (f & 0xFFFF) >> 5


def resample(img0, h, w):
    """Level image [h, w] from level 0: weights 2048 - w and w per axis, (sum + 2^21) >> 22."""
    img0 = np.asarray(img0, np.int64)
    y0, y1, wy = _axis_map(h, img0.shape[0])
    x0, x1, wx = _axis_map(w, img0.shape[1])
    wy, wx = wy[:, None], wx[None, :]
    top = img0[y0][:, x0] * (2048 - wx) + img0[y0][:, x1] * wx
    bot = img0[y1][:, x0] * (2048 - wx) + img0[y1][:, x1] * wx
    return ((top * (2048 - wy) + bot * wy + (1 << 21)) >> 22).astype(np.uint8)


def blur(img):
    """7x7 binomial, replicate border: the horizontal pass keeps its exact 14-bit sums, one rounding: (sum + 2048) >> 12."""
    a = np.pad(np.asarray(img, np.int64), 3, mode="edge")
    h, w = img.shape
    hor = sum(BLUR_TAPS[k] * a[:, k:k + w] for k in range(7))
    ver = sum(BLUR_TAPS[k] * hor[k:k + h, :] for k in range(7))
    return ((ver + 2048) >> 12).astype(np.uint8)


def fast_scores(img, t):
    """u8 score map: the largest t' >= t at which the pixel passes FAST-9/16, 0 where it does not or within BORDER of an edge."""
    h, w = img.shape
    out = np.zeros((h, w), np.uint8)
    if h < 2 * BORDER + 1 or w < 2 * BORDER + 1:
        return out
    a = np.asarray(img, np.int64)
    B = BORDER
    p = a[B:h - B, B:w - B]
    d = np.stack([a[B + dy:h - B + dy, B + dx:w - B + dx] - p for dx, dy in RING])
    best = np.full(p.shape, -(1 << 20), np.int64)
    for s in range(16):
        arc = d[[(s + i) % 16 for i in range(9)]]
        best = np.maximum(best, np.maximum(arc.min(0), (-arc).min(0)))
    score = best - 1                       # ring > p + t'  <=>  t' <= ring - p - 1
    out[B:h - B, B:w - B] = np.where(score >= t, score, 0)
    return out


def nms(score):
    """bool map: score > 0 and strictly greater than all 8 neighbours."""
    s = np.pad(np.asarray(score, np.int64), 1)
    h, w = score.shape
    c = s[1:-1, 1:-1]
    keep = c > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                keep &= c > s[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    return keep


def harris(img, ys, xs):
    """int64 R = 25 (a c - b^2) - (a + c)^2 with a, b, c the 7x7 sums of Sobel products at the given pixels."""
    a_img = np.asarray(img, np.int64)
    ys, xs = np.asarray(ys, np.int64), np.asarray(xs, np.int64)
    a = np.zeros(len(ys), np.int64)
    b, c = a.copy(), a.copy()
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            y, x = ys + dy, xs + dx
            ix = (a_img[y - 1, x + 1] + 2 * a_img[y, x + 1] + a_img[y + 1, x + 1]) - (a_img[y - 1, x - 1] + 2 * a_img[y, x - 1] + a_img[y + 1, x - 1])
            iy = (a_img[y + 1, x - 1] + 2 * a_img[y + 1, x] + a_img[y + 1, x + 1]) - (a_img[y - 1, x - 1] + 2 * a_img[y - 1, x] + a_img[y - 1, x + 1])
            a += ix * ix
            b += ix * iy
            c += iy * iy
    return 25 * (a * c - b * b) - (a + c) ** 2


def level0_position(v, n0, nl):
    """rint(v n0 / nl) with halves up, clamped to the image."""
    v = np.asarray(v, np.int64)
    return np.minimum((2 * v * n0 + nl) // (2 * nl), n0 - 1)


def candidates(img, t, mask0=None, shape0=None):
    """(R, y, x) int64 arrays of the NMS survivors of one level whose level-0 position the mask allows, in raster order."""
    ys, xs = np.nonzero(nms(fast_scores(img, t)))
    if mask0 is not None:
        H0, W0 = shape0 if shape0 is not None else mask0.shape
        ok = mask0[level0_position(ys, H0, img.shape[0]), level0_position(xs, W0, img.shape[1])] != 0
        ys, xs = ys[ok], xs[ok]
    return harris(img, ys, xs), ys.astype(np.int64), xs.astype(np.int64)


def select(R, ys, xs, quota):
    """Indices of the best `quota` under (R descending, y ascending, x ascending), in that order."""
    return np.lexsort((xs, ys, -np.asarray(R, np.int64)))[:max(int(quota), 0)]


def moments(img, ys, xs):
    """(m10, m01) = sums of x I and y I over the disc x^2 + y^2 <= 15^2."""
    a = np.asarray(img, np.int64)
    ys, xs = np.asarray(ys, np.int64), np.asarray(xs, np.int64)
    m10, m01 = np.zeros(len(ys), np.int64), np.zeros(len(ys), np.int64)
    for dy in range(-RADIUS, RADIUS + 1):
        for dx in range(-RADIUS, RADIUS + 1):
            if dx * dx + dy * dy <= RADIUS * RADIUS:
                v = a[ys + dy, xs + dx]
                m10 += dx * v
                m01 += dy * v
    return m10, m01


def orientation_bin(m10, m01):
    """Bin b holds the directions from boundary b-1 (included) to boundary b (excluded); (0, 0) goes to bin 0."""
    d = angle_boundaries()
    m10, m01 = np.atleast_1d(np.asarray(m10, np.int64)), np.atleast_1d(np.asarray(m01, np.int64))
    cross = d[:, 0][:, None] * m01[None, :] - d[:, 1][:, None] * m10[None, :]        # [32, n], >= 0: at or past the boundary
    out = np.zeros(len(m10), np.int64)
    for b in range(32):
        out[(cross[(b - 1) % 32] >= 0) & (cross[b] < 0)] = b
    return out


def describe(blurred, ys, xs, bins, table):
    """u8 [n, 32]: bit j = blur[y + ay, x + ax] < blur[y + by, x + bx], first test in the least significant bit of byte 0."""
    a = np.asarray(blurred, np.int64)
    ys, xs = np.asarray(ys, np.int64)[:, None], np.asarray(xs, np.int64)[:, None]
    t = np.asarray(table, np.int64)[np.asarray(bins, np.int64)]                        # [n, 256, 4]
    bits = a[ys + t[:, :, 1], xs + t[:, :, 0]] < a[ys + t[:, :, 3], xs + t[:, :, 2]]
    return np.packbits(bits.astype(np.uint8).reshape(len(bits), 32, 8), axis=2, bitorder="little").reshape(len(bits), 32)


def pyramid(img0, lh, lw):
    return [np.asarray(img0, np.uint8) if l == 0 else resample(img0, int(lh[l]), int(lw[l])) for l in range(len(lh))]


def extract(img0, lh, lw, quota, t, table, mask0=None):
    """One image through every stage.  Returns a dict of arrays ordered by (level, R desc, y, x): x, y, level, bin (int64),
    response (int64), descriptors u8 [n, 32]; plus 'stages', per level (image, blurred, scores, (R, y, x) candidates)."""
    out = {k: [] for k in ("x", "y", "level", "bin", "response", "descriptors")}
    stages = []
    for l, img in enumerate(pyramid(img0, lh, lw)):
        blurred = blur(img)
        scores = fast_scores(img, t)
        R, ys, xs = candidates(img, t, mask0, np.asarray(img0).shape)
        stages.append((img, blurred, scores, (R, ys, xs)))
        keep = select(R, ys, xs, quota[l])
        R, ys, xs = R[keep], ys[keep], xs[keep]
        bins = orientation_bin(*moments(img, ys, xs))
        out["x"].append(xs)
        out["y"].append(ys)
        out["level"].append(np.full(len(xs), l, np.int64))
        out["bin"].append(bins)
        out["response"].append(R)
        out["descriptors"].append(describe(blurred, ys, xs, bins, table))
    res = {k: np.concatenate(v) for k, v in out.items()}
    res["descriptors"] = res["descriptors"].reshape(-1, 32)
    res["stages"] = stages
    return res


# ------------------------------------------------------------------------------------------------------ test images
class _Lcg:
    """A 64-bit linear congruential generator (Knuth's MMIX constants): the images do not depend on any library's stream."""

    def __init__(self, seed):
        self.s = (int(seed) * 2654435761 + 1) & ((1 << 64) - 1)

    def below(self, n):
        self.s = (self.s * 6364136223846793005 + 1442695040888963407) & ((1 << 64) - 1)
        return int((self.s >> 33) % n)


def scene(h, w, seed=0, shapes=24):
    """Overlapping rectangles, discs and ramps of differing contrast on a soft ramp, u8 [h, w]."""
    g = _Lcg(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    img = 90 + (40 * xx) // max(w, 1) + (30 * yy) // max(h, 1)
    for _ in range(shapes):
        kind, level = g.below(3), 20 + g.below(216)
        cy, cx = g.below(h), g.below(w)
        ry, rx = 3 + g.below(max(h // 6, 4)), 3 + g.below(max(w // 6, 4))
        if kind == 0:
            inside = (abs(yy - cy) <= ry) & (abs(xx - cx) <= rx)
            img = np.where(inside, level, img)
        elif kind == 1:
            inside = (yy - cy) ** 2 + (xx - cx) ** 2 <= min(ry, rx) ** 2
            img = np.where(inside, level, img)
        else:
            inside = (abs(yy - cy) <= ry) & (abs(xx - cx) <= rx)
            img = np.where(inside, (level + (120 * (xx - cx + rx)) // (2 * rx + 1)) % 256, img)
    return np.clip(img, 0, 255).astype(np.uint8)


def noise(h, w, seed=0):
    """Uniform noise u8 [h, w] from a 32-bit integer hash of the pixel index (no generator state)."""
    i = (np.arange(h * w, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    i = ((i ^ (i >> np.uint64(16))) * np.uint64(0x7FEB352D)) & np.uint64(0xFFFFFFFF)
    i = ((i ^ (i >> np.uint64(15))) * np.uint64(0x846CA68B)) & np.uint64(0xFFFFFFFF)
    i = i ^ (i >> np.uint64(16))
    return (i >> np.uint64(24)).astype(np.uint8).reshape(h, w)


def tiled_noise(h, w, period=32, seed=0):
    """A noise tile repeated with the given period: identical neighbourhoods, so many candidates tie exactly on R."""
    t = noise(period, period, seed)
    return np.tile(t, (h // period + 1, w // period + 1))[:h, :w].copy()
