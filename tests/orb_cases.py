"""Edge cases of the ORB extraction of DESIGN.md §4d: the images, masks and parameters of tests/test_orb_edges_cpu.py and
tests/test_orb_edges_gpu.py, with the expectations that can be written down without running anything.

Plain numpy on top of orb_ref.py; the product is not imported here.  A "dot image" is a constant background with single pixels
of another value.  A dot of value fg on background bg, at least 16 pixels from the edge and with no other dot within 8 pixels,
is a FAST corner of score |fg - bg| - 1 (all 16 ring pixels differ from it by |fg - bg|); its Sobel responses are those of one
pixel, a = c = 12 (fg - bg)^2 and b = 0, so R = 25 a c - (a + c)^2 = 3024 (fg - bg)^4.  The background cancels over the
symmetric disc and the dot itself sits at (0, 0), so its moment is the sum of (dx, dy) (value - bg) over the OTHER dots inside
its radius-15 disc: (0, 0), hence bin 0, when the disc holds no other dot.
"""
from __future__ import annotations

import numpy as np

import orb_ref as ref

SEL_THREADS = 1024                     # threads of the selection block: a list longer than this takes several strides


# ------------------------------------------------------------------------------------------- the reference, computed once
_CACHE = {}


def reference(img, P, mask=None):
    """orb_ref.extract for the sizes, quotas, threshold and table of P (an OrbParams, or anything with lh, lw, quota, t, table),
    computed once per distinct input and shared by every test of the session; callers must not modify what they get."""
    img = np.ascontiguousarray(img)
    key = (img.shape, hash(img.tobytes()), None if mask is None else hash(np.ascontiguousarray(mask).tobytes()),
           tuple(P.lh.tolist()), tuple(P.lw.tolist()), tuple(np.asarray(P.quota).tolist()), int(P.t), hash(P.table.tobytes()))
    if key not in _CACHE:
        _CACHE[key] = ref.extract(img, P.lh, P.lw, P.quota, P.t, P.table, mask0=mask)
    return _CACHE[key]


def with_quota(P, quota):
    """A copy of the parameters P with the per-level quotas replaced (the geometric rule cannot give every cut)."""
    import copy

    Q = copy.copy(P)
    Q.quota = np.asarray(quota, np.int32)
    Q.n_max = int(Q.quota.sum())
    return Q


def xy(r):
    """[(x, y)] of a result of the reference, in its order."""
    return list(zip(r["x"].tolist(), r["y"].tolist()))


def per_level(r, L):
    return np.bincount(r["level"], minlength=L).tolist()


# ------------------------------------------------------------------------------------------------------- closed forms
def dot_R(fg, bg=0):
    """Harris response of an isolated dot."""
    return 3024 * (int(fg) - int(bg)) ** 4


def dot_score(fg, bg=0):
    """FAST score of an isolated dot."""
    return abs(int(fg) - int(bg)) - 1


R_255 = 12786229890000                 # dot_R(255, 0), as a literal
assert dot_R(255) == R_255 and dot_score(255) == 254


def dot_image(h, w, dots, bg=0):
    """u8 [h, w] of value bg with img[y, x] = v for every (x, y, v) in dots."""
    img = np.full((h, w), bg, np.uint8)
    for x, y, v in dots:
        img[y, x] = v
    return img


def dot_moment(dots, i, bg=0):
    """(m10, m01) of dot i of a dot image: the other dots inside the radius-15 disc, each (dx, dy) (v - bg)."""
    x0, y0, _ = dots[i]
    m10 = m01 = 0
    for j, (x, y, v) in enumerate(dots):
        dx, dy = x - x0, y - y0
        if j != i and dx * dx + dy * dy <= ref.RADIUS ** 2:
            m10 += dx * (int(v) - bg)
            m01 += dy * (int(v) - bg)
    return m10, m01


def bin_of_direction(m10, m01):
    """The bin of a moment on an axis or a diagonal, from the angle alone: 4 per 45 degrees, y down; (0, 0) -> 0."""
    if m10 == 0 and m01 == 0:
        return 0
    assert m10 == 0 or m01 == 0 or abs(m10) == abs(m01), "only axes and diagonals have a bin one can state without the table"
    octant = {(1, 0): 0, (1, 1): 1, (0, 1): 2, (-1, 1): 3, (-1, 0): 4, (-1, -1): 5, (0, -1): 6, (1, -1): 7}
    return 4 * octant[(int(np.sign(m10)), int(np.sign(m01)))]


# ------------------------------------------------------------------------------------- 1: seams, first / last pixel, capacity
SEAM_H, SEAM_W = 65, 145               # pitch 148; 3 x 5 tiles of 64 x 16, partial on both axes; scoreable x 16..128, y 16..48
SEAM_DOTS = [(16, 16, 255), (63, 16, 255), (64, 31, 255), (128, 32, 255), (16, 48, 255), (128, 48, 255), (127, 40, 255), (128, 24, 255)]
SEAM_ORDER = [(16, 16), (63, 16), (128, 24), (64, 31), (128, 32), (127, 40), (16, 48), (128, 48)]          # (x, y) by (y, x): all R tie
# the bins, by hand: the four dots on the right lie within 15 pixels of their neighbours in the column
#   (128,24): (128,32) below -> (0, +8)            -> +y   -> 8
#   (128,32): (128,24) above, (127,40) at (-1, 8)   -> (-1, 0) -> -x -> 16
#   (127,40): (128,32) at (1,-8), (128,48) at (1,8) -> (+2, 0) -> +x -> 0
#   (128,48): (127,40) at (-1,-8)                   -> not on an axis: left to the reference
SEAM_BINS = [0, 0, 8, 0, 16, 0, 0, None]


def seam_dots():
    return dot_image(SEAM_H, SEAM_W, SEAM_DOTS)


PAIR_DOTS = [(63, 24, 255), (64, 24, 255), (40, 31, 255), (40, 32, 255), (100, 16, 255), (100, 15, 255)]
PAIR_TIED = [(63, 24), (64, 24), (40, 31), (40, 32)]                      # both pixels of each pair score 254, and both drop
PAIR_KEPT = (100, 16)                                                     # its neighbour (100, 15) is in the border: score 0


def seam_pairs():
    return dot_image(SEAM_H, SEAM_W, PAIR_DOTS)


def seam_unequal_pair():
    """255 at (63, 24), 200 at (64, 24): scores 254 and 199, only the first survives."""
    return dot_image(SEAM_H, SEAM_W, [(63, 24, 255), (64, 24, 200)])


def capacity_cases():
    """[(image, number of keypoints = capacity of level 0)]: the two cases that fill the candidate list exactly."""
    return [(dot_image(33, 33, [(16, 16, 255)]), 1),
            (dot_image(35, 35, [(16, 16, 255), (18, 16, 255), (16, 18, 255), (18, 18, 255)]), 4)]


def capacity(h, w):
    """The proven capacity of a level: one survivor per 2 x 2 block of the scoreable region."""
    return ((w - 31) // 2) * ((h - 31) // 2) if h >= 33 and w >= 33 else 0


# ---------------------------------------------------------------------------------------------- 2: degenerate and extreme sizes
TOO_SMALL = [(1, 1), (3, 2), (32, 200), (200, 32), (33, 4), (5, 97)]      # (H, W), n_levels = 3, noise
TOO_SMALL_KW = dict(n_features=50, n_levels=3)
TINY_SCALE4_KW = dict(n_features=50, n_levels=3, scale=4.0)               # 2 x 2: the upper levels round to 0 and are clamped to 1


def too_small_image(h, w):
    return ref.noise(h, w, 13)


STRIP_KW = dict(n_features=20000, n_levels=2)
STRIP_COUNTS = {(40, 8192): 7968, (8192, 40): 8005}


def strip(h, w):
    return ref.noise(h, w, 7)


LEVEL_CASES = {                                                           # on ref.scene(83, 97, 11, shapes=80)
    "sixteen": dict(n_features=500, n_levels=16),                         # levels 6..15 below 33 pixels
    "scale2": dict(n_features=500, n_levels=3, scale=2.0),
    "scale1.05": dict(n_features=500, n_levels=16, scale=1.05),           # weights close to the identity, every level alive
}
SIXTEEN_PER_LEVEL = [37, 35, 28, 13, 5, 1] + [0] * 10


def level_image():
    return ref.scene(83, 97, 11, shapes=80)


# ------------------------------------------------------------------------------------------------------------- 3: selection
def long_list_image():
    return ref.noise(256, 256, 3)


def long_list_quotas(n):
    """Quotas around a list of n > 4096 candidates: both strided loops more than once, one dropped, exact, short, one."""
    return [1100, n - 1, n, n + 500, 1]


def all_tied_image():
    """128 x 128, dots at [4::8, 4::8]: 144 candidates (x, y in 20, 28 .. 108), every R = R_255, every moment (0, 0)."""
    img = np.zeros((128, 128), np.uint8)
    img[4::8, 4::8] = 255
    return img


ALL_TIED_QUOTAS = [1, 50, 143, 144]
ALL_TIED_ORDER = [(x, y) for y in range(20, 109, 8) for x in range(20, 109, 8)]        # (y, x) ascending
assert len(ALL_TIED_ORDER) == 144 and ALL_TIED_ORDER[49] == (28, 52)


def mixed_sign_image():
    return ref.scene(120, 160, 8, shapes=70)


MIXED_SIGN_KW = dict(n_features=3000, n_levels=3)


def quota_above_the_negatives(r):
    """int32 [L]: per level the number of candidates with R >= 0, from a reference result: the quota that cuts between the
    last non-negative R and the first negative one."""
    return np.asarray([int((s[3][0] >= 0).sum()) for s in r["stages"]], np.int32)


SATURATED_RECTS = [(20, 20, 6, 9), (18, 24, 1, 1),        # (y, x, h, w): a dot above a top edge, one black row between
                   (20, 44, 4, 4), (26, 49, 1, 1),        # a dot off the lower right corner
                   (40, 20, 10, 3), (45, 25, 1, 1),       # a dot beside a tall bar
                   (40, 40, 2, 12), (44, 46, 1, 1), (37, 46, 1, 1),
                   (60, 20, 1, 1), (60, 22, 1, 1),        # two dots two apart
                   (60, 40, 1, 1), (63, 40, 1, 1),        # two dots three apart: on each other's ring
                   (72, 22, 1, 1),                        # a lone dot: R_255
                   (70, 40, 5, 5), (68, 37, 1, 1)]
SATURATED_QUOTAS = [1, 2, 9, 21, 22, 30]


def saturated_rectangles():
    """96 x 128 of 0 and 255 only: white axis-aligned rectangles on black, the left half mirrored into the right half, so every
    candidate has a mirror image with the same R (Harris is invariant under x -> -x).  In a saturated image every corner scores
    254, so a rectangle of two or more pixels a side leaves no survivor of its own (its corner pixels are adjacent corners of
    equal score, and strict suppression drops them all); the survivors are the 1 x 1 rectangles, and the ones that stand within
    4 pixels of a larger rectangle take its edge gradients into their 7 x 7 Harris window: R up to twelve times a lone dot's."""
    half = np.zeros((96, 64), np.uint8)
    for y, x, h, w in SATURATED_RECTS:
        half[y:y + h, x:x + w] = 255
    return np.concatenate([half, half[:, ::-1]], axis=1)


# ------------------------------------------------------------------------------------------------- 4: value range, orientation
def threshold_noise():
    return ref.noise(64, 80, 5)


THRESHOLD_DOTS = [(30, 30, 255), (50, 20, 255), (40, 40, 254)]            # at t = 254 the 254-valued dot (score 253) is gone


def threshold_dots():
    return dot_image(64, 80, THRESHOLD_DOTS)


INVERSE_DOTS = [(30, 30, 0), (50, 20, 0)]


def inverse_dots():
    """Dots of 0 on 255: every ring pixel is brighter by 255, the 'brighter' arc at p + t = 254."""
    return dot_image(64, 80, INVERSE_DOTS, bg=255)


AXIS_BINS = [0, 4, 8, 12, 16, 20, 24, 28]


def axis_batch():
    """u8 [8, 65, 65]: a 255 dot at (32, 32) and a 3 x 3 patch of 60 ten pixels away at 0, 45 .. 315 degrees (y down):
    the moment is 540 (dx, dy), exactly on an axis or a diagonal."""
    out = np.zeros((8, 65, 65), np.uint8)
    for k in range(8):
        a = np.deg2rad(45.0 * k)
        cx, cy = 32 + int(np.rint(10 * np.cos(a))), 32 + int(np.rint(10 * np.sin(a)))
        out[k, cy - 1:cy + 2, cx - 1:cx + 2] = 60
        out[k, 32, 32] = 255
    return out


AXIS_KW = dict(n_features=10, n_levels=1, fast_threshold=100)


# --------------------------------------------------------------------------------------------------------------------- 5: mask
def mask_image():
    return ref.noise(96, 112, 9)


MASK_KW = dict(n_features=5000, n_levels=4)


def checkerboard(h=96, w=112, value=7):
    yy, xx = np.mgrid[0:h, 0:w]
    return (((yy + xx) % 2) * value).astype(np.uint8)


def checkerboard_inverse(h=96, w=112, value=200):
    yy, xx = np.mgrid[0:h, 0:w]
    return (((yy + xx + 1) % 2) * value).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------- 6: state and batch
def dirty_batch():
    return np.stack([ref.scene(83, 97, 11, shapes=80), ref.noise(83, 97, 21)])


def dense_and_constant():
    return np.stack([ref.noise(83, 97, 22), np.full((83, 97), 140, np.uint8)])


DIRTY_KW = dict(n_features=300, n_levels=4)


def big_batch(n=70):
    return np.stack([ref.noise(40, 48, 100 + i) for i in range(n)])


BIG_BATCH_KW = dict(n_features=100, n_levels=1)
