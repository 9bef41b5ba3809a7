"""The hand-made cases of the quadtree keypoint distribution with the answers one can write down without running
anything; tests/test_orb_dist_cpu.py holds the numpy statement to them and tests/test_orb_dist_gpu.py the device.

Dot images as in orb_cases.py: an isolated dot of contrast c scores c - 1 and has R = 3024 c^4.  A 145 x 65 level has the
scoreable rectangle x 16..128, y 16..48 (w = 113, h = 33), hence n_ini = (226 + 33) // 66 = 3 roots: x in [16, 53), [53, 91),
[91, 129).  Root 0 is cut at xm = 16 + 19 = 35 and ym = 16 + 17 = 33.
"""
from __future__ import annotations

import numpy as np

import orb_cases as C
import orb_dist_ref as dref
import orb_ref as ref

H, W, BG = 65, 145, 100
ROOT0 = (16, 16, 53, 49)
QUADRANTS0 = [(16, 16, 35, 33), (35, 16, 53, 33), (16, 33, 35, 49), (35, 33, 53, 49)]


def dots(points, h=H, w=W):
    """A flat image of value BG with a dot of value BG + c at every (x, y, c)."""
    return C.dot_image(h, w, [(x, y, BG + c) for x, y, c in points], bg=BG)


class Case:
    """One image on one level with its thresholds, quota and the keypoints [(x, y)] expected in output order (None: only the
    reference says); `harris`, where given, is what the selection by R alone returns at t_ini."""

    def __init__(self, name, img, quota, want, t_ini=20, t_min=20, harris=None):
        self.name, self.img, self.quota, self.want, self.t_ini, self.t_min, self.harris = name, img, quota, want, t_ini, t_min, harris


# spread: the three strongest dots crowd in quadrant 0 of root 0, one weak dot in each other quadrant
SPREAD = [(18, 18, 60), (28, 18, 50), (18, 28, 45), (44, 20, 30), (20, 40, 30), (44, 40, 30)]
# order of the cut: two dots in each quadrant of root 0, each pair in different sub-quadrants; 50 beats 40
CUT = [(18, 18, 50), (30, 28, 40), (37, 18, 50), (48, 28, 40), (18, 35, 50), (30, 45, 40), (40, 36, 50), (50, 46, 40)]
# zero gain: 165 x 165 has one root [16, 149) x [16, 149); the path to the corner has widths 133, 67, 34, 17, 9, 5, 3, and only
# the seventh split (of [16, 19), at 18) parts x = 16 from x = 18.  (On 145 x 65 no node wider than 2 survives five splits.)
PAIR_SIDE = 165
PAIR = [(16, 16, 60), (18, 16, 50)]
# roots: 150 x 97 has w = 118, h = 65, n_ini = 301 // 130 = 2: [16, 75) and [75, 134); two dots in each
TWO_ROOTS_H, TWO_ROOTS_W = 97, 150
TWO_ROOTS = [(20, 20, 40), (60, 70, 30), (80, 30, 60), (120, 60, 50)]
TALL = [(20, 20, 40), (40, 100, 60), (24, 120, 30)]                      # 65 x 145 (W x H): one root
# adaptive cells, t_ini = 20, t_min = 7: contrast 30 scores 29, contrast 12 scores 11
SAME_CELL = [(20, 20, 30), (40, 30, 12)]                                  # both in cell (0, 0)
SEAM_LEFT = [(39, 20, 30), (47, 20, 12)]                                  # the weak dot at x - 16 = 31: still cell 0, dropped
SEAM_RIGHT = [(40, 20, 30), (48, 20, 12)]                                 # the weak dot at x - 16 = 32: cell 1, kept


def cases():
    return [
        Case("spread", dots(SPREAD), 4, [(18, 18), (44, 20), (20, 40), (44, 40)], harris=[(18, 18), (28, 18), (18, 28), (44, 20)]),
        Case("cut5", dots(CUT), 5, [(18, 18), (37, 18), (18, 35), (40, 36), (30, 28)]),
        Case("cut6", dots(CUT), 6, [(18, 18), (37, 18), (18, 35), (40, 36), (30, 28), (48, 28)]),
        Case("zero_gain", dots(PAIR, PAIR_SIDE, PAIR_SIDE), 2, [(16, 16), (18, 16)]),
        Case("two_roots_1", dots(TWO_ROOTS, TWO_ROOTS_H, TWO_ROOTS_W), 1, [(80, 30)]),
        Case("two_roots_2", dots(TWO_ROOTS, TWO_ROOTS_H, TWO_ROOTS_W), 2, [(80, 30), (20, 20)]),
        Case("tall", dots(TALL, 145, 65), 2, [(40, 100), (20, 20)]),
        Case("narrow", ref.noise(80, 32, 3), 10, []),
        Case("same_cell", dots(SAME_CELL), 10, [(20, 20)], t_min=7),
        Case("seam_left", dots(SEAM_LEFT), 10, [(39, 20)], t_min=7),
        Case("seam_right", dots(SEAM_RIGHT), 10, [(40, 20), (48, 20)], t_min=7),
        Case("weak_never", dots(SEAM_RIGHT), 10, [(40, 20)], t_min=20),
    ]


def half_noise():
    return dref.half_noise_image()


# ------------------------------------------------------------------------------------------- the reference, computed once
_CACHE = {}


def reference(img, P, mask=None):
    """orb_dist_ref.extract for the parameters of P (an OrbParams of the quadtree mode, or anything with lh, lw, quota, t, t_min,
    table), computed once per distinct input; callers must not modify what they get."""
    img = np.ascontiguousarray(img)
    key = (img.shape, hash(img.tobytes()), None if mask is None else hash(np.ascontiguousarray(mask).tobytes()), tuple(P.lh.tolist()),
           tuple(P.lw.tolist()), tuple(np.asarray(P.quota).tolist()), int(P.t), int(P.t_min), hash(P.table.tobytes()))
    if key not in _CACHE:
        _CACHE[key] = dref.extract(img, P.lh, P.lw, P.quota, P.t, P.t_min, P.table, mask0=mask)
    return _CACHE[key]
