"""Numpy statement of the quadtree keypoint distribution with an adaptive FAST threshold, node by node.

Test infrastructure in the manner of orb_ref.py, whose stages it takes for everything up to the candidate list and after the
selection.  Per level: (1) a candidate is live if it scores >= t_ini or if its 32 x 32 cell holds no candidate that does;
(2) the roots are n_ini vertical strips of the scoreable rectangle; (3) rounds split the fullest nodes, in the order (count
descending, y0, x0), until there are N nodes or none holds two candidates; (4) every node gives its best candidate under
(R descending, y, x) and the best N of those are kept.  Nothing here is shared with the kernel.
"""
from __future__ import annotations

import numpy as np

import orb_ref as ref

BORDER = ref.BORDER
CELL_SHIFT = 5


def live_mask(scores, ys, xs, t_ini):
    """bool [n]: the candidates that survive the adaptive threshold."""
    s = np.asarray(scores, np.int64)[ys, xs]
    cells = list(zip(((xs - BORDER) >> CELL_SHIFT).tolist(), ((ys - BORDER) >> CELL_SHIFT).tolist()))
    strong = {c for c, v in zip(cells, s.tolist()) if v >= t_ini}
    return np.asarray([v >= t_ini or c not in strong for c, v in zip(cells, s.tolist())], bool).reshape(len(s))


def n_roots(h_l, w_l):
    w, h = w_l - 2 * BORDER, h_l - 2 * BORDER
    return max(1, (2 * w + h) // (2 * h))


def roots(h_l, w_l):
    """[(x0, y0, x1, y1)] of the root strips of a level h_l x w_l (both >= 33)."""
    w, h = w_l - 2 * BORDER, h_l - 2 * BORDER
    n = n_roots(h_l, w_l)
    return [(BORDER + i * w // n, BORDER, BORDER + (i + 1) * w // n, BORDER + h) for i in range(n)]


def children(node):
    x0, y0, x1, y1 = node
    xm, ym = x0 + ((x1 - x0 + 1) >> 1), y0 + ((y1 - y0 + 1) >> 1)
    return [(x0, y0, xm, ym), (xm, y0, x1, ym), (x0, ym, xm, y1), (xm, ym, x1, y1)]


def inside(node, pts):
    x0, y0, x1, y1 = node
    return [(x, y) for x, y in pts if x0 <= x < x1 and y0 <= y < y1]


def distribute(ys, xs, h_l, w_l, N, trace=None):
    """The final nodes {rectangle: [(x, y)]} of the live candidates (ys, xs) of one level at quota N; `trace`, if a list, gets one
    entry per round: the rectangles that were split, in the order of the cut."""
    pts = list(zip(np.asarray(xs).tolist(), np.asarray(ys).tolist()))
    nodes = {}
    if h_l < 2 * BORDER + 1 or w_l < 2 * BORDER + 1:
        return nodes
    for r in roots(h_l, w_l):
        p = inside(r, pts)
        if p:
            nodes[r] = p
    while len(nodes) < N:
        order = sorted((r for r, p in nodes.items() if len(p) > 1), key=lambda r: (-len(nodes[r]), r[1], r[0]))
        if not order:
            break
        n, split = len(nodes), []
        for r in order:
            kids = [(c, inside(c, nodes[r])) for c in children(r)]
            kids = [(c, p) for c, p in kids if p]
            split.append((r, kids))
            n += len(kids) - 1
            if n >= N:
                break
        for r, kids in split:
            del nodes[r]
            nodes.update(kids)
        if trace is not None:
            trace.append([r for r, _ in split])
    return nodes


def select(R, ys, xs, scores, h_l, w_l, N, t_ini, trace=None):
    """Indices into the candidate list of the keypoints of one level, in output order."""
    R, ys, xs = np.asarray(R, np.int64), np.asarray(ys, np.int64), np.asarray(xs, np.int64)
    if len(R) == 0 or N <= 0:
        return np.zeros(0, np.int64)
    live = np.nonzero(live_mask(scores, ys, xs, t_ini))[0]
    index = {(int(xs[i]), int(ys[i])): int(i) for i in live}
    nodes = distribute(ys[live], xs[live], h_l, w_l, N, trace)
    best = []
    for pts in nodes.values():
        best.append(min((index[p] for p in pts), key=lambda i: (-int(R[i]), int(ys[i]), int(xs[i]))))
    best.sort(key=lambda i: (-int(R[i]), int(ys[i]), int(xs[i])))
    return np.asarray(best[:N], np.int64)


def extract(img0, lh, lw, quota, t_ini, t_min, table, mask0=None):
    """One image through every stage with the quadtree selection: the dict of orb_ref.extract (its 'stages' are those of a run at
    t_min), plus 'live': per level the number of live candidates."""
    out = {k: [] for k in ("x", "y", "level", "bin", "response", "descriptors")}
    stages, n_live = [], []
    for l, img in enumerate(ref.pyramid(img0, lh, lw)):
        blurred = ref.blur(img)
        scores = ref.fast_scores(img, t_min)
        R, ys, xs = ref.candidates(img, t_min, mask0, np.asarray(img0).shape)
        stages.append((img, blurred, scores, (R, ys, xs)))
        n_live.append(int(live_mask(scores, ys, xs, t_ini).sum()) if len(R) else 0)
        keep = select(R, ys, xs, scores, img.shape[0], img.shape[1], int(quota[l]), t_ini)
        R, ys, xs = R[keep], ys[keep], xs[keep]
        bins = ref.orientation_bin(*ref.moments(img, ys, xs))
        out["x"].append(xs)
        out["y"].append(ys)
        out["level"].append(np.full(len(xs), l, np.int64))
        out["bin"].append(bins)
        out["response"].append(R)
        out["descriptors"].append(ref.describe(blurred, ys, xs, bins, table))
    res = {k: np.concatenate(v) for k, v in out.items()}
    res["descriptors"] = res["descriptors"].reshape(-1, 32)
    res["stages"] = stages
    res["live"] = n_live
    return res


def occupied_cells(xs, ys):
    """The number of distinct 32 x 32 cells ((x - 16) >> 5, (y - 16) >> 5) that hold a keypoint."""
    return len(set(zip(((np.asarray(xs) - BORDER) >> CELL_SHIFT).tolist(), ((np.asarray(ys) - BORDER) >> CELL_SHIFT).tolist())))


def half_noise_image():
    """300 x 200 (W x H): the left half noise, the right half a lattice of dots of contrast 12 on a flat ground."""
    img = np.full((200, 300), 100, np.uint8)
    img[:, :150] = ref.noise(200, 150, 4)
    img[8::16, 158::16] = 112
    return img
