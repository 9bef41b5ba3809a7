"""numpy restatement of the projection search of DESIGN.md 4l (ORBmatcher::SearchByProjection): the gates in f64 in the order
the specification writes them, the windowed top-2 with NO grid (every point against every frame row), ORB-SLAM's selection, and
the one-to-one step and rotation histogram of 4k (``bow_match_ref``).  numpy fuses nothing, so the doubles are the device's
bit for bit; everything behind the gates is a comparison or an integer."""
import numpy as np

import bow_match_ref as B

NONE_IDX, NONE_DIST = B.NONE_IDX, B.NONE_DIST
_BIG = np.int64(2**62)


def hamming(a, b):
    """int64 [len(a), len(b)] distances of uint8 [., 32] rows, on four 64-bit words a row where numpy can count bits."""
    if not hasattr(np, "bitwise_count"):
        return B.hamming(a, b)
    a, b = np.ascontiguousarray(a, np.uint8).reshape(-1, 32).view(np.uint64), np.ascontiguousarray(b, np.uint8).reshape(-1, 32).view(np.uint64)
    out = np.zeros((len(a), len(b)), np.int64)
    for w in range(4):
        out += np.bitwise_count(a[:, None, w] ^ b[None, :, w])
    return out


def scale_tables(n_levels, scale):
    """(scale[l], scale2[l]) as ORB-SLAM's extractor makes them: s_0 = 1, s_l = s_{l-1} * scale; scale2 = s_l * s_l."""
    s = np.ones(int(n_levels), np.float64)
    for l in range(1, int(n_levels)):
        s[l] = s[l - 1] * np.float64(scale)
    return s, s * s


def gates(X, A, Ow, th, camera, bounds, scale, scale2, rng=None, normal=None, level=None, cos2_limit=0.25):
    """(status int32, u, v f64, lp int32, r f64) of the points X [n,3] under the pose A [3,4]: 4l (a), gate by gate."""
    X = np.asarray(X, np.float64).reshape(-1, 3)
    A = np.asarray(A, np.float64).reshape(3, 4)
    Ow = np.asarray(Ow, np.float64).reshape(3)
    fx, fy, cx, cy = (np.float64(c) for c in camera)
    min_x, max_x, min_y, max_y = (np.float64(b) for b in bounds)
    scale, scale2 = np.asarray(scale, np.float64), np.asarray(scale2, np.float64)
    n, L = len(X), len(scale)
    with np.errstate(all="ignore"):
        xc = ((A[0, 0] * X[:, 0] + A[0, 1] * X[:, 1]) + A[0, 2] * X[:, 2]) + A[0, 3]
        yc = ((A[1, 0] * X[:, 0] + A[1, 1] * X[:, 1]) + A[1, 2] * X[:, 2]) + A[1, 3]
        zc = ((A[2, 0] * X[:, 0] + A[2, 1] * X[:, 1]) + A[2, 2] * X[:, 2]) + A[2, 3]
        status = np.zeros(n, np.int32)
        front = zc > 0
        status[~front] = 1
        iz = 1.0 / zc
        u = fx * (xc * iz) + cx
        v = fy * (yc * iz) + cy
        inside = (min_x <= u) & (u < max_x) & (min_y <= v) & (v < max_y)
        status[(status == 0) & ~inside] = 2
        d2 = (xc * xc + yc * yc) + zc * zc
        if rng is not None:
            rng = np.asarray(rng, np.float64).reshape(n, 2)
            status[(status == 0) & ((d2 < rng[:, 0]) | (d2 > rng[:, 1]))] = 3
        if normal is not None:
            nr = np.asarray(normal, np.float64).reshape(n, 3)
            po = X - Ow[None, :]
            dot = (po[:, 0] * nr[:, 0] + po[:, 1] * nr[:, 1]) + po[:, 2] * nr[:, 2]
            po2n = (po[:, 0] * po[:, 0] + po[:, 1] * po[:, 1]) + po[:, 2] * po[:, 2]
            status[(status == 0) & (~(dot > 0) | (dot * dot < np.float64(cos2_limit) * po2n))] = 4
        lp = np.zeros(n, np.int32)
        if rng is not None:
            for l in range(L - 1):
                lp += (scale2[l] * d2 < rng[:, 1]).astype(np.int32)
        elif level is not None:
            lp = np.clip(np.asarray(level, np.int64).reshape(n), 0, L - 1).astype(np.int32)
        r = np.float64(th) * scale[lp]
    ok = status == 0
    u = np.where(status == 1, np.nan, u)
    v = np.where(status == 1, np.nan, v)
    return status, u, v, np.where(ok, lp, -1).astype(np.int32), np.where(ok, r, np.nan)


def window_top2(d1, status, u, v, r, lp, d2, xy2, level2, taken2=None, level_rule=False, lo=0, hi=0):
    """(idx, dist) int32 [n1, 2]: 4l (b) - per point its two nearest candidates by (distance, row), in slabs of points."""
    d1, d2 = np.asarray(d1, np.uint8).reshape(-1, 32), np.asarray(d2, np.uint8).reshape(-1, 32)
    xy2 = np.asarray(xy2, np.float32).reshape(-1, 2)
    level2 = np.asarray(level2, np.int64).reshape(-1)
    n1, n2 = len(d1), len(d2)
    idx = np.full((n1, 2), NONE_IDX, np.int32)
    dist = np.full((n1, 2), NONE_DIST, np.int32)
    if n1 == 0 or n2 == 0:
        return idx, dist
    free = np.ones(n2, bool) if taken2 is None else np.asarray(taken2).reshape(-1) == 0
    x2, y2 = xy2[:, 0].astype(np.float64), xy2[:, 1].astype(np.float64)
    rows = np.arange(n2, dtype=np.int64)
    step = max(1, (1 << 19) // n2)
    for s in range(0, n1, step):
        e = min(n1, s + step)
        live = status[s:e] == 0
        with np.errstate(invalid="ignore"):
            cand = (np.abs(x2[None, :] - u[s:e, None]) < r[s:e, None]) & (np.abs(y2[None, :] - v[s:e, None]) < r[s:e, None])
        cand &= live[:, None] & free[None, :]
        if level_rule:
            l = lp[s:e].astype(np.int64)
            cand &= (l[:, None] + lo <= level2[None, :]) & (level2[None, :] <= l[:, None] + hi)
        key = np.where(cand, hamming(d1[s:e], d2) * (1 << 23) + rows[None, :], _BIG)
        for k in range(2):
            j = key.argmin(1)
            best = key[np.arange(e - s), j]
            has = best < _BIG
            idx[s:e, k][has] = j[has]
            dist[s:e, k][has] = best[has] >> 23
            key[np.arange(e - s), j] = _BIG
    return idx, dist


def proposed(idx, dist, level2, th_high=100, ratio=0.9):
    """bool [n1]: 4l (c) - ORB-SLAM's rule: the ratio counts only between two neighbours of one level; a lone one passes."""
    level2 = np.asarray(level2, np.int64).reshape(-1)
    first = idx[:, 0] >= 0
    second = idx[:, 1] >= 0
    l0 = level2[np.where(first, idx[:, 0], 0)] if len(level2) else np.zeros(len(idx), np.int64)
    l1 = level2[np.where(second, idx[:, 1], 0)] if len(level2) else np.zeros(len(idx), np.int64)
    with np.errstate(invalid="ignore"):
        worse = dist[:, 0].astype(np.float64) > np.float64(ratio) * dist[:, 1].astype(np.float64)
    return first & (dist[:, 0].astype(np.int64) <= int(th_high)) & ~(second & (l0 == l1) & worse)


def search(points, frame, A, Ow, th, camera, bounds, scale, scale2, th_high=100, ratio=0.9, cos2_limit=0.25, level_rule=None,
           offsets=None):
    """One pair.  ``points``: dict with xyz, desc and optionally range [n,2], normal, level, bins; ``frame``: dict with desc, xy,
    level and optionally bins, taken.  Returns (matches12, count, tables) with tables = dict(status, u, v, lp, idx, dist)."""
    rng, normal, level = points.get("range"), points.get("normal"), points.get("level")
    if level_rule is None:
        level_rule = rng is not None or level is not None
    if offsets is None:
        offsets = (-1, 0) if rng is not None else (-1, 1)
    status, u, v, lp, r = gates(points["xyz"], A, Ow, th, camera, bounds, scale, scale2, rng, normal, level, cos2_limit)
    idx, dist = window_top2(points["desc"], status, u, v, r, lp, frame["desc"], frame["xy"], frame["level"], frame.get("taken"),
                            bool(level_rule), int(offsets[0]), int(offsets[1]))
    n2 = len(np.asarray(frame["level"]).reshape(-1))
    m12 = B.one_to_one(idx, dist, proposed(idx, dist, frame["level"], th_high, ratio), n2)
    if points.get("bins") is not None and frame.get("bins") is not None:
        m12 = B.rotation_keep(m12, points["bins"], frame["bins"])
    return m12, int((m12 >= 0).sum()), dict(status=status, u=u, v=v, lp=lp, idx=idx, dist=dist)


def mutual(m12, rows1, m21, rows2):
    """ORB-SLAM's SearchBySim3 agreement: point i of side 1 (feature row rows1[i] of frame 1) matched feature row m12[i] of
    frame 2; it stays iff that row belongs to a point k of side 2 (rows2[k] == m12[i]) whose own match m21[k] is rows1[i].
    Returns (i, k) int32 arrays, i ascending."""
    rows1, rows2 = np.asarray(rows1, np.int64), np.asarray(rows2, np.int64)
    point_of_row2 = {int(r): k for k, r in enumerate(rows2)}
    out = []
    for i in np.flatnonzero(np.asarray(m12) >= 0):
        k = point_of_row2.get(int(m12[i]))
        if k is not None and int(m21[k]) == int(rows1[i]):
            out.append((i, k))
    a = np.asarray(out, np.int32).reshape(-1, 2)
    return a[:, 0].copy(), a[:, 1].copy()


def compose(S, T):
    """[3,4] of x -> S (T x): S [3,4] = [sR | t] after T [3,4] = [R | t]."""
    S, T = np.asarray(S, np.float64).reshape(3, 4), np.asarray(T, np.float64).reshape(-1, 4)[:3]
    return np.c_[S[:, :3] @ T[:, :3], S[:, :3] @ T[:, 3] + S[:, 3]]


def invert(S):
    """The inverse of [sR | t] as [3,4]."""
    S = np.asarray(S, np.float64).reshape(3, 4)
    Mi = np.linalg.inv(S[:, :3])
    return np.c_[Mi, -Mi @ S[:, 3]]
