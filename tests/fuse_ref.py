"""numpy restatement of the fusion search and the map-point refresh of DESIGN.md 4n (ORBmatcher::Fuse,
MapPoint::ComputeDistinctiveDescriptors, MapPoint::UpdateNormalAndDepth): dense, with no grid (every point against every frame
row), the doubles in the order the specification writes them - numpy fuses nothing, so they are the device's bit for bit - and
everything else a comparison or an integer.  ``apply_fusion`` is restated in plain Python by another route."""
import numpy as np

import proj_match_ref as R

NONE_DIST = R.NONE_DIST
_BIG = np.int64(2**62)


def gates(X, A, Ow, th, camera, bounds, scale, scale2, rng=None, normal=None, level=None, cos2_limit=0.25, margins=(0.64, 1.44)):
    """(status, u, v, lp, r) as ``proj_match_ref.gates`` with the range gate d2 < m_lo2 dmin2 || d2 > m_hi2 dmax2; the level
    comes from dmax2 as it stands."""
    X = np.asarray(X, np.float64).reshape(-1, 3)
    A = np.asarray(A, np.float64).reshape(3, 4)
    Ow = np.asarray(Ow, np.float64).reshape(3)
    fx, fy, cx, cy = (np.float64(c) for c in camera)
    min_x, max_x, min_y, max_y = (np.float64(b) for b in bounds)
    scale, scale2 = np.asarray(scale, np.float64), np.asarray(scale2, np.float64)
    m_lo2, m_hi2 = np.float64(margins[0]), np.float64(margins[1])
    n, L = len(X), len(scale)
    with np.errstate(all="ignore"):
        xc = ((A[0, 0] * X[:, 0] + A[0, 1] * X[:, 1]) + A[0, 2] * X[:, 2]) + A[0, 3]
        yc = ((A[1, 0] * X[:, 0] + A[1, 1] * X[:, 1]) + A[1, 2] * X[:, 2]) + A[1, 3]
        zc = ((A[2, 0] * X[:, 0] + A[2, 1] * X[:, 1]) + A[2, 2] * X[:, 2]) + A[2, 3]
        status = np.zeros(n, np.int32)
        status[~(zc > 0)] = 1
        iz = 1.0 / zc
        u = fx * (xc * iz) + cx
        v = fy * (yc * iz) + cy
        inside = (min_x <= u) & (u < max_x) & (min_y <= v) & (v < max_y)
        status[(status == 0) & ~inside] = 2
        d2 = (xc * xc + yc * yc) + zc * zc
        if rng is not None:
            rng = np.asarray(rng, np.float64).reshape(n, 2)
            status[(status == 0) & ((d2 < m_lo2 * rng[:, 0]) | (d2 > m_hi2 * rng[:, 1]))] = 3
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


def observed(ids, lists, frame):
    """bool [n]: the list of point ids[i] (>= 0) holds an observation in ``frame``."""
    return np.array([m >= 0 and any(int(f) == frame for f, _ in lists[m]) for m in np.asarray(ids).reshape(-1)], bool)


def search(points, frame, frame_index, lists, A, Ow, th, camera, bounds, scale, scale2, th_low=50, margins=(0.64, 1.44), chi2=5.99,
           offsets=(-1, 0), cos2_limit=0.25):
    """One pair.  ``points``: dict xyz, desc, id and optionally range, normal, level; ``frame``: dict desc, xy, level, point;
    ``lists``: the observation lists of the map.  Returns dict row, dist, status, other, u, v, lp, count [3]."""
    ids = np.asarray(points["id"], np.int64).reshape(-1)
    n1 = len(ids)
    d2rows = np.asarray(frame["desc"], np.uint8).reshape(-1, 32)
    xy2 = np.asarray(frame["xy"], np.float32).reshape(-1, 2)
    level2 = np.asarray(frame["level"], np.int64).reshape(-1)
    point2 = np.asarray(frame["point"], np.int64).reshape(-1)
    n2 = len(level2)
    status, u, v, lp, r = gates(points["xyz"], A, Ow, th, camera, bounds, scale, scale2, points.get("range"), points.get("normal"),
                                points.get("level"), cos2_limit, margins)
    seen = observed(ids, lists, frame_index)
    status = np.where(seen, 5, status).astype(np.int32)
    u, v = np.where(seen, np.nan, u), np.where(seen, np.nan, v)
    lp = np.where(seen, -1, lp).astype(np.int32)
    row = np.full(n1, -1, np.int32)
    dist = np.full(n1, NONE_DIST, np.int32)
    other = np.full(n1, -1, np.int32)
    live = np.flatnonzero(status == 0)
    if n2 and len(live):
        lim = np.float64(chi2) * np.asarray(scale2, np.float64)[np.clip(level2, 0, len(scale) - 1)]
        x2, y2 = xy2[:, 0].astype(np.float64), xy2[:, 1].astype(np.float64)
        ul, vl, rl, ll = u[live, None], v[live, None], r[live, None], lp[live, None].astype(np.int64)
        with np.errstate(invalid="ignore"):
            cand = (np.abs(x2[None, :] - ul) < rl) & (np.abs(y2[None, :] - vl) < rl)
            cand &= (np.maximum(ll + offsets[0], 0) <= level2[None, :]) & (level2[None, :] <= ll + offsets[1])
            ex, ey = ul - x2[None, :], vl - y2[None, :]
            cand &= ~((ex * ex + ey * ey) > lim[None, :])
        key = np.where(cand, R.hamming(np.asarray(points["desc"], np.uint8).reshape(-1, 32)[live], d2rows) * (1 << 23) + np.arange(n2)[None, :], _BIG)
        j = key.argmin(1)
        best = key[np.arange(len(live)), j]
        has = best < _BIG
        row[live[has]] = j[has]
        dist[live[has]] = best[has] >> 23
    status[(status == 0) & (row < 0)] = 6
    status[(status == 0) & (dist > th_low)] = 7
    # one-to-one: the smallest (d, i) keeps a contested row
    winner = {}
    for i in np.flatnonzero(status == 0):
        k = (int(dist[i]), int(i))
        if int(row[i]) not in winner or k < winner[int(row[i])]:
            winner[int(row[i])] = k
    for i in np.flatnonzero(status == 0):
        w = winner[int(row[i])][1]
        if w == i:
            other[i] = point2[row[i]]
        else:
            status[i] = 8
            other[i] = ids[w]
    count = np.array([((status == 0) & (other < 0)).sum(), ((status == 0) & (other >= 0)).sum(), (status == 8).sum()], np.int32)
    return dict(row=row, dist=dist, status=status, other=other, u=u, v=v, lp=lp, count=count)


def median_choice(D):
    """(medians, chosen row) of the table D [N,N]: the element of rank (N - 1) // 2 of each sorted row, the smallest (median, i)."""
    D = np.asarray(D, np.int64)
    N = len(D)
    if N == 0:
        return np.zeros(0, np.int64), -1
    med = np.sort(D, axis=1)[:, (N - 1) // 2]
    return med, int(np.lexsort((np.arange(N), med))[0])


def refresh(xyz, lists, frame_desc, frame_level, centres, scale, ref=None, select=None):
    """The refresh of the points ``select`` (None: all): ``frame_desc[b]`` u8 [n_b,32] and ``frame_level[b]`` int [n_b] in row
    order, ``centres`` f64 [B,3].  Returns dict best, descriptors, normal, dmin2, dmax2."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    centres = np.asarray(centres, np.float64).reshape(-1, 3)
    scale = np.asarray(scale, np.float64)
    sel = range(len(lists)) if select is None else [int(m) for m in select]
    K = len(sel)
    best = np.full(K, -1, np.int32)
    desc = np.zeros((K, 32), np.uint8)
    normal = np.full((K, 3), np.nan)
    rng = np.full((K, 2), np.nan)
    for o, m in enumerate(sel):
        ob = lists[m]
        N = len(ob)
        if N == 0:
            continue
        rows = np.stack([np.asarray(frame_desc[f], np.uint8).reshape(-1, 32)[r] for f, r in ob])
        _, b = median_choice(R.hamming(rows, rows))
        best[o] = b
        desc[o] = rows[b]
        with np.errstate(all="ignore"):
            s, lens = None, []
            for f, _ in ob:
                p = xyz[m] - centres[f]
                ln = np.sqrt((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2])
                t = p / ln
                s = t if s is None else s + t
                lens.append(ln)
            inv = np.float64(1.0) / np.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])
            nr = s * inv
            k = 0 if ref is None else min(max(int(ref[m]), 0), N - 1)
            l = min(max(int(np.asarray(frame_level[ob[k][0]]).reshape(-1)[ob[k][1]]), 0), len(scale) - 1)
            dmax = lens[k] * scale[l]
            dmin = dmax / scale[-1]
            if np.isfinite(nr).all():
                normal[o] = nr
                rng[o] = (dmin * dmin, dmax * dmax)
    return dict(best=best, descriptors=desc, normal=normal, dmin2=rng[:, 0].copy(), dmax2=rng[:, 1].copy())


def apply_fusion(lists, results):
    """Plain Python, by another route than the library's union-find: the classes as the connected components of the link graph,
    found by a flood fill.  ``lists``: list of lists of (frame, row).  Returns (new lists, alias list, updates sorted list of
    (frame, row, id))."""
    M = len(lists)
    edges = {m: set() for m in range(M)}
    adds, by_row = [], {}
    for r in results:
        for m, st, q, row in zip(r["id"], r["status"], r["other"], r["row"]):
            m, st, q, row = int(m), int(st), int(q), int(row)
            if m < 0 or st not in (0, 8):
                continue
            if st == 0 and q < 0:
                adds.append((m, int(r["frame"]), row))
                by_row.setdefault((int(r["frame"]), row), []).append(m)
            elif q >= 0:
                edges[m].add(q)
                edges[q].add(m)
    for ms in by_row.values():
        for m in ms[1:]:
            edges[ms[0]].add(m)
            edges[m].add(ms[0])
    alias, seen = list(range(M)), set()
    new = [list(map(tuple, x)) for x in lists]
    before, after = {}, {}
    for start in range(M):
        if start in seen:
            continue
        comp, todo = [], [start]
        seen.add(start)
        while todo:
            a = todo.pop()
            comp.append(a)
            for b in edges[a]:
                if b not in seen:
                    seen.add(b)
                    todo.append(b)
        comp.sort()
        s = max(comp, key=lambda m: (len(lists[m]), -m))
        gained = [(f, r) for m, f, r in adds if m in comp]
        if len(comp) == 1 and not gained:
            continue
        own = dict(lists[s])
        kept = dict(own)
        for f, r in [(f, r) for m in comp if m != s for f, r in lists[m]] + gained:
            if f not in own and (f not in kept or r < kept[f]):
                kept[f] = r
        for f, r in gained:
            before[(f, r)] = -1
        for m in comp:
            alias[m] = s
            for f, r in lists[m]:
                before[(int(f), int(r))] = m
            new[m] = []
        new[s] = sorted(kept.items())
        for f, r in new[s]:
            after[(f, r)] = s
    upd = sorted((f, r, after.get((f, r), -1)) for (f, r), was in before.items() if after.get((f, r), -1) != was)
    return new, alias, upd
