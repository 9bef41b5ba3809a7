"""numpy restatement of the node-constrained search of DESIGN.md 4k (ORBmatcher::SearchByBoW over the direct index): the node
top-2, the selection, the one-to-one step and the rotation histogram, from their definitions.  Everything is an integer, or
a double that holds an integer <= 256; the device must match bit for bit."""
import numpy as np

NONE_IDX, NONE_DIST = -1, 2**31 - 1
NO_SECOND = 256
N_BINS = 32
_POP = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def hamming(a, b):
    """int64 [len(a), len(b)] distances of uint8 [., 32] rows, in slabs of side-1 rows."""
    a, b = np.asarray(a, np.uint8).reshape(-1, 32), np.asarray(b, np.uint8).reshape(-1, 32)
    out = np.zeros((len(a), len(b)), np.int64)
    step = max(1, (1 << 20) // max(1, len(b)))
    for s in range(0, len(a), step):
        out[s:s + step] = _POP[a[s:s + step, None, :] ^ b[None, :, :]].sum(-1, dtype=np.int64)
    return out


def group(nodes):
    """(order, nodes_sorted) of one image: its rows sorted by (node id as unsigned 32-bit, row); masked rows go last."""
    nodes = np.asarray(nodes, np.int32).reshape(-1)
    order = np.argsort(nodes.view(np.uint32), kind="stable").astype(np.int32)
    return order, nodes[order]


def node_top2(d1, nodes1, d2, nodes2):
    """(idx, dist) int32 [n1, 2]: per side-1 row its two nearest side-2 rows of the same node id >= 0, by (distance, row)."""
    nodes1, nodes2 = np.asarray(nodes1, np.int64).reshape(-1), np.asarray(nodes2, np.int64).reshape(-1)
    d1, d2 = np.asarray(d1, np.uint8).reshape(-1, 32), np.asarray(d2, np.uint8).reshape(-1, 32)
    idx = np.full((len(nodes1), 2), NONE_IDX, np.int32)
    dist = np.full((len(nodes1), 2), NONE_DIST, np.int32)
    for v in np.unique(nodes1[nodes1 >= 0]):
        r1, r2 = np.flatnonzero(nodes1 == v), np.flatnonzero(nodes2 == v)
        if len(r2) == 0:
            continue
        d = hamming(d1[r1], d2[r2])
        k = min(2, len(r2))
        o = np.argsort(d * (1 << 23) + r2[None, :], axis=1, kind="stable")[:, :k]
        idx[r1[:, None], np.arange(k)[None, :]] = r2[o]
        dist[r1[:, None], np.arange(k)[None, :]] = np.take_along_axis(d, o, axis=1)
    return idx, dist


def proposed(idx, dist, th_low=50, ratio=0.75):
    """bool [n1]: a first neighbour, d0 <= th_low and (double)d0 < ratio * (double)d1, a missing second one counting as 256."""
    d0 = dist[:, 0].astype(np.float64)
    d1 = np.where(idx[:, 1] >= 0, dist[:, 1], NO_SECOND).astype(np.float64)
    return (idx[:, 0] >= 0) & (dist[:, 0].astype(np.int64) <= int(th_low)) & (d0 < np.float64(ratio) * d1)


def one_to_one(idx, dist, keep, n2):
    """matches12 int32 [n1]: among the kept rows that name one side-2 row the smallest (d0, i) keeps it."""
    m12 = np.full(len(idx), -1, np.int32)
    owner = np.full(n2, 2**62, np.int64)
    rows = np.flatnonzero(keep)
    key = dist[rows, 0].astype(np.int64) * (1 << 13) + rows
    np.minimum.at(owner, idx[rows, 0], key)
    won = rows[owner[idx[rows, 0]] == key]
    m12[won] = idx[won, 0]
    return m12


def rotation_keep(m12, bins1, bins2):
    """``m12`` without the matches outside the first bin by (count descending, bin ascending) of the histogram of
    (bin1 - bin2) & 31, and the second and third while their count c > 0 and 10 c >= the first's."""
    m12 = m12.copy()
    rows = np.flatnonzero(m12 >= 0)
    r = (np.asarray(bins1, np.int64)[rows] - np.asarray(bins2, np.int64)[m12[rows]]) & (N_BINS - 1)
    hist = np.bincount(r, minlength=N_BINS)
    first = np.lexsort((np.arange(N_BINS), -hist))[:3]
    c1 = hist[first[0]]
    ok = [first[0]] + [b for b in first[1:] if hist[b] > 0 and 10 * hist[b] >= c1]
    m12[rows[~np.isin(r, ok)]] = -1
    return m12


def search(d1, nodes1, d2, nodes2, bins1=None, bins2=None, th_low=50, ratio=0.75):
    """(matches12 int32 [n1], count, (idx, dist)) of one pair."""
    idx, dist = node_top2(d1, nodes1, d2, nodes2)
    m12 = one_to_one(idx, dist, proposed(idx, dist, th_low, ratio), len(np.asarray(nodes2).reshape(-1)))
    if bins1 is not None and bins2 is not None:
        m12 = rotation_keep(m12, bins1, bins2)
    return m12, int((m12 >= 0).sum()), (idx, dist)


def search_loops(d1, nodes1, d2, nodes2, bins1=None, bins2=None, th_low=50, ratio=0.75):
    """``search`` as plain loops over the rows (tiny pairs only): what ``search`` is checked against."""
    n1, n2 = len(nodes1), len(nodes2)
    best = []
    for i in range(n1):
        cand = []
        for j in range(n2):
            if nodes1[i] == nodes2[j] and nodes1[i] >= 0:
                cand.append((int(_POP[np.asarray(d1[i]) ^ np.asarray(d2[j])].sum()), j))
        cand.sort()
        best.append(cand[:2])
    idx = np.full((n1, 2), NONE_IDX, np.int32)
    dist = np.full((n1, 2), NONE_DIST, np.int32)
    prop = []
    for i, c in enumerate(best):
        for s, (d, j) in enumerate(c):
            idx[i, s], dist[i, s] = j, d
        if c and c[0][0] <= th_low and float(c[0][0]) < ratio * float(c[1][0] if len(c) > 1 else NO_SECOND):
            prop.append(i)
    m12 = np.full(n1, -1, np.int32)
    for j in range(n2):
        named = sorted((best[i][0][0], i) for i in prop if best[i][0][1] == j)
        if named:
            m12[named[0][1]] = j
    if bins1 is not None and bins2 is not None:
        hist = [0] * N_BINS
        for i in range(n1):
            if m12[i] >= 0:
                hist[(int(bins1[i]) - int(bins2[m12[i]])) % N_BINS] += 1
        ranked = sorted(range(N_BINS), key=lambda b: (-hist[b], b))[:3]
        ok = {ranked[0]} | {b for b in ranked[1:] if hist[b] > 0 and 10 * hist[b] >= hist[ranked[0]]}
        for i in range(n1):
            if m12[i] >= 0 and (int(bins1[i]) - int(bins2[m12[i]])) % N_BINS not in ok:
                m12[i] = -1
    return m12, int((m12 >= 0).sum()), (idx, dist)
