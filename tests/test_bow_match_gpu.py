"""The node-constrained search on the device (slam_bow_match_*, slamhip/bow_match.py) against
tests/bow_match_ref.py, bit for bit.  The shapes are the smallest at which each path is taken: segments around one wave,
images around the scan's 64-row workgroups and at the limit of the LDS sort, batches up to the pair limit."""
import ctypes

import numpy as np
import pytest

import bow_match_ref as R
from hamming_families import prefix_rows

pytestmark = pytest.mark.gpu

INT_MAX = 2**31 - 1


@pytest.fixture(scope="module")
def bm(gpu_ctx):
    from slamhip import bow_match as module
    return module


def rows(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def noisy(rng, d, flips=3):
    """A copy of the rows with up to `flips` bits flipped in each."""
    d = d.copy()
    n = len(d)
    for _ in range(flips):
        bit = rng.integers(0, 256, n)
        d[np.arange(n), bit >> 3] ^= (128 >> (bit & 7)).astype(np.uint8)
    return d


def make_set(bm, ctx, images, **kw):
    """FeatureVectors of a list of (rows, node ids) images."""
    d = np.concatenate([np.asarray(i[0], np.uint8).reshape(-1, 32) for i in images] + [np.zeros((0, 32), np.uint8)])
    nodes = np.concatenate([np.asarray(i[1], np.int64).reshape(-1) for i in images] + [np.zeros(0, np.int64)])
    off = np.cumsum([0] + [len(i[1]) for i in images])
    return bm.FeatureVectors.from_nodes(d, nodes, off, ctx=ctx, **kw)


def cat_bins(bins):
    return None if bins is None else np.concatenate([np.asarray(b, np.int64).reshape(-1) for b in bins] + [np.zeros(0, np.int64)])


def check(bm, ctx, images1, images2, pairs, bins1=None, bins2=None, refs=None, **kw):
    """search_by_bow on the two sets against the reference pair by pair; returns the device's (matches, counts)."""
    fv1, fv2 = make_set(bm, ctx, images1), make_set(bm, ctx, images2)
    try:
        m, c, t = bm.search_by_bow(fv1, fv2, pairs, cat_bins(bins1), cat_bins(bins2), return_tables=True, ctx=ctx, **kw)
        tables = bm.node_top2(fv1, fv2, pairs, ctx=ctx)
    finally:
        fv1.free()
        fv2.free()
    assert len(m) == len(pairs) == len(c) == len(t) and c.dtype == np.int32
    for p, (a, b) in enumerate(pairs):
        ref = refs[p] if refs is not None else R.search(images1[a][0], images1[a][1], images2[b][0], images2[b][1],
                                                        None if bins1 is None else bins1[a], None if bins2 is None else bins2[b], **kw)
        assert m[p].dtype == np.int32 and np.array_equal(m[p], ref[0]), (p, a, b)
        assert int(c[p]) == ref[1], (p, a, b)
        assert np.array_equal(t[p][0], ref[2][0]) and np.array_equal(t[p][1], ref[2][1]), (p, a, b)
        assert np.array_equal(tables[p][0], ref[2][0]) and np.array_equal(tables[p][1], ref[2][1]), (p, a, b)
    return m, c


# ---- segments -----------------------------------------------------------------------------------------------------------------

SEGMENT_SIZES = (0, 1, 2, 63, 64, 65)          # rows of side 2 in nodes 0 .. 5; node 6 exists on side 2 only


def segment_pair(rng):
    nodes2 = np.concatenate([np.full(s, v) for v, s in enumerate(SEGMENT_SIZES)] + [np.full(200 - sum(SEGMENT_SIZES), 6)])
    nodes2 = nodes2[rng.permutation(200)]
    nodes1 = rng.integers(0, 6, 200)
    nodes1[:6] = np.arange(6)                  # every node at least once, the one that side 2 lacks included
    d2 = rows(rng, 200)
    d1 = rows(rng, 200)
    for i in range(200):                       # most side-1 rows are a noisy copy of a side-2 row of their node
        cand = np.flatnonzero(nodes2 == nodes1[i])
        if len(cand) and i % 5:
            d1[i] = noisy(rng, d2[cand[i % len(cand)]][None, :])[0]
    return d1, nodes1, d2, nodes2


def test_segments_of_every_size_around_a_wave(bm, gpu_ctx):
    from slamhip import knn_match_arrays

    rng = np.random.default_rng(4001)
    d1, n1, d2, n2 = segment_pair(rng)
    assert sorted(np.bincount(n2, minlength=7)[:6].tolist()) == sorted(SEGMENT_SIZES)
    check(bm, gpu_ctx, [(d1, n1)], [(d2, n2)], [(0, 0)])
    check(bm, gpu_ctx, [(d1, n1)], [(d2, n2)], [(0, 0)], th_low=256, ratio=1.0)
    # all ids equal: the dense search
    same = np.full(200, 77)
    idx, dist = bm.node_match_arrays(d1, d2, same, same, ctx=gpu_ctx)
    kidx, kdist = knn_match_arrays(d1, d2, 2, ctx=gpu_ctx)
    assert np.array_equal(idx, kidx) and np.array_equal(dist, kdist)
    check(bm, gpu_ctx, [(d1, same)], [(d2, same)], [(0, 0)])
    # all ids distinct: every segment is one row
    distinct = rng.permutation(200)
    m, c = check(bm, gpu_ctx, [(d1, np.arange(200))], [(d1[distinct], distinct)], [(0, 0)])
    assert c[0] == 200 and np.array_equal(distinct[m[0]], np.arange(200))
    # the ends of the id range, and masked rows on either side
    relabel = np.array([0, INT_MAX, 1, INT_MAX - 1, 5, 2**30, 9])
    check(bm, gpu_ctx, [(d1, relabel[n1])], [(d2, relabel[n2])], [(0, 0)])
    masked1, masked2 = relabel[n1].copy(), relabel[n2].copy()
    masked1[::3] = -1
    masked2[1::4] = -(2**31)
    masked2[2::7] = -5
    m, _ = check(bm, gpu_ctx, [(d1, masked1)], [(d2, masked2)], [(0, 0)], th_low=256, ratio=1.0)
    assert (m[0][::3] == -1).all() and not np.isin(m[0], np.flatnonzero(masked2 < 0)).any()
    check(bm, gpu_ctx, [(d1, np.full(200, -1))], [(d2, np.full(200, -1))], [(0, 0)])       # equal negative ids do not match


# ---- ties ---------------------------------------------------------------------------------------------------------------------

def test_ties_go_to_the_lowest_side2_row(bm, gpu_ctx):
    rng = np.random.default_rng(4002)
    d2 = rows(rng, 150)
    n2 = rng.integers(0, 3, 150)
    d2[100:150] = d2[20:70]                    # every row of 20 .. 69 has a twin 80 rows later, in the same node
    n2[100:150] = n2[20:70]
    d1, n1 = d2[20:70].copy(), n2[20:70].copy()
    idx, dist = bm.node_match_arrays(d1, d2, n1, n2, ctx=gpu_ctx)
    assert np.array_equal(idx[:, 0], np.arange(20, 70)) and np.array_equal(idx[:, 1], np.arange(100, 150))
    assert (dist == 0).all()
    ref = R.node_top2(d1, n1, d2, n2)
    assert np.array_equal(idx, ref[0]) and np.array_equal(dist, ref[1])
    i1, di1 = bm.node_match_arrays(d1, d2, n1, n2, k=1, ctx=gpu_ctx)
    assert i1.shape == (50, 1) and np.array_equal(i1[:, 0], idx[:, 0]) and np.array_equal(di1[:, 0], dist[:, 0])
    # a plateau of equal distances across a whole segment: prefix rows at the same length
    a2 = np.r_[np.full(70, 40), np.full(70, 44)]
    idx, dist = bm.node_match_arrays(prefix_rows([42, 40]), prefix_rows(a2), [0, 0], np.zeros(140, np.int64), ctx=gpu_ctx)
    assert idx.tolist() == [[0, 1], [0, 1]] and dist.tolist() == [[2, 2], [0, 0]]


# ---- image sizes --------------------------------------------------------------------------------------------------------------

SIZES = (0, 1, 63, 64, 65, 8191, 8192)


def sized_image(rng, n):
    """n rows over nodes of about 60 rows, one segment of several hundred rows under the largest id, and masked rows; in the
    two large images the sort's padding (8191) or nothing at all (8192) follows the masked rows."""
    nodes = rng.integers(0, max(1, n // 60), n) * 1000
    nodes[rng.random(n) < 0.07] = INT_MAX
    nodes[rng.random(n) < 0.03] = -1
    return rows(rng, n), nodes


@pytest.fixture(scope="module")
def sized(gpu_ctx):
    rng = np.random.default_rng(4003)
    images = [sized_image(rng, n) for n in SIZES]
    base = images[-1][0]
    for d, nodes in images[:-1]:               # the smaller images share rows with the largest one, so that rows do match
        d[:] = noisy(rng, base[:len(d)])
        nodes[:] = images[-1][1][:len(d)]
    return images


def test_image_sizes_on_each_side(bm, gpu_ctx, sized):
    small = SIZES.index(65)
    pairs = [(i, small) for i in range(len(SIZES))] + [(small, i) for i in range(len(SIZES))] + [(5, 6), (6, 5), (6, 6), (0, 0), (1, 1)]
    m, c = check(bm, gpu_ctx, sized, sized, pairs, th_low=256, ratio=1.0)
    assert c[pairs.index((6, 5))] > 4000 and c[pairs.index((0, small))] == 0 and len(m[pairs.index((0, small))]) == 0
    assert (m[pairs.index((small, 0))] == -1).all()


def test_feature_vectors_are_the_stable_argsort(bm, gpu_ctx, sized):
    fv = make_set(bm, gpu_ctx, sized)
    try:
        assert len(fv) == len(SIZES) and fv.offsets.tolist() == np.cumsum((0,) + SIZES).tolist()
        order, ns, ds = fv.order, fv.nodes_sorted, fv.descriptors_sorted
        for b, (d, nodes) in enumerate(sized):
            lo, hi = fv.offsets[b], fv.offsets[b + 1]
            want = np.argsort(np.asarray(nodes, np.int32).view(np.uint32), kind="stable")
            assert np.array_equal(order[lo:hi], want) and np.array_equal(ns[lo:hi], np.asarray(nodes, np.int32)[want])
            assert np.array_equal(order[lo:hi], R.group(nodes)[0]) and np.array_equal(ds[lo:hi], d[want])
            masked = int((np.asarray(nodes) < 0).sum())
            assert (ns[lo:hi][hi - lo - masked:] < 0).all() and (ns[lo:hi][:hi - lo - masked] >= 0).all()
    finally:
        fv.free()


# ---- batches ------------------------------------------------------------------------------------------------------------------

def test_batches_ragged_shared_and_single(bm, gpu_ctx):
    rng = np.random.default_rng(4004)
    base = rows(rng, 300)
    bnodes = rng.integers(0, 12, 300)          # the same ids in every image: rows of different pairs must never meet
    images2 = [(base, bnodes), (rows(rng, 0), np.zeros(0, np.int64)), (noisy(rng, base[:130]), bnodes[:130])]
    images1 = [(noisy(rng, base[50:250]), bnodes[50:250]), (rows(rng, 0), np.zeros(0, np.int64)), (noisy(rng, base[:77]), bnodes[:77]),
               (noisy(rng, base[100:165]), bnodes[100:165])]
    check(bm, gpu_ctx, images1, images2, [(0, 0)])                                            # B = 1
    ragged = [(0, 0), (1, 1), (2, 2)]
    m, c = check(bm, gpu_ctx, images1, images2, ragged)                                       # an empty image in the middle
    assert len(m[1]) == 0 and c[1] == 0 and c[0] > 100
    shared = [(0, 0), (2, 0), (3, 0), (1, 0), (0, 0)]                                         # one side-2 image for all pairs
    ms, cs = check(bm, gpu_ctx, images1, images2, shared)
    assert np.array_equal(ms[0], ms[4]) and np.array_equal(ms[0], m[0])
    mixed = [(3, 2), (0, 1), (1, 0), (2, 0), (0, 2)]
    mm, cm = check(bm, gpu_ctx, images1, images2, mixed)
    for p, (a, b) in enumerate(mixed):                                                        # every pair equals the single-pair call
        one, cnt = check(bm, gpu_ctx, [images1[a]], [images2[b]], [(0, 0)])
        assert np.array_equal(one[0], mm[p]) and cnt[0] == cm[p]


def test_batch_at_the_pair_limit(bm, gpu_ctx):
    rng = np.random.default_rng(4005)
    side = 64
    assert side * side == bm.PAIRS_MAX
    pool = rows(rng, 6)
    images1 = [(pool[rng.integers(0, 6, n)], rng.integers(-1, 2, n)) for n in rng.integers(0, 6, side)]
    images2 = [(pool[rng.integers(0, 6, n)], rng.integers(-1, 2, n)) for n in rng.integers(0, 6, side)]
    pairs = [(a, b) for a in range(side) for b in range(side)]
    m, c = check(bm, gpu_ctx, images1, images2, pairs, th_low=256, ratio=1.0)
    assert c.sum() > 100


# ---- selection ----------------------------------------------------------------------------------------------------------------

def test_selection_edges(bm, gpu_ctx):
    # one node per case; side 1 holds one row of prefix length 0 per node, so a distance is the prefix length on side 2
    cases = [([50, 200], True), ([51, 200], False),             # th_low = 50 inclusive
             ([29, 40], True), ([30, 40], False),               # ratio 0.75 of d1 = 40 is 30: strict
             ([191], True), ([192], False),                     # a lone candidate: d1 = 256, 0.75 * 256 = 192
             ([0, 0], False), ([0, 1], True)]                   # 0 < 0.75 * 0 is false
    a2 = np.concatenate([c[0] for c in cases])
    n2 = np.concatenate([np.full(len(c[0]), v) for v, c in enumerate(cases)])
    first = np.cumsum([0] + [len(c[0]) for c in cases])[:-1]
    image1, image2 = (prefix_rows(np.zeros(len(cases))), np.arange(len(cases))), (prefix_rows(a2), n2)
    m, c = check(bm, gpu_ctx, [image1], [image2], [(0, 0)], th_low=256)
    lone = [cases[v][1] or v in (0, 1) for v in range(len(cases))]        # without th_low the 50 / 51 pair passes the ratio
    assert m[0].tolist() == [int(first[v]) if lone[v] else -1 for v in range(len(cases))]
    m, c = check(bm, gpu_ctx, [image1], [image2], [(0, 0)])                # the defaults: th_low = 50, ratio = 0.75
    want = [v for v in range(len(cases)) if cases[v][1] and a2[first[v]] <= 50]
    assert np.flatnonzero(m[0] >= 0).tolist() == want and c[0] == len(want)
    assert m[0][0] == 0 and m[0][1] == -1 and m[0][2] == first[2] and m[0][3] == -1
    m, c = check(bm, gpu_ctx, [image1], [image2], [(0, 0)], th_low=256, ratio=1e9)          # keeps all but 0 < r * 0
    assert np.flatnonzero(m[0] < 0).tolist() == [6]
    for kw in (dict(th_low=-1), dict(ratio=0.0), dict(ratio=-1.0)):
        m, c = check(bm, gpu_ctx, [image1], [image2], [(0, 0)], **kw)                         # keeps none
        assert c[0] == 0 and (m[0] == -1).all()


def test_one_to_one(bm, gpu_ctx):
    # three side-1 rows name side-2 row 0 (prefix 100), two of them at distance 3; row 1 of side 2 (prefix 140) stays free
    image2 = (prefix_rows([100, 140, 7]), np.array([4, 4, 9]))
    image1 = (prefix_rows([105, 103, 97, 8]), np.array([4, 4, 4, 9]))
    m, c = check(bm, gpu_ctx, [image1], [image2], [(0, 0)])
    assert m[0].tolist() == [-1, 0, -1, 2] and c[0] == 2       # the lowest row of the two at distance 3; no loser falls back
    image1 = (prefix_rows([97, 103, 105, 8]), np.array([4, 4, 4, 9]))
    m, c = check(bm, gpu_ctx, [image1], [image2], [(0, 0)])
    assert m[0].tolist() == [0, -1, -1, 2]


# ---- rotation -----------------------------------------------------------------------------------------------------------------

def rotation_case(counts):
    """A pair of identical rows, one node each, so that every row matches its twin; `counts` {rotation: rows}."""
    r = np.concatenate([np.full(c, b) for b, c in counts.items()])
    n = len(r)
    bins2 = (np.arange(n) * 7) % 32
    bins1 = (bins2 + r) % 32
    d = prefix_rows(np.arange(n) % 257)
    return (d, np.arange(n)), bins1, bins2, r


@pytest.mark.parametrize("counts,kept", [
    ({5: 20, 9: 2, 11: 1}, {5, 9}),             # 10 * 2 >= 20
    ({5: 21, 9: 2, 11: 2}, {5}),                # 10 * 2 < 21
    ({30: 5, 3: 5, 20: 5, 8: 5}, {3, 8, 20}),   # a tie of counts: the lower bins are the three maxima
    ({0: 9, 31: 9, 16: 1}, {0, 31, 16}),        # 10 * 1 >= 9
    ({7: 10, 2: 1}, {7, 2}),                    # two bins only
    ({7: 11, 2: 1}, {7}),
    ({13: 4}, {13}),                            # one bin
])
def test_rotation_histogram(bm, gpu_ctx, counts, kept):
    image, bins1, bins2, r = rotation_case(counts)
    assert (bins1 < bins2).any() or len(counts) == 1             # wrap-around differences are among them
    m, c = check(bm, gpu_ctx, [image], [image], [(0, 0)], [bins1], [bins2])
    assert np.array_equal(m[0] >= 0, np.isin(r, list(kept))) and c[0] == int(np.isin(r, list(kept)).sum())
    assert np.array_equal(m[0][m[0] >= 0], np.flatnonzero(m[0] >= 0))
    m, c = check(bm, gpu_ctx, [image], [image], [(0, 0)])                                    # no bins: no check
    assert c[0] == len(r)


def test_rotation_per_pair_in_a_batch(bm, gpu_ctx):
    a, b = rotation_case({5: 20, 9: 2, 11: 1}), rotation_case({1: 3, 31: 30})
    m, c = check(bm, gpu_ctx, [a[0], b[0]], [a[0], b[0]], [(0, 0), (1, 1), (0, 0)], [a[1], b[1]], [a[2], b[2]])
    assert c.tolist() == [22, 33, 22]


# ---- determinism, residency ---------------------------------------------------------------------------------------------------

def test_same_bits_twice_and_under_both_scan_orders(bm, gpu_ctx, sized):
    rng = np.random.default_rng(4006)
    bins = [rng.integers(0, 32, n) for n in SIZES]
    fv = make_set(bm, gpu_ctx, sized)
    try:
        pairs = [(6, 5), (4, 6), (5, 5), (2, 3)]
        runs = [bm.search_by_bow(fv, fv, pairs, cat_bins(bins), cat_bins(bins), th_low=256, ratio=1.0, return_tables=True, scan_order=o)
                for o in (0, 0, 1, 1)]
        tables = [bm.node_top2(fv, fv, pairs, scan_order=o) for o in (0, 1)]
    finally:
        fv.free()
    for other in runs[1:]:
        assert other[1].tobytes() == runs[0][1].tobytes()
        for p in range(len(pairs)):
            assert other[0][p].tobytes() == runs[0][0][p].tobytes()
            assert other[2][p][0].tobytes() == runs[0][2][p][0].tobytes() and other[2][p][1].tobytes() == runs[0][2][p][1].tobytes()
    for p in range(len(pairs)):
        assert tables[0][p][0].tobytes() == tables[1][p][0].tobytes() == runs[0][2][p][0].tobytes()
    assert runs[0][1][0] > 300                   # (about three of 32 rotation bins of some 7900 matches)


def test_resident_rows_and_resident_feature_vectors(bm, gpu_ctx):
    rng = np.random.default_rng(4007)
    d2, n2 = rows(rng, 500), rng.integers(-1, 9, 500)
    d1, n1 = noisy(rng, d2[100:400]), n2[100:400]
    off1, off2 = [0, 120, 300], [0, 500]
    ref = [R.search(d1[:120], n1[:120], d2, n2), R.search(d1[120:], n1[120:], d2, n2)]
    host1, host2 = bm.FeatureVectors.from_nodes(d1, n1, off1, ctx=gpu_ctx), bm.FeatureVectors.from_nodes(d2, n2, off2, ctx=gpu_ctx)
    bufs = [gpu_ctx.upload(d1), gpu_ctx.upload(n1.astype(np.int32)), gpu_ctx.upload(d2), gpu_ctx.upload(n2.astype(np.int32))]
    dev1 = bm.FeatureVectors.from_nodes((bufs[0], 300), bufs[1], off1, ctx=gpu_ctx)
    dev2 = bm.FeatureVectors.from_nodes((bufs[2], 500), bufs[3], off2, ctx=gpu_ctx)
    cold = bm.FeatureVectors.from_nodes(d2, n2, off2, keep_on_device=False, ctx=gpu_ctx)
    try:
        assert cold.device is None and np.array_equal(cold.order, dev2.order) and np.array_equal(host2.nodes_sorted, dev2.nodes_sorted)
        pairs = [(0, 0), (1, 0)]
        for f1, f2 in ((host1, host2), (dev1, dev2), (dev1, cold), (dev1, dev2)):      # built once, searched more than once
            m, c = bm.search_by_bow(f1, f2, pairs, ctx=gpu_ctx)
            for p in range(2):
                assert np.array_equal(m[p], ref[p][0]) and c[p] == ref[p][1]
        with pytest.raises(ValueError):
            bm.FeatureVectors.from_nodes((bufs[0], 301), bufs[1], [0, 301], ctx=gpu_ctx)      # more rows than the buffer holds
    finally:
        for o in (host1, host2, dev1, dev2, cold, *bufs):
            o.free()


# ---- end to end ---------------------------------------------------------------------------------------------------------------

def test_vocabulary_to_correspondences_to_pose(bm, gpu_ctx):
    import bow_ref
    from backend import Backend
    from slamhip import bow
    from test_bow_gpu import random_tree

    rng = np.random.default_rng(4008)
    tree = random_tree(rng, 6, 4, p_leaf=0.1)
    vocab = bow.Vocabulary.from_arrays(**tree)
    leaves = np.flatnonzero(tree["child_count"] == 0)
    scene = noisy(rng, tree["node_desc"][rng.choice(leaves, 300)], flips=12)                  # 300 landmarks near the words
    kf_src, fr_src = rng.permutation(300), rng.permutation(300)
    kf = np.concatenate([noisy(rng, scene[kf_src], 2), rows(rng, 80)])                       # two views, and distractors
    fr = np.concatenate([noisy(rng, scene[fr_src], 2), rows(rng, 120)])
    other = rows(rng, 150)
    kf_all, kf_off = np.concatenate([other, kf]), [0, 150, 150 + len(kf)]
    bins_kf, bins_fr = rng.integers(0, 32, len(kf_all)), rng.integers(0, 32, len(fr))
    bins_kf[150:450] = (bins_fr[np.argsort(fr_src)][kf_src] + 3) % 32                        # the true matches turn by three bins
    try:
        for up in (2, 0, 4):
            f1 = bm.bow_feature_vectors(vocab, kf_all, kf_off, levels_up=up, ctx=gpu_ctx)
            f2 = bm.bow_feature_vectors(vocab, fr, [0, len(fr)], levels_up=up, ctx=gpu_ctx)
            try:
                n_kf, n_fr = bow_ref.transform(tree, kf_all, up)[1], bow_ref.transform(tree, fr, up)[1]
                for bins in ((None, None), (bins_kf, bins_fr)):
                    m, c = bm.search_by_bow(f1, f2, [(1, 0), (0, 0)], bins[0], bins[1], ctx=gpu_ctx)
                    for p, (lo, hi) in enumerate(((150, len(kf_all)), (0, 150))):
                        ref = R.search(kf_all[lo:hi], n_kf[lo:hi], fr, n_fr, None if bins[0] is None else bins[0][lo:hi], bins[1])
                        assert np.array_equal(m[p], ref[0]) and c[p] == ref[1], (up, p)
                one, cnt = bm.search_by_bow_descriptors(vocab, kf, fr, levels_up=up, ctx=gpu_ctx)
                assert np.array_equal(one, bm.search_by_bow(f1, f2, [(1, 0)], ctx=gpu_ctx)[0][0]) and cnt == (one >= 0).sum()
                if up == 2:
                    pairs = Backend().match_by_bow(f1, f2, [1, 0], keyframe_bins=bins_kf, frame_bins=bins_fr)
            finally:
                f1.free()
                f2.free()
    finally:
        vocab.free()
    (i1, i2), (j1, j2) = pairs
    assert i1.dtype == i2.dtype == np.int32 and len(i1) == len(i2) > 200 and (np.diff(i1) > 0).all() and len(np.unique(i2)) == len(i2)
    right = (i1 < 300) & (i2 < 300)
    same = kf_src[i1[right]] == fr_src[i2[right]]                                            # the same landmark on both sides
    assert right.sum() > 200 and same.mean() > 0.95
    assert len(j1) == len(j2) < 20
    # the form relocalize takes: (map points of the keyframe's rows, pixels of the frame's rows)
    fx, fy, cx, cy = 500.0, 500.0, 320.0, 240.0
    X = np.c_[rng.uniform(-2, 2, (300, 2)), rng.uniform(4, 9, 300)]
    points_kf = np.concatenate([X[kf_src], rng.uniform(-2, 2, (80, 3)) + [0, 0, 6]])
    Xf = np.concatenate([X[fr_src], rng.uniform(-2, 2, (120, 3)) + [0, 0, 6]])
    pixels_fr = np.c_[fx * Xf[:, 0] / Xf[:, 2] + cx, fy * Xf[:, 1] / Xf[:, 2] + cy]
    poses, counts, masks = Backend().relocalize([(points_kf[i1], pixels_fr[i2])], fx, fy, cx, cy)
    assert counts[0] >= 0.9 * same.sum() and len(masks[0]) == len(i1)
    assert np.allclose(poses[0], np.eye(4), atol=1e-4)


# ---- errors -------------------------------------------------------------------------------------------------------------------

def test_invalid_calls_launch_nothing_and_leave_the_context_usable(bm, gpu_ctx):
    from slamhip import SlamHipError
    from slamhip._lib import BowGroups, addr

    rng = np.random.default_rng(4009)
    d, nodes = rows(rng, 100), rng.integers(0, 4, 100)
    fv = bm.FeatureVectors.from_nodes(d, nodes, [0, 40, 100], ctx=gpu_ctx)
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    out = gpu_ctx.malloc(1 << 16)
    try:
        gpu_ctx.sync()
        before = out.download(np.uint8, (1 << 16,))
        good_off = fv.offsets
        long_off = np.array([0, bm.ROWS_MAX + 1], np.int64)
        down_off = np.array([0, 50, 40], np.int64)
        pairs = np.array([[0, 1], [1, 0]], np.int32)

        def groups(off, B, desc=fv.device[0].ptr):
            return BowGroups(desc, fv.device[1].ptr, fv.device[2].ptr, fv.device[3].ptr, None, addr(off), B)

        g = groups(good_off, 2)

        def search(g1=g, g2=g, p=addr(pairs), P=2, th=50, ratio=0.75, order=0, m=out.ptr, c=out.ptr + 4096, i=None, dd=None, ctx=h):
            return lib.slam_bow_match_search(ctx, ctypes.byref(g1) if g1 else None, ctypes.byref(g2) if g2 else None, p, P, th, ratio, order,
                                             m, c, i, dd)

        bad = [search(ctx=None), search(g1=None), search(g2=None), search(p=None), search(P=bm.PAIRS_MAX + 1), search(P=-1),
               search(g1=groups(long_off, 1)), search(g2=groups(down_off, 2)), search(g1=groups(good_off, 2, desc=None)),
               search(p=addr(np.array([[0, 2], [0, 0]], np.int32))), search(p=addr(np.array([[-1, 0], [0, 0]], np.int32))),
               search(order=2), search(ratio=float("nan")), search(m=None), search(c=None), search(i=out.ptr + 8192),
               lib.slam_bow_match_top2(h, ctypes.byref(g), ctypes.byref(g), addr(pairs), 2, 0, None, None),
               lib.slam_bow_match_top2(h, ctypes.byref(g), ctypes.byref(g), addr(pairs), 2, 0, out.ptr, None),
               lib.slam_bow_match_group(h, fv.device[0].ptr, fv.device[1].ptr, addr(long_off), 1, out.ptr, out.ptr, out.ptr, out.ptr),
               lib.slam_bow_match_group(h, None, fv.device[1].ptr, addr(good_off), 2, out.ptr, out.ptr, out.ptr, out.ptr),
               lib.slam_bow_match_group(h, fv.device[0].ptr, fv.device[1].ptr, None, 2, out.ptr, out.ptr, out.ptr, out.ptr),
               lib.slam_bow_match_group(None, fv.device[0].ptr, fv.device[1].ptr, addr(good_off), 2, out.ptr, out.ptr, out.ptr, out.ptr)]
        assert bad == [-1] * len(bad)
        with pytest.raises(SlamHipError):
            bm.plan_describe(1, bm.ROWS_MAX + 1)
        for call in (lambda: bm.search_by_bow(fv, fv, [(0, 2)]), lambda: bm.search_by_bow(fv, fv, [(0, 0)], bins1=np.full(100, 32), bins2=np.zeros(100, int)),
                     lambda: bm.node_match_arrays(d, d, nodes, nodes, k=3, ctx=gpu_ctx),
                     lambda: bm.FeatureVectors.from_nodes(np.zeros((8193, 32), np.uint8), np.zeros(8193, int), ctx=gpu_ctx)):
            with pytest.raises(ValueError):
                call()
        gpu_ctx.sync()
        assert np.array_equal(out.download(np.uint8, (1 << 16,)), before)        # nothing was written
        assert gpu_ctx.state_dirty() == 0
        assert search() == 0                                                     # and the same call with valid arguments succeeds
        m, c = bm.search_by_bow(fv, fv, [(0, 1), (1, 0)], ctx=gpu_ctx)
        ref = R.search(d[:40], nodes[:40], d[40:], nodes[40:])
        assert np.array_equal(m[0], ref[0]) and c[0] == ref[1]
        assert np.array_equal(out.download(np.int32, (100,))[:40], ref[0])
        # empty sides are no error
        empty = bm.FeatureVectors.from_nodes(np.zeros((0, 32), np.uint8), np.zeros(0, int), ctx=gpu_ctx)
        m, c = bm.search_by_bow(empty, fv, [(0, 0)], ctx=gpu_ctx)
        assert len(m[0]) == 0 and c.tolist() == [0]
        m, c = bm.search_by_bow(fv, empty, [(1, 0)], ctx=gpu_ctx)
        assert (m[0] == -1).all() and len(m[0]) == 60 and c.tolist() == [0]
        empty.free()
        assert gpu_ctx.state_dirty() == 0
    finally:
        out.free()
        fv.free()
