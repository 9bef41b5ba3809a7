"""Bag-of-words place recognition on the device (slam_bow_*, slamhip/bow.py) against tests/bow_ref.py: bit for bit unless a
test says otherwise.  The shapes are the smallest at which each path is taken: trees whose descent leaves the rows staged in
LDS, images at the limit of the LDS sort, databases around one and two LDS passes of the query."""
import os

import numpy as np
import pytest

import bow_ref as R
from hamming_families import prefix_rows
from test_bow_cpu import PREFIX_NODES, PREFIX_QUERIES, PREFIX_WORDS, prefix_tree

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def random_tree(rng, k, depth, p_leaf=0.3, full=False, cap=30000):
    """A breadth-first random tree: inner nodes have 1..k children (k when full), leaves sit at mixed depths, word ids are a
    shuffled table, and some siblings repeat their neighbour's centre."""
    begin, count, level = [0], [0], [0]
    v = 0
    while v < len(begin):
        if level[v] < depth and (v == 0 or full or (rng.random() >= p_leaf and len(begin) < cap)):
            c = k if full else int(rng.integers(1, k + 1))
            begin[v], count[v] = len(begin), c
            begin += [0] * c
            count += [0] * c
            level += [level[v] + 1] * c
        v += 1
    n = len(begin)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    if not full:
        for v in np.flatnonzero(np.asarray(count) > 1)[::3]:
            c = int(rng.integers(1, count[v]))
            desc[begin[v] + c] = desc[begin[v] + c - 1]           # duplicate siblings: the tie goes to the lower child
    count = np.asarray(count, np.int32)
    leaves = np.flatnonzero(count == 0)
    won = np.full(n, -1, np.int32)
    won[leaves] = rng.permutation(len(leaves)).astype(np.int32)
    return {"k": k, "depth": depth, "node_desc": desc, "child_begin": np.asarray(begin, np.int32), "child_count": count,
            "word_of_node": won, "idf": rng.uniform(0.0, 9.0, len(leaves)) * (rng.random(len(leaves)) > 0.1)}


def queries_for(rng, v, n):
    """Random rows, rows equal to a centre, and rows a few bits away from one."""
    d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    pick = rng.integers(0, len(v["node_desc"]), n)
    near = v["node_desc"][pick].copy()
    flips = rng.integers(0, 256, (n, 3))
    for j in range(3):
        near[np.arange(n), flips[:, j] >> 3] ^= (128 >> (flips[:, j] & 7)).astype(np.uint8)
    d[1::3] = v["node_desc"][pick][1::3]
    d[2::3] = near[2::3]
    return d


def same_vocab(a, ref):
    for name in ("node_desc", "child_begin", "child_count", "word_of_node", "idf"):
        x, y = getattr(a, name), ref[name]
        assert x.shape == y.shape and np.array_equal(x, y), name
    assert a.idf.tobytes() == ref["idf"].tobytes()


@pytest.fixture(scope="module")
def bow(gpu_ctx):
    from slamhip import bow as module
    return module


@pytest.fixture(scope="module")
def scene():
    base, off, qd, qoff = R.scene()
    ref = R.train(base, off, 8, 3)
    ev, qv = R.vectors(ref, base, off), R.vectors(ref, qd, qoff)
    rows = lambda x: [(x[1][x[0][i]:x[0][i + 1]], x[2][x[0][i]:x[0][i + 1]], x[3][x[0][i]:x[0][i + 1]]) for i in range(len(x[0]) - 1)]
    s, c = R.dense(rows(ev), rows(qv))
    return {"base": base, "off": off, "qd": qd, "qoff": qoff, "ref": ref, "ev": ev, "qv": qv, "erows": rows(ev), "qrows": rows(qv),
            "s": s, "c": c}


# ---- transform --------------------------------------------------------------------------------------------------------------

def test_transform_prefix_tree(bow, gpu_ctx):
    v = bow.Vocabulary.from_arrays(**prefix_tree())
    for up, nodes in PREFIX_NODES.items():
        for lanes in (0, 1, 16):
            w, n = bow.bow_transform(v, prefix_rows(PREFIX_QUERIES), levels_up=up, ctx=gpu_ctx, lanes=lanes)
            assert w.tolist() == PREFIX_WORDS and n.tolist() == nodes, (up, lanes)
    v.free()


@pytest.mark.parametrize("k,depth", [(2, 1), (3, 10), (10, 4), (16, 3), (32, 2)])
def test_transform_random_trees(bow, gpu_ctx, k, depth):
    rng = np.random.default_rng(100 * k + depth)
    ref = random_tree(rng, k, depth, p_leaf=0.15 if depth == 10 else 0.3)
    assert depth < 3 or len(set(ref["child_count"][ref["child_count"] > 0].tolist())) > 1
    v = bow.Vocabulary.from_arrays(**ref)
    d = queries_for(rng, ref, 2000)
    for n in (0, 1, 63, 64, 65, 2000):
        for up in ((0, 2, depth, depth + 3) if n in (65, 2000) else (0,)):
            rw, rn = R.transform(ref, d[:n], up)
            for lanes in (1, 16):                                   # one lane per descriptor, and sixteen
                w, nodes = bow.bow_transform(v, d[:n], levels_up=up, ctx=gpu_ctx, lanes=lanes)
                assert w.dtype == np.int32 and np.array_equal(w, rw) and np.array_equal(nodes, rn), (n, up, lanes)
    v.free()


def test_transform_full_tree_beyond_the_staged_rows(bow, gpu_ctx):
    rng = np.random.default_rng(106)
    ref = random_tree(rng, 10, 6, full=True)
    assert len(ref["node_desc"]) == 1111111
    v = bow.Vocabulary.from_arrays(**ref)
    d = queries_for(rng, ref, 2000)
    for up, lanes in ((0, 1), (2, 1), (0, 16), (0, 0)):
        w, nodes = bow.bow_transform(v, d, levels_up=up, ctx=gpu_ctx, lanes=lanes)
        rw, rn = R.transform(ref, d, up)
        assert np.array_equal(w, rw) and np.array_equal(nodes, rn), (up, lanes)
    v.free()


def test_transform_lane_rule_on_both_sides(bow, gpu_ctx):
    """lanes = 0 at the last size that takes sixteen lanes per descriptor and at the first that takes one."""
    edge = bow.limits()["lanes16_up_to"]
    rng = np.random.default_rng(9)
    ref = random_tree(rng, 4, 2)
    v = bow.Vocabulary.from_arrays(**ref)
    d = queries_for(rng, ref, edge + 1)
    rw, rn = R.transform(ref, d, 1)
    for n in (edge, edge + 1):
        w, nodes = bow.bow_transform(v, d[:n], levels_up=1, ctx=gpu_ctx)
        assert np.array_equal(w, rw[:n]) and np.array_equal(nodes, rn[:n]), n
    v.free()


# ---- vectors ----------------------------------------------------------------------------------------------------------------

def test_vectors_batch(bow, gpu_ctx):
    rng = np.random.default_rng(7)
    ref = random_tree(rng, 10, 4)
    v = bow.Vocabulary.from_arrays(**ref)
    one = rng.integers(0, 256, (1, 32), dtype=np.uint8)
    d = np.concatenate([queries_for(rng, ref, 300), np.repeat(one, 50, 0), queries_for(rng, ref, 8192), queries_for(rng, ref, 1)])
    off = np.array([0, 300, 300, 350, 350 + 8192, 350 + 8193], np.int64)       # an empty image, one repeated row, an image at the limit
    got = bow.bow_vectors(v, d, off, ctx=gpu_ctx)
    ro, rw, rv, rq = R.vectors(ref, d, off)
    assert np.array_equal(got.offsets, ro) and np.array_equal(got.words, rw) and np.array_equal(got.q, rq)
    assert got.values.tobytes() == rv.tobytes()                                 # raw f64 bits
    assert ro[2] == ro[1] and ro[3] - ro[2] <= 1
    row = got[3]
    assert len(row) == 1 and np.array_equal(row.words, rw[ro[3]:ro[4]]) and row.values.tobytes() == rv[ro[3]:ro[4]].tobytes()
    with pytest.raises(ValueError):
        bow.bow_vectors(v, np.zeros((8193, 32), np.uint8), [0, 8193], ctx=gpu_ctx)
    empty = bow.bow_vectors(v, np.zeros((0, 32), np.uint8), [0], ctx=gpu_ctx)
    assert len(empty) == 0 and empty.offsets.tolist() == [0]
    v.free()


def test_vectors_repeated_row_and_zero_idf(bow, gpu_ctx):
    tree = prefix_tree()
    v = bow.Vocabulary.from_arrays(**tree)
    got = bow.bow_vectors(v, prefix_rows([250] * 40 + [80] * 3), [0, 40, 43], ctx=gpu_ctx)
    assert got.offsets.tolist() == [0, 1, 2] and got.words.tolist() == [4, 1] and got.values.tolist() == [1.0, 1.0]
    assert got.q.tolist() == [1 << 31, 1 << 31]
    v.free()
    tree["idf"] = np.zeros(6)
    z = bow.Vocabulary.from_arrays(**tree)
    got = bow.bow_vectors(z, prefix_rows(PREFIX_QUERIES), [0, 5], ctx=gpu_ctx)
    assert got.offsets.tolist() == [0, 0] and len(got.words) == 0
    z.free()


# ---- database ---------------------------------------------------------------------------------------------------------------

def as_vectors(bow, rows):
    off = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r[0]) for r in rows], out=off[1:])
    cat = lambda i, dt: np.concatenate([r[i] for r in rows]).astype(dt) if rows else np.zeros(0, dt)
    return bow.BowVectors(off, cat(0, np.int32), cat(1, np.float64), cat(2, np.uint32))


def test_database_scene_scores_and_order(bow, gpu_ctx, scene):
    v = bow.Vocabulary.from_arrays(**scene["ref"])
    db = bow.BowDatabase(v, gpu_ctx, capacity=64)                              # the store grows on the way
    ids, sc, cm = db.query(as_vectors(bow, scene["qrows"][:2]), 5)              # an empty database
    assert (ids == -1).all() and (sc == 0).all() and (cm == 0).all()
    assert db.scores_dense(as_vectors(bow, scene["qrows"][:2]))[0].shape == (2, 0)
    for r in scene["erows"][:40]:
        db.add(as_vectors(bow, [r]))
    q = as_vectors(bow, scene["qrows"])
    s40, c40 = db.scores_dense(q)
    assert np.array_equal(s40, scene["s"][:, :40]) and np.array_equal(c40, scene["c"][:, :40])
    assert list(db.add_vectors(as_vectors(bow, scene["erows"][40:]))) == list(range(40, 64))      # add between two queries
    planted = [scene["erows"][5], scene["erows"][5], scene["erows"][17]]
    assert [db.add(as_vectors(bow, [r])) for r in planted] == [64, 65, 66] and len(db) == 67
    s_ref = np.c_[scene["s"], scene["s"][:, [5, 5, 17]]]
    c_ref = np.c_[scene["c"], scene["c"][:, [5, 5, 17]]]
    s, c = db.scores_dense(q)
    assert s.dtype == np.uint32 and np.array_equal(s, s_ref) and np.array_equal(c, c_ref)
    for i in range(64):                                                         # the derived bound against DBoW2's f64 formula
        for j in (i, (i + 1) % 64):
            l1 = R.score_l1(scene["qrows"][i][0], scene["qrows"][i][1], scene["erows"][j][0], scene["erows"][j][1])
            assert -1e-12 <= l1 - s[i, j] / 2.0 ** 31 < c[i, j] * 2.0 ** -31 + 1e-12
    for R_, max_id in ((1, None), (10, None), (64, None), (10, 30), (10, 65), (10, 67), (10, 1000), (3, 0), (64, 20)):   # (64, 20): 44 fillers
        got = db.query(q, R_, max_id)
        ref = R.query(s_ref, c_ref, R_, max_id)
        for a, b in zip(got, ref):
            assert a.dtype == b.dtype and np.array_equal(a, b), (R_, max_id)
    ids, sc, cm = db.query(q, 3)
    assert ids[5].tolist() == [5, 64, 65] and sc[5, 0] == sc[5, 1] == sc[5, 2]   # equal scores by ascending id
    assert (ids[:, 0] == np.where(np.arange(64) == 17, 17, np.arange(64))).all()
    for Q in (1, 3, 257):                                                       # many queries in one call; an empty query among them
        pick = [scene["qrows"][i % 64] for i in range(Q)]
        if Q == 3:
            pick[1] = (np.zeros(0, np.int32), np.zeros(0), np.zeros(0, np.uint32))
        got = db.query(as_vectors(bow, pick), 12)
        rs, rc = s_ref[np.arange(Q) % 64].copy(), c_ref[np.arange(Q) % 64].copy()
        if Q == 3:
            rs[1], rc[1] = 0, 0
        for a, b in zip(got, R.query(rs, rc, 12)):
            assert np.array_equal(a, b), Q
        again = db.query(as_vectors(bow, pick), 12)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))      # two runs identical
    for bad in (0, 65):
        with pytest.raises(ValueError):
            db.query(q, bad)
    with pytest.raises(ValueError):
        db.add(bow.BowVectors(np.array([0, 2]), np.array([7, 3], np.int32), np.zeros(2), np.ones(2, np.uint32)))
    db.free()
    v.free()


def test_database_around_the_lds_pass(bow, gpu_ctx):
    """Entries of two or three words out of 16, one of them held by every entry, at E = capacity - 1, capacity, capacity + 1
    and 2 * capacity + 3 of one LDS pass; the best entries are planted behind the first pass."""
    cap = bow.limits()["query_pass_entries"]
    rng = np.random.default_rng(3)
    ref = random_tree(rng, 4, 2, full=True)
    v = bow.Vocabulary.from_arrays(**ref)
    E = 2 * cap + 3
    table = np.zeros((E, 16), np.uint32)
    table[:, 0] = rng.integers(1, 1 << 20, E)                                    # word 0: in every entry
    second = rng.integers(1, 16, E)
    table[np.arange(E), second] = rng.integers(1, 1 << 29, E)
    third = rng.integers(1, 16, E)
    table[np.arange(E)[::2], third[::2]] = rng.integers(1, 1 << 29, (E + 1) // 2)
    for e in (cap - 1, cap, cap + 1, 2 * cap, 2 * cap + 2, 7, 8):
        table[e] = 0
        table[e, [0, 3, 9]] = [1 << 20, 1 << 29, 1 << 29]                        # equal best scores on both sides of every boundary
    qt = np.zeros((2, 16), np.uint32)
    qt[0, [0, 3, 9, 12]] = [1 << 22, 1 << 30, 1 << 29, 5]
    qt[1, [5]] = [1 << 30]
    to_rows = lambda t: [(np.flatnonzero(r).astype(np.int32), np.zeros(int((r > 0).sum())), r[r > 0]) for r in t]
    q = as_vectors(bow, to_rows(qt))
    db = bow.BowDatabase(v, gpu_ctx)
    at = 0
    for size in (cap - 1, cap, cap + 1, E):
        db.add_vectors(as_vectors(bow, to_rows(table[at:size])))
        at = size
        s_ref, c_ref = R.dense_from_tables(table[:size], qt)
        s, c = db.scores_dense(q)
        assert np.array_equal(s, s_ref) and np.array_equal(c, c_ref), size
        for R_, max_id in ((64, None), (5, cap), (5, size - 1)):
            for a, b in zip(db.query(q, R_, max_id), R.query(s_ref, c_ref, R_, max_id)):
                assert np.array_equal(a, b), (size, R_, max_id)
    ids, _, cm = db.query(q, 8)
    assert ids[0, :7].tolist() == [7, 8, cap - 1, cap, cap + 1, 2 * cap, 2 * cap + 2] and cm[0, :7].tolist() == [3] * 7
    db.free()
    v.free()


# ---- training ---------------------------------------------------------------------------------------------------------------

def test_training_scene_and_the_scene_end_to_end(bow, gpu_ctx, scene):
    v = bow.train_vocabulary(scene["base"], scene["off"], 8, 3, ctx=gpu_ctx)
    same_vocab(v, scene["ref"])
    db = bow.BowDatabase(v, gpu_ctx)
    ids = db.add_vectors(bow.bow_vectors(v, scene["base"], scene["off"], ctx=gpu_ctx))
    assert list(ids) == list(range(64))
    qv = bow.bow_vectors(v, scene["qd"], scene["qoff"], keep_on_device=True, ctx=gpu_ctx)
    top, sc, cm = db.query(qv, 2)
    s, c = db.scores_dense(qv)
    qv.free()
    assert (top[:, 0] == np.arange(64)).sum() == 64 and sc[:, 0].min() > sc[:, 1].max()
    assert np.array_equal(s, scene["s"]) and np.array_equal(c, scene["c"])      # the reference's integer scores
    db.free()
    v.free()


@pytest.mark.parametrize("case", ["identical groups", "n < k", "n = 1", "max_iters binds", "ragged images"])
def test_training_equals_reference(bow, gpu_ctx, case):
    rng = np.random.default_rng(41)
    iters = 16
    if case == "identical groups":
        seeds = rng.integers(0, 256, (5, 32), dtype=np.uint8)
        d = np.repeat(seeds, [300, 1, 200, 40, 7], axis=0)[rng.permutation(548)]
        d = np.concatenate([d, rng.integers(0, 256, (60, 32), dtype=np.uint8)])
        off, k, depth = [0, 100, 100, 400, 608], 4, 3
    elif case == "n < k":
        d, off, k, depth = rng.integers(0, 256, (3, 32), dtype=np.uint8), [0, 2, 3], 8, 2
    elif case == "n = 1":
        d, off, k, depth = rng.integers(0, 256, (1, 32), dtype=np.uint8), [0, 1], 10, 6
    elif case == "max_iters binds":
        d, off, k, depth, iters = rng.integers(0, 256, (3000, 32), dtype=np.uint8), [0, 1000, 3000], 4, 2, 2
        assert not np.array_equal(R.train(d, off, k, depth, 2)["node_desc"], R.train(d, off, k, depth, 16)["node_desc"])
    else:
        d, off, k, depth = rng.integers(0, 256, (700, 32), dtype=np.uint8), [0, 0, 513, 513, 700], 32, 2
    v = bow.train_vocabulary(d, off, k, depth, max_iters=iters, ctx=gpu_ctx)
    same_vocab(v, R.train(d, off, k, depth, iters))
    v.free()


# ---- resident descriptors, the backend, argument errors -------------------------------------------------------------------

def test_resident_descriptors_never_leave_the_device(bow, gpu_ctx, scene):
    from slamhip import orb

    img = np.load(os.path.join(HERE, "golden", "orb_desk_320x240.npz"))["image"]
    res = orb.orb_extract_arrays(np.stack([img, img[::-1].copy()]), n_features=200, ctx=gpu_ctx, keep_on_device=True)
    v = bow.Vocabulary.from_arrays(**scene["ref"])
    try:
        for b in range(2):
            block = res.device_descriptors(b)
            assert block[1] == len(res.descriptors[b]) > 50
            for up in (0, 1):
                dev, host = bow.bow_transform(v, block, levels_up=up, ctx=gpu_ctx), bow.bow_transform(v, res.descriptors[b], levels_up=up, ctx=gpu_ctx)
                assert np.array_equal(dev[0], host[0]) and np.array_equal(dev[1], host[1])
                assert np.array_equal(dev[0], R.transform(scene["ref"], res.descriptors[b], up)[0])
            a, h = bow.bow_vectors(v, block, [0, block[1]], ctx=gpu_ctx), bow.bow_vectors(v, res.descriptors[b], [0, block[1]], ctx=gpu_ctx)
            assert np.array_equal(a.words, h.words) and a.values.tobytes() == h.values.tobytes()
    finally:
        res.free()
        v.free()


def test_backend_detect_loop_candidates(bow, gpu_ctx):
    from backend import Backend

    ref = random_tree(np.random.default_rng(3), 4, 2, full=True)
    v = bow.Vocabulary.from_arrays(**ref)
    table = np.zeros((6, 16), np.uint32)
    table[0, [1, 2, 3, 4, 5]] = [100, 100, 100, 100, 100]          # 5 shared words, score 500
    table[1, [1, 2, 3, 4]] = [300, 300, 100, 100]                  # 4 shared (not > 0.8 * 5): dropped
    table[2, [1, 2, 3, 4, 5]] = [200, 200, 200, 200, 200]          # 5 shared, score 1000, but connected
    table[3, [1, 2, 3, 4, 5, 6]] = [100, 100, 100, 100, 100, 7]    # as entry 0: the tie goes to the lower id
    table[4, [9]] = [1 << 30]                                      # shares nothing
    table[5, [1, 2, 3, 4, 5]] = [50, 50, 50, 50, 50]               # 5 shared, score 250: below min_score
    q = np.zeros((1, 16), np.uint32)
    q[0, [1, 2, 3, 4, 5]] = 1 << 28
    to_rows = lambda t: [(np.flatnonzero(r).astype(np.int32), np.zeros(int((r > 0).sum())), r[r > 0]) for r in t]
    db = bow.BowDatabase(v, gpu_ctx)
    db.add_vectors(as_vectors(bow, to_rows(table)))
    ids, sc = Backend().detect_loop_candidates(db, as_vectors(bow, to_rows(q)), connected=[2], min_score=300 / 2.0 ** 31)
    assert ids.tolist() == [0, 3] and sc.tolist() == [500 / 2.0 ** 31] * 2
    ids, sc = Backend().detect_loop_candidates(db, as_vectors(bow, to_rows(q)))
    assert ids.tolist() == [2, 0, 3, 5]
    with pytest.raises(ValueError):
        Backend().detect_loop_candidates(db, as_vectors(bow, to_rows(q)), connected=[6])
    db.free()
    v.free()


def test_argument_errors(bow, gpu_ctx):
    import ctypes

    from slamhip import _lib

    v = bow.Vocabulary.from_arrays(**prefix_tree())
    with pytest.raises(ValueError):
        bow.bow_transform(v, np.zeros((3, 32), np.uint8), offsets=[0, 2], ctx=gpu_ctx)
    with pytest.raises(ValueError):
        bow.bow_vectors(v, np.zeros((3, 32), np.uint8), [0, 2, 1, 3], ctx=gpu_ctx)
    buf = gpu_ctx.malloc(64)
    with pytest.raises(ValueError):
        bow.bow_transform(v, (buf, 3), ctx=gpu_ctx)
    dv = v.upload(gpu_ctx)
    lib = gpu_ctx.lib
    rc = lib.slam_bow_transform(gpu_ctx.handle, buf.ptr, 2, dv.node_desc.ptr, dv.child.ptr, dv.word_of_node.ptr, v.n_nodes, 11, 0, 0, buf.ptr, buf.ptr)
    assert rc == _lib.SLAM_ERR_INVALID and b"depth" in lib.slam_last_error()
    rc = lib.slam_bow_transform(gpu_ctx.handle, buf.ptr, 2, dv.node_desc.ptr, dv.child.ptr, dv.word_of_node.ptr, v.n_nodes, 2, 0, 8, buf.ptr, buf.ptr)
    assert rc == _lib.SLAM_ERR_INVALID and b"lanes" in lib.slam_last_error()
    with pytest.raises(ValueError):
        bow.bow_transform(v, np.zeros((3, 32), np.uint8), ctx=gpu_ctx, lanes=4)
    rc = lib.slam_bow_query(gpu_ctx.handle, buf.ptr, buf.ptr, buf.ptr, 1, buf.ptr, buf.ptr, 6, 4, 4, 65, buf.ptr, buf.ptr, buf.ptr, None, None)
    assert rc == _lib.SLAM_ERR_INVALID and b"max_results" in lib.slam_last_error()
    rc = lib.slam_bow_vectors(gpu_ctx.handle, buf.ptr, buf.ptr, 1, 2, dv.idf.ptr, 6, buf.ptr, 8, buf.ptr, buf.ptr, buf.ptr, buf.ptr)
    assert rc == _lib.SLAM_ERR_INVALID and b"workspace" in lib.slam_last_error()
    moved = ctypes.c_int64(0)
    rc = lib.slam_bow_train_step(gpu_ctx.handle, buf.ptr, 2, buf.ptr, 1, 33, buf.ptr, buf.ptr, buf.ptr, None, 0, None, None, buf.ptr, 0, ctypes.byref(moved))
    assert rc == _lib.SLAM_ERR_INVALID
    buf.free()
    v.free()
