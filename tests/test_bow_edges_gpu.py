"""GPU: slam_bow_* past the single-tile shapes of tests/test_bow_gpu.py, bit for bit against tests/bow_ref.py on
the cases of tests/bow_cases.py: child groups on either side of row 1152 of the one-lane transform, planted ties between the
children, malformed tables through the raw entry, images around every size at which the vectors kernel changes its partition,
more than 256 images in one call, ids outside the table, the counting sort past 4096 keys, a database over 4913 words, hits of
score 0 and of score 1 through the query, empty entries, a store that grows, trainings whose frontier passes 256 nodes and
whose row grouping and word count pass 4096 keys, the exact-half majority.  tests/test_bow_edges_cpu.py asserts, on the
reference alone, that each case has the property it is here for."""
import ctypes

import numpy as np
import pytest

import bow_cases as C
import bow_ref as R
from test_bow_gpu import as_vectors, same_vocab

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bow(gpu_ctx):
    from slamhip import bow as module
    return module


@pytest.fixture(scope="module")
def big_vocab(bow):
    """4913 words: more than one tile of the key scan, and not a multiple of it."""
    v = bow.Vocabulary.from_arrays(**C.full_tree(17, 3))
    yield v
    v.free()


# ---------------------------------------------------------------------------------------------------------------- helpers
def buffers(ctx):
    from slamhip.two_view import _Buffers
    return _Buffers(ctx)


def device_vectors(ctx, words, off, idf, n_words):
    """slam_bow_vectors on word ids as they are: (offsets, words, values, q); every output starts as 0xFF bytes."""
    from slamhip._lib import check

    B, n = len(off) - 1, len(words)
    m = buffers(ctx)
    try:
        need = ctypes.c_uint64(0)
        check(ctx.lib.slam_bow_vectors_workspace(B, n, ctypes.byref(need)))
        dw, do, di, ws = m.up(np.ascontiguousarray(words, np.int32)), m.up(np.ascontiguousarray(off, np.int64)), m.up(idf), m.new(need.value)
        out = [m.up(np.full(B + 1, -1, np.int64)), m.up(np.full(n + 4, -1, np.int32)), m.up(np.full(n + 4, -1, np.int64)),
               m.up(np.full(n + 4, -1, np.int32))]
        check(ctx.lib.slam_bow_vectors(ctx.handle, dw.ptr, do.ptr, B, n, di.ptr, n_words, ws.ptr, ws.nbytes, out[0].ptr, out[1].ptr,
                                       out[2].ptr, out[3].ptr))
        o = out[0].download(np.int64, (B + 1,))
        assert o[0] == 0 and (np.diff(o) >= 0).all() and o[-1] <= n, "offsets"
        t = int(o[-1])
        words_out, q = out[1].download(np.int32, (n + 4,)), out[3].download(np.uint32, (n + 4,))
        values = out[2].download(np.float64, (n + 4,))
        assert (words_out[t:] == -1).all() and (q[t:] == 0xFFFFFFFF).all(), "a slot past the total was written"
        return o, words_out[:t], values[:t], q[:t]
    finally:
        m.free()


def assert_vectors(got, ref):
    """Offsets, words and q equal, values equal as raw f64 bytes; and for every vector 2^31 - K < sum(q) <= 2^31, the premise
    of the no-carry argument of the score."""
    (o, w, v, q), (ro, rw, rv, rq) = got, ref
    assert np.array_equal(o, ro), "offsets"
    assert np.array_equal(w, rw), "words"
    assert v.tobytes() == rv.tobytes(), "values"
    assert q.dtype == np.uint32 and np.array_equal(q, rq), "q"
    for b in range(len(o) - 1):
        K = int(o[b + 1] - o[b])
        total = int(q[o[b]:o[b + 1]].astype(np.int64).sum())
        assert K == 0 or (1 << 31) - K < total <= (1 << 31), (b, K, total)


def vectors_case(ctx, case):
    words, off, idf, n_words = case[:4]
    got = device_vectors(ctx, words, off, idf, n_words)
    assert_vectors(got, R.vectors_of_words(words, off, idf, n_words))
    return got


def rows_of(vectors):
    o, w, v, q = vectors
    return [(w[o[b]:o[b + 1]], v[o[b]:o[b + 1]], q[o[b]:o[b + 1]]) for b in range(len(o) - 1)]


EMPTY = (np.zeros(0, np.int32), np.zeros(0), np.zeros(0, np.uint32))


def assert_queries(db, q, s_ref, c_ref, Rs, max_ids=(None,)):
    for R_ in Rs:
        for max_id in max_ids:
            for a, b, name in zip(db.query(q, R_, max_id), R.query(s_ref, c_ref, R_, max_id), ("ids", "scores", "common")):
                assert a.dtype == b.dtype and np.array_equal(a, b), (name, R_, max_id)


# -------------------------------------------------------------------------------------------------------------- 1: transform
@pytest.mark.parametrize("which", sorted(C.STAGED_COUNTS))
def test_transform_groups_at_row_1152(bow, gpu_ctx, which):
    """The group that ends on row 1152 (LDS), the one that starts there and the one that straddles it (memory): every leaf of
    the three groups around the line is reached by a planted query, under both lane mappings."""
    assert bow.limits()["staged_nodes"] == C.STAGE
    tree = C.staged_tree(which)
    q = C.staged_queries(tree)
    n = len(tree["node_desc"])
    for i, (leaf, parent) in enumerate(C.staged_targets(tree)):
        planted = C.staged_plant(tree, leaf, parent, q[i])
        v = bow.Vocabulary.from_arrays(**planted)
        for up, node in ((0, leaf), (1, parent)):
            rw, rn = R.transform(planted, q, up)
            for lanes in (1, 16):
                w, at = bow.bow_transform(v, q, levels_up=up, ctx=gpu_ctx, lanes=lanes)
                assert (int(w[i]), int(at[i])) == (n - 1 - leaf, node), (leaf, up, lanes)       # the closed form
                assert np.array_equal(w, rw) and np.array_equal(at, rn), (leaf, up, lanes)
        v.free()


@pytest.mark.parametrize("k", C.TIE_KS)
def test_transform_planted_ties_and_distance_256(bow, gpu_ctx, k):
    """Equal children across the eight-row batches of bow_nearest (7 | 8, 15 | 16), between a lane's first and second child
    (c | c + 16), all equal, only the last, and distance 256 everywhere: the lowest child wins under both mappings."""
    for name, tree, q, win in C.tie_cases(k):
        v = bow.Vocabulary.from_arrays(**tree)
        rw, rn = R.transform(tree, q)
        for lanes in (1, 16):
            w, at = bow.bow_transform(v, q, ctx=gpu_ctx, lanes=lanes)
            assert np.array_equal(at, (1 + win).astype(np.int32)) and np.array_equal(w, tree["word_of_node"][1 + win]), (name, lanes)
            assert np.array_equal(w, rw) and np.array_equal(at, rn), (name, lanes)
        v.free()


@pytest.mark.parametrize("lanes", [1, 16])
def test_transform_raw_entry_clamps(gpu_ctx, lanes):
    """slam_bow_transform on tables that from_arrays refuses: a negative child_begin, one at and one above n_nodes, a
    child_count of 40, a range past n_nodes, a cycle through the root and a chain deeper than depth (word -1).  The tables are
    views into the middle of larger allocations whose spare rows are bait (bow_cases.raw_case): a read outside the view stays
    inside the test's own memory and changes the answer."""
    from slamhip._lib import check

    c = C.raw_case()
    f, n = c["front"], len(c["desc"])
    rows, child, won = C.raw_views(c)
    m = buffers(gpu_ctx)
    try:
        d_rows, d_child, d_won, d_desc = m.up(c["rows_full"]), m.up(c["child_full"]), m.up(c["won_full"]), m.up(c["desc"])
        assert d_rows.nbytes == 32 * (f + c["n_nodes"] + c["back"])
        for up in (0, 1):
            dw, dn = m.up(np.full(n, -7, np.int32)), m.up(np.full(n, -7, np.int32))
            check(gpu_ctx.lib.slam_bow_transform(gpu_ctx.handle, d_desc.ptr, n, d_rows.ptr + 32 * f, d_child.ptr + 8 * f, d_won.ptr + 4 * f,
                                                 c["n_nodes"], c["depth"], up, lanes, dw.ptr, dn.ptr))
            w, at = dw.download(np.int32, (n,)), dn.download(np.int32, (n,))
            rw, rn = R.transform_raw(c["desc"], rows, child, won, c["n_nodes"], c["depth"], up)
            assert (w != C.RAW_WORD_OUTSIDE).all() and (at >= 0).all() and (at < c["n_nodes"]).all(), up
            assert np.array_equal(w, rw) and np.array_equal(at, rn), up
            assert (w[c["kind"] == 6] == -1).all()                               # the chain cut at depth 3 ends on an inner node
    finally:
        m.free()


# ---------------------------------------------------------------------------------------------------------------- 2: vectors
def test_vectors_image_sizes_around_every_partition(gpu_ctx):
    """Images of 1, 2, 3, 255 .. 257, 511 .. 513 and 4095 .. 4097 ids in one call, an empty image between any two."""
    got = vectors_case(gpu_ctx, C.vector_sizes_case())
    assert len(got[0]) == 26


def test_vectors_full_images_runs_and_a_zero_q(gpu_ctx):
    """Five images over 10 000 words: 8192 distinct ids descending (U = K = 8192), 8192 copies of one id (one run over every
    thread's chunk), idf 0 and idf > 0 alternating (kept != U in every chunk), only words of idf 0 between two vectors (K = 0),
    and weights more than 2^31 apart (a stored q of 0)."""
    case = C.vector_full_case()
    o, w, v, q = vectors_case(gpu_ctx, case)
    assert np.diff(o).tolist() == [8192, 1, 904, 0, 4]
    assert q[o[1]] == 1 << 31 and q[o[4]] == 0 and v[o[4]] > 0 and w[o[4]] == C.FULL_TINY


def test_vectors_kept_lists_of_63_64_65_words(gpu_ctx):
    """Kept lists of exactly 1, 63, 64, 65, 128 and 129 words with idf values that are not dyadic: the 64 partial sums and
    their left-to-right total, equal as raw f64 bytes."""
    o = vectors_case(gpu_ctx, C.vector_kept_case())[0]
    assert np.diff(o).tolist() == list(C.KEPT_LENGTHS)


@pytest.mark.parametrize("B", C.MANY_IMAGES)
def test_vectors_more_than_256_images_in_one_call(gpu_ctx, B):
    """B = 255, 256, 257 and 513 images of 0 to 3 ids: the running total of bow_offsets_kernel across its tiles of 256 images
    (B > 256), empty images on the tile positions 255, 256 and 511."""
    o = vectors_case(gpu_ctx, C.vector_many_case(B))[0]
    assert len(o) == B + 1


def test_vectors_ids_outside_the_table_weigh_nothing(gpu_ctx):
    """-1, n_words and 2^31 - 1 among good ids: they leave the list, the rest is as if they had not been there."""
    words, off, idf, n_words = C.vector_outside_case()
    got = vectors_case(gpu_ctx, (words, off, idf, n_words))
    assert got[1].min() >= 0 and got[1].max() < n_words and got[0][2] == got[0][1]
    keep = (words >= 0) & (words < n_words)
    off2 = np.concatenate([[0], np.cumsum(keep)[off[1:] - 1]]).astype(np.int64)
    assert_vectors(device_vectors(gpu_ctx, words[keep], off2, idf, n_words), got)


# -------------------------------------------------------------------------------------------------------- 3: index and query
@pytest.mark.parametrize("n_keys", C.GROUP_KEYS)
def test_group_keys_past_4096_keys(gpu_ctx, n_keys):
    """slam_bow_group_keys against numpy at n_keys = 1, 4095, 4096, 4097 and 3 * 4096 + 5 (the running total of
    bow_scan_kernel across its tiles of 4096 keys) and n = 0, 1, 20000, with keys -1 and n_keys among the good ones."""
    from slamhip._lib import check

    for n in C.GROUP_ROWS:
        keys = C.group_keys_case(n_keys, n)
        r_off, r_order = C.group_reference(keys, n_keys)
        m = buffers(gpu_ctx)
        try:
            d_keys, d_off, d_cur = m.up(keys), m.up(np.full(n_keys + 1, -5, np.int32)), m.up(np.full(n_keys, -5, np.int32))
            d_perm = m.up(np.full(n + 2, -1, np.int32))
            check(gpu_ctx.lib.slam_bow_group_keys(gpu_ctx.handle, d_keys.ptr, n, n_keys, d_off.ptr, d_cur.ptr, d_perm.ptr))
            off, perm = d_off.download(np.int32, (n_keys + 1,)), d_perm.download(np.int32, (n + 2,))
        finally:
            m.free()
        assert np.array_equal(off, r_off), (n_keys, n)                           # the exclusive scan, the total in the last slot
        total = int(r_off[-1])
        assert (perm[total:] == -1).all(), (n_keys, n)
        # inside a key the order is unspecified: sorted by (key, row) the permutation is numpy's stable grouping
        got = perm[:total]
        assert total == 0 or (got.min() >= 0 and got.max() < n)
        assert np.array_equal(got[np.lexsort((got, keys[got]))] if total else got, r_order), (n_keys, n)
        assert np.array_equal(keys[got], np.repeat(np.arange(n_keys), np.diff(r_off))), (n_keys, n)
        left_out = np.flatnonzero((keys < 0) | (keys >= n_keys))
        assert not np.isin(left_out, got).any()


def test_database_over_4913_words(bow, gpu_ctx, big_vocab):
    """An index build of more than 4096 keys: 200 entries of 3 to 40 words on both sides of word 4096, words 4095 and 4096
    themselves in most of them; the dense scores and the queries at R = 1, 10, 64."""
    nw = big_vocab.n_words
    entries, queries = C.crafted_entries(nw, 200, 33), C.crafted_entries(nw, 24, 34)
    s_ref, c_ref = R.dense(entries, queries)
    assert (c_ref > 0).sum() > 2000 and ((c_ref > 0).sum(1) > 64).all()
    db = bow.BowDatabase(big_vocab, gpu_ctx)
    assert list(db.add_vectors(as_vectors(bow, entries))) == list(range(200))
    q = as_vectors(bow, queries)
    s, c = db.scores_dense(q)
    assert np.array_equal(s, s_ref) and np.array_equal(c, c_ref)
    assert_queries(db, q, s_ref, c_ref, (1, 10, 64), (None, 100))
    db.free()


def test_query_hits_of_score_zero_and_of_score_one(bow, gpu_ctx, big_vocab):
    """The two ends of the packed key (s_int + 1) << 32 | ~id.  s_int = 0 with common >= 1: entries that share a word with the
    query only where the stored q or the query's q is 0; they come after every positive score, by ascending id, with score 0.0,
    and are no fillers.  s_int = 2^31: entries identical to a one-word query score exactly 1.0, two of them tie, the lower id
    first."""
    entries, queries = C.score_ends_case()
    s_ref, c_ref = R.dense(entries, queries)
    db = bow.BowDatabase(big_vocab, gpu_ctx)
    db.add_vectors(as_vectors(bow, entries))
    q = as_vectors(bow, queries)
    s, c = db.scores_dense(q)
    assert np.array_equal(s, s_ref) and np.array_equal(c, c_ref)
    ids, sc, cm = db.query(q, 10)                                                # R larger than the 7 and the 4 hits
    assert ids[0].tolist() == [0, 9, 4, 6, 1, 2, 7, -1, -1, -1] and cm[0].tolist() == [3, 1, 1, 1, 1, 1, 2, 0, 0, 0]
    assert sc[0].tolist() == [0.5, 0.25, 0.125, 100 / 2.0 ** 31, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert ids[1].tolist() == [3, 5, 4, 6] + [-1] * 6 and sc[1, :4].tolist() == [1.0, 1.0, 2.0 ** -11, 0.0] and cm[1, :4].tolist() == [1] * 4
    ids, sc, cm = db.query(q, 7)                                                 # R equal to the hits of query 0
    assert ids[0].tolist() == [0, 9, 4, 6, 1, 2, 7] and ids[1].tolist() == [3, 5, 4, 6, -1, -1, -1]
    ids, sc, cm = db.query(q, 5)                                                 # R inside the zero scores
    assert ids[0].tolist() == [0, 9, 4, 6, 1] and sc[0, 4] == 0.0 and cm[0, 4] == 1
    assert db.query(q, 4)[0][1].tolist() == [3, 5, 4, 6]                         # R equal to the hits of query 1
    assert db.query(q, 1)[0][:, 0].tolist() == [0, 3]
    assert_queries(db, q, s_ref, c_ref, (1, 3, 4, 5, 7, 10, 64), (None, 5, 2))
    db.free()


def test_database_empty_entries_keep_their_ids(bow, gpu_ctx, big_vocab):
    """Vectors with no words at the first id, between real ones and at the last id: len counts them, the others keep their ids,
    no result names them, max_id at an empty id and just past one."""
    real = C.crafted_entries(big_vocab.n_words, 3, 35)
    entries = [EMPTY, real[0], EMPTY, real[1], real[2], EMPTY]
    queries = real + C.crafted_entries(big_vocab.n_words, 4, 36) + [EMPTY]
    s_ref, c_ref = R.dense(entries, queries)
    assert not c_ref[:, [0, 2, 5]].any() and (c_ref[[0, 1, 2], [1, 3, 4]] > 0).all()
    db = bow.BowDatabase(big_vocab, gpu_ctx)
    assert list(db.add_vectors(as_vectors(bow, entries[:3]))) == [0, 1, 2] and db.add(as_vectors(bow, [entries[3]])) == 3
    assert list(db.add_vectors(as_vectors(bow, entries[4:]))) == [4, 5] and len(db) == 6
    q = as_vectors(bow, queries)
    s, c = db.scores_dense(q)
    assert s.shape == (8, 6) and np.array_equal(s, s_ref) and np.array_equal(c, c_ref)
    ids, sc, _ = db.query(q, 6)
    assert ids[0, 0] == 1 and ids[1, 0] == 3 and ids[2, 0] == 4 and sc[0, 0] > 0.999
    assert not np.isin(ids, [0, 2, 5]).any() and (ids[7] == -1).all()
    assert_queries(db, q, s_ref, c_ref, (1, 6, 64), (None, 0, 1, 2, 3, 5, 6))
    assert db.query(q, 6, 2)[0][0].tolist() == [1, -1, -1, -1, -1, -1] == db.query(q, 6, 3)[0][0].tolist()
    db.free()


def test_database_store_grows_by_more_than_one_doubling(bow, gpu_ctx, big_vocab):
    """capacity = 16, then one add_vectors call of some 600 words (16 -> 1024 slots), queries before and after it: the results
    are those of a database built in one go."""
    entries = C.crafted_entries(big_vocab.n_words, 40, 37)
    small = sorted(range(40), key=lambda e: len(entries[e][0]))[:2]
    entries = [entries[e] for e in small] + [entries[e] for e in range(40) if e not in small]
    assert sum(len(e[0]) for e in entries[:2]) <= 16 and sum(len(e[0]) for e in entries) > 4 * 16
    q = as_vectors(bow, C.crafted_entries(big_vocab.n_words, 12, 38))
    s_ref, c_ref = R.dense(entries, rows_of((q.offsets, q.words, q.values, q.q)))
    db = bow.BowDatabase(big_vocab, gpu_ctx, capacity=16)
    db.add_vectors(as_vectors(bow, entries[:2]))
    assert db._cap == 16
    assert_queries(db, q, s_ref[:, :2], c_ref[:, :2], (1, 10))
    assert list(db.add_vectors(as_vectors(bow, entries[2:]))) == list(range(2, 40)) and db._cap >= 4 * 16
    once = bow.BowDatabase(big_vocab, gpu_ctx)
    once.add_vectors(as_vectors(bow, entries))
    for a, b in zip(db.scores_dense(q) + db.query(q, 10) + db.query(q, 64, 17), once.scores_dense(q) + once.query(q, 10) + once.query(q, 64, 17)):
        assert a.tobytes() == b.tobytes()
    assert np.array_equal(db.scores_dense(q)[0], s_ref)
    assert_queries(db, q, s_ref, c_ref, (1, 10, 64))
    db.free()
    once.free()


# ---------------------------------------------------------------------------------------------------------------- 4: training
@pytest.mark.parametrize("name", sorted(C.TRAIN))
def test_training_past_256_frontier_nodes_and_4096_keys(bow, gpu_ctx, name):
    """a: a frontier of 289 nodes (a second workgroup of the seeding kernels) and more than 4096 words (the per-word image
    count crosses a scan tile).  b: frontiers of 256 and then 1022 nodes, ragged.  deep: a with one more depth,
    so that the grouping of the rows by node has 4766 keys, more than a scan tile.  Every array equals the reference's."""
    d, off, k, depth = C.train_case(name)
    ref = R.train(d, off, k, depth)
    assert max(C.level_sizes(ref)[:depth]) > C.OFFSET_TILE
    v = bow.train_vocabulary(d, off, k, depth, ctx=gpu_ctx)
    same_vocab(v, ref)
    v.free()


def test_training_exact_half_majority(bow, gpu_ctx):
    """2 * count >= rows on the device: centre 1 holds a row of ones and a row of ones with 100 bits cleared, so the cleared
    bits are set in exactly half of its rows and the child is all ones."""
    d, off, k, depth = C.half_case()
    v = bow.train_vocabulary(d, off, k, depth, ctx=gpu_ctx)
    assert v.node_desc[1].tolist() == [0] * 32 and v.node_desc[2].tolist() == [255] * 32
    assert v.child_begin.tolist() == [1, 0, 0] and v.child_count.tolist() == [2, 0, 0] and v.word_of_node.tolist() == [-1, 0, 1]
    same_vocab(v, R.train(d, off, k, depth))
    w, _ = bow.bow_transform(v, d, ctx=gpu_ctx)
    assert w.tolist() == [0, 0, 1, 1]
    v.free()


def test_training_word_in_every_image_vanishes_from_the_vectors(bow, gpu_ctx):
    """A word that occurs in every image has idf ln(1) = 0 and leaves bow_vectors."""
    d, off, k, depth = C.everywhere_case()
    v = bow.train_vocabulary(d, off, k, depth, ctx=gpu_ctx)
    same_vocab(v, R.train(d, off, k, depth))
    assert v.idf.tolist() == [0.0, np.log(2.0)]
    got = bow.bow_vectors(v, d, off, ctx=gpu_ctx)
    assert got.offsets.tolist() == [0, 1, 1] and got.words.tolist() == [1] and got.values.tolist() == [1.0] and got.q.tolist() == [1 << 31]
    v.free()
