"""CPU: the edge cases of tests/bow_cases.py on the numpy reference alone (tests/bow_ref.py).  For every case the
condition that makes it bite is asserted here, where no GPU is needed: which child groups lie on which side of row 1152, which
child a planted tie must go to, that the bait of the raw-entry tables lies outside the view and inside the allocation and
would change the answer, how long the runs and kept lists of the vector cases are and that a zero q occurs, how wide the
training frontiers get, that the hand-made centre sees an exact half.  tests/test_bow_edges_gpu.py then compares the device
with the reference on the same cases, bit for bit."""
import os

import numpy as np
import pytest

import bow_cases as C
import bow_ref as R
from hamming_families import prefix_rows
from slamhip import bow
from test_bow_cpu import PREFIX_QUERIES, prefix_tree

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---------------------------------------------------------------------------------------------------------------- 1: transform
def test_staged_trees_put_their_groups_on_the_stated_side_of_row_1152():
    a, b = C.staged_tree("ends on the line"), C.staged_tree("straddles the line")
    for t in (a, b):
        bow.Vocabulary.from_arrays(**t)
        assert len(t["node_desc"]) == 1200 and C.level_sizes(t) == [1, 10, 100, 1000, 89]
        assert (t["child_count"][C.STAGED_FIRST_LEAF:] == 0).all() and (t["child_count"][:C.STAGED_FIRST_LEAF] > 0).all()
    ga, gb = C.staged_groups(a), C.staged_groups(b)
    assert ga[3][1:] == (1141, 10) and ga[4][1:] == (1151, 1) and ga[5][1:] == (1152, 10)
    assert ga[4][1] + ga[4][2] == C.STAGE                                        # ends exactly on the line: still from LDS
    assert ga[5][1] == C.STAGE                                                   # the first group read from memory
    assert gb[4][1:] == (1151, 5) and gb[4][1] < C.STAGE < gb[4][1] + gb[4][2]    # straddles: from memory
    assert gb[5][1:] == (1156, 10)
    assert [leaf for leaf, _ in C.staged_targets(a)] == list(range(1141, 1162))
    assert [leaf for leaf, _ in C.staged_targets(b)] == list(range(1141, 1166))


@pytest.mark.parametrize("which", sorted(C.STAGED_COUNTS))
def test_staged_plants_force_the_descent(which):
    tree = C.staged_tree(which)
    q = C.staged_queries(tree)
    n = len(tree["node_desc"])
    for i, (leaf, parent) in enumerate(C.staged_targets(tree)):
        planted = C.staged_plant(tree, leaf, parent, q[i])
        bow.Vocabulary.from_arrays(**planted)
        for up, node in ((0, leaf), (1, parent)):
            w, at = R.transform(planted, q, up)
            assert (int(w[i]), int(at[i])) == (n - 1 - leaf, node)                 # the closed form
            rw, rat = R.transform_raw(q, planted["node_desc"], np.stack([planted["child_begin"], planted["child_count"]], 1),
                                      planted["word_of_node"], n, 4, up)
            assert np.array_equal(w, rw) and np.array_equal(at, rat)


@pytest.mark.parametrize("k", C.TIE_KS)
def test_tie_cases_go_to_the_stated_child(k):
    cases = C.tie_cases(k)
    names = [c[0] for c in cases]
    assert len(names) == 3 + (k > 8) + 2 * (k > 16)
    for name, tree, q, win in cases:
        bow.Vocabulary.from_arrays(**tree)
        assert q.shape == (C.TIE_N, 32)
        w, at = R.transform(tree, q)
        assert np.array_equal(at, 1 + win) and np.array_equal(w, tree["word_of_node"][1 + win]), name
        d = R.hamming(q[:, None, :], tree["node_desc"][None, 1:])
        assert (d.min(1) == d[np.arange(len(q)), win]).all(), name               # the winner is a nearest child ...
        if "equal" in name and "last" not in name:
            assert ((d == d.min(1, keepdims=True)).sum(1) >= 2).all(), name      # ... and not the only one
        if "256" in name:
            assert (d == 256).all()
        if "c + 16" in name:
            assert set(win.tolist()) == set(range(k - 16)) and (d[np.arange(len(q)), win + 16] == d.min(1)).all()


def test_raw_case_layout_and_bait():
    c = C.raw_case()
    f, b, n = c["front"], c["back"], c["n_nodes"]
    assert (f, b, n) == (32, 64, 44) and len(c["rows_full"]) == len(c["child_full"]) == len(c["won_full"]) == f + n + b
    rows, child, won = C.raw_views(c)
    assert rows.base is c["rows_full"] and len(rows) == len(child) == len(won) == n
    spare = np.r_[0:f, f + n:f + n + b]                                          # outside the view, inside the allocation
    types = c["types"]
    assert all(any(np.array_equal(c["rows_full"][s], t) for t in types) for s in spare)     # every spare node row is bait
    assert (c["won_full"][spare] == C.RAW_WORD_OUTSIDE).all() and not c["child_full"][spare].any()
    assert (won != C.RAW_WORD_OUTSIDE).all()
    with pytest.raises(ValueError):
        bow.Vocabulary.from_arrays(3, c["depth"], rows, child[:, 0], child[:, 1], won, np.ones(1))
    # every range a kernel without clamps would read stays inside the allocation, and holds the bait of the query that gets there
    for v, ((begin, count), what) in C.RAW_MALFORMED.items():
        assert tuple(child[v]) == (begin, count)
        assert -f <= begin and begin + count <= n + b, what
        if v <= 5:
            outside = [r for r in range(begin, begin + count) if r < 0 or r >= n]
            assert outside and any(np.array_equal(c["rows_full"][f + r], types[v - 1]) for r in outside), what
    assert child[4][1] > 32 and n - child[4][0] > 32 and np.array_equal(rows[41], types[3])    # the cap of 32 binds by itself


@pytest.mark.parametrize("up", [0, 1])
def test_raw_case_answers_by_hand_and_without_clamps(up):
    c = C.raw_case()
    rows, child, won = C.raw_views(c)
    w, at = R.transform_raw(c["desc"], rows, child, won, c["n_nodes"], c["depth"], up)
    kind = c["kind"]
    assert (w != C.RAW_WORD_OUTSIDE).all() and (at >= 0).all() and (at < c["n_nodes"]).all()
    # type 0: node 1, whose clamped children are rows 0 .. 7, node 1 among them at distance 0: it stays there
    assert (w[kind == 0] == 1001).all() and (at[kind == 0] == 1).all()
    # types 1 and 2: child_begin at or above n_nodes is the last node alone
    assert (w[(kind == 1) | (kind == 2)] == 1043).all() and (at[(kind == 1) | (kind == 2)] == 43).all()
    # type 3: the copy at row 41 is the 34th child of node 4 and is not looked at
    assert (w[kind == 3] != 1041).all()
    # type 5: the cycle 0 -> 6 -> (0 | 1) -> ... ends after three steps
    assert np.isin(w[kind == 5], [1006, 1001, -1]).all()
    # type 6: the chain is cut at depth 3, at inner node 9, whose word is -1
    assert (w[kind == 6] == -1).all() and (at[kind == 6] == (9 if up == 0 else 8)).all()
    uw, uat, lo, hi = C.raw_unclamped(c, up)
    assert -c["front"] <= lo < 0 and c["n_nodes"] <= hi < c["n_nodes"] + c["back"]
    for t in range(5):                                                            # the five malformed ranges: the answer changes
        assert (uw[kind == t] != w[kind == t]).all(), C.RAW_MALFORMED[t + 1][1]
    assert (uw[kind == 3] == C.RAW_WORD_OUTSIDE).all() or (uw[kind == 3] == 1041).all()


def _valid_trees():
    base, off, _, _ = R.scene()
    small, soff, _, _ = R.scene(places=6, per_place=40)
    gold = bow.read_dbow2_text(os.path.join(GOLDEN, "bow_vocab_small.txt")).arrays()
    return [(prefix_tree(), prefix_rows(PREFIX_QUERIES + list(range(0, 256, 7)))), (R.train(base, off, 8, 3), base[::9]),
            (R.train(small, soff, 4, 3), small), (gold, C.random_rows(np.random.default_rng(1), 50)),
            (R.train(prefix_rows([0, 0, 100, 100, 250]), [0, 2, 5], k=3, depth=1), prefix_rows([0, 60, 100, 180, 250])),
            (R.train(prefix_rows([9]), [0, 1], k=4, depth=3), prefix_rows([9, 200]))]


def test_transform_raw_is_transform_on_valid_trees():
    for tree, desc in _valid_trees():
        child = np.stack([tree["child_begin"], tree["child_count"]], 1)
        for up in (0, 1, 2, 5):
            w, at = R.transform(tree, desc, up)
            rw, rat = R.transform_raw(desc, tree["node_desc"], child, tree["word_of_node"], len(tree["node_desc"]), tree["depth"], up)
            assert np.array_equal(w, rw) and np.array_equal(at, rat), (len(child), up)


# ----------------------------------------------------------------------------------------------------------------- 2: vectors
def _images(case):
    words, off = case[0], case[1]
    return [words[off[b]:off[b + 1]] for b in range(len(off) - 1)]


def _premise(q):
    """2^31 - K < sum(q) <= 2^31 for a vector of K > 0 words."""
    return len(q) == 0 or (1 << 31) - len(q) < int(q.astype(np.int64).sum()) <= (1 << 31)


def test_vector_sizes_case_has_the_stated_sizes():
    case = C.vector_sizes_case()
    sizes = np.diff(case[1]).tolist()
    assert sizes[1::2] == list(C.IMAGE_SIZES) and not any(sizes[0::2]) and len(sizes) == 25
    assert all(_premise(R.vector(w, case[2], case[3])[2]) for w in _images(case))


def test_vector_full_case_runs_kept_lists_and_a_zero_q():
    words, off, idf, n_words, names = C.vector_full_case()
    assert n_words == 10000 and np.diff(off).tolist() == [8192, 8192, 8192, 300, 6]
    img = _images((words, off))
    out = [R.vector(w, idf, n_words) for w in img]
    assert (np.diff(img[0]) == -1).all() and len(out[0][0]) == 8192               # U = K = 8192
    assert len(set(img[1].tolist())) == 1 and len(out[1][0]) == 1 and out[1][2].tolist() == [1 << 31]      # one run over every chunk
    u = np.unique(img[2])
    per = -(-len(u) // 256)
    chunks = [u[i:i + per] for i in range(0, len(u), per)]
    assert len(u) == 1808 and all(0 < (idf[ch] > 0).sum() < len(ch) for ch in chunks)       # kept != U in every thread's chunk
    assert len(out[2][0]) == 904
    assert len(img[3]) > 0 and len(out[3][0]) == 0 and len(out[2][0]) > 0 and len(out[4][0]) > 0          # K = 0 between two vectors
    w, v, q = out[4]
    assert w.tolist() == [C.FULL_TINY, 5, 7, 9] and q[0] == 0 and v[0] > 0 and v.max() / v.min() > 2.0 ** 31
    assert (out[2][2] == 0).any()                                                # the tiny word beside 1807 others
    assert all(_premise(o[2]) for o in out)


def test_vector_kept_case_lengths_and_an_order_that_shows():
    case = C.vector_kept_case()
    out = [R.vector(w, case[2], case[3]) for w in _images(case)]
    assert [len(o[0]) for o in out] == list(C.KEPT_LENGTHS)
    assert all(len(np.unique(w)) == K + 20 for w, K in zip(_images(case), C.KEPT_LENGTHS))
    differs = 0
    for w, o in zip(_images(case), out):
        ids, cnt = np.unique(w, return_counts=True)
        t = cnt * case[2][ids]
        t = t[t > 0]
        differs += float(np.sum(t[::-1])) != R.ordered_sum(t) or float(np.sum(t)) != R.ordered_sum(t)
    assert differs >= 2                                                          # another order of the sum gives other bits
    assert all(_premise(o[2]) for o in out)


@pytest.mark.parametrize("B", C.MANY_IMAGES)
def test_vector_many_case_has_empty_images_on_the_tile_positions(B):
    words, off, idf, n_words = C.vector_many_case(B)
    sizes = np.diff(off)
    assert len(sizes) == B and sizes.max() <= 3 and sizes[0] > 0 and sizes[254] > 0
    assert all(sizes[b] == 0 for b in (255, 256, 511) if b < B) and (sizes[-1] == 0) == (B in (256, 257))
    ro = R.vectors_of_words(words, off, idf, n_words)[0]
    assert ro[-1] > 0 and (B <= C.OFFSET_TILE or ro[C.OFFSET_TILE] > 0)          # the carry of the second tile is not zero


def test_vector_outside_case_drops_the_ids_outside_the_table():
    words, off, idf, n_words = C.vector_outside_case()
    assert {-1, n_words, (1 << 31) - 1} <= set(words.tolist()) and (idf > 0).all()
    # only ids the kernel's u32 comparison refuses before it reads idf
    assert ((words.astype(np.int64) & 0xFFFFFFFF >= n_words) == ((words < 0) | (words >= n_words))).all()
    out = [R.vector(w, idf, n_words) for w in _images((words, off))]
    assert [len(o[0]) for o in out][1] == 0 and out[3][0].tolist() == [0, n_words - 1]
    for w, o in zip(_images((words, off)), out):
        good = w[(w >= 0) & (w < n_words)]
        assert all(np.array_equal(a, b) for a, b in zip(o, R.vector(good, idf)))
    with pytest.raises(IndexError):
        R.vector(words, idf)                                                     # without n_words the reference would read outside


# -------------------------------------------------------------------------------------------------------- 3: index and query
@pytest.mark.parametrize("n_keys", C.GROUP_KEYS)
def test_group_keys_case_and_its_reference(n_keys):
    for n in C.GROUP_ROWS:
        keys = C.group_keys_case(n_keys, n)
        off, order = C.group_reference(keys, n_keys)
        assert len(keys) == n and off[0] == 0 and off[-1] == len(order) == ((keys >= 0) & (keys < n_keys)).sum()
        if n == 20000:
            assert (keys == -1).any() and (keys == n_keys).any() and off[-1] < n
            assert n_keys <= C.SCAN_TILE or off[C.SCAN_TILE] > 0                  # the carry into the second tile is not zero
        for k in {0, n_keys // 2, n_keys - 1}:
            assert np.array_equal(order[off[k]:off[k + 1]], np.flatnonzero(keys == k))


def test_crafted_entries_lie_on_both_sides_of_word_4096():
    tree = C.full_tree(17, 3)
    n_words = len(tree["idf"])
    bow.Vocabulary.from_arrays(**tree)
    assert n_words == 4913 > C.SCAN_TILE and n_words % C.SCAN_TILE
    entries = C.crafted_entries(n_words, 200, 33)
    assert all(3 <= len(e[0]) <= 40 and (np.diff(e[0]) > 0).all() and e[0].min() >= 0 and e[0].max() < n_words for e in entries)
    assert all(_premise(e[2]) for e in entries)
    has = lambda w: sum(w in e[0] for e in entries)
    assert has(C.SCAN_TILE - 1) >= 50 and has(C.SCAN_TILE) >= 50
    assert sum(e[0].min() < C.SCAN_TILE <= e[0].max() for e in entries) >= 150


def test_score_ends_case_by_hand():
    entries, queries = C.score_ends_case()
    s, c = R.dense(entries, queries)
    assert s[0].tolist() == [1 << 30, 0, 0, 0, 1 << 28, 0, 100, 0, 0, 1 << 29] and c[0].tolist() == [3, 1, 1, 0, 1, 0, 1, 2, 0, 1]
    assert s[1].tolist() == [0, 0, 0, 1 << 31, 1 << 20, 1 << 31, 0, 0, 0, 0] and c[1].tolist() == [0, 0, 0, 1, 1, 1, 1, 0, 0, 0]
    assert all(int(e[2].astype(np.int64).sum()) <= 1 << 31 and (np.diff(e[0]) > 0).all() for e in entries + queries)
    ids, sc, cm = R.query(s, c, 10)
    assert ids[0].tolist() == [0, 9, 4, 6, 1, 2, 7, -1, -1, -1] and sc[0, 4:].tolist() == [0.0] * 6 and cm[0, 4:7].tolist() == [1, 1, 2]
    assert ids[1].tolist() == [3, 5, 4, 6] + [-1] * 6 and sc[1, :4].tolist() == [1.0, 1.0, 2.0 ** -11, 0.0]


def test_big_database_queries_have_more_than_64_hits():
    s, c = R.dense(C.crafted_entries(4913, 200, 33), C.crafted_entries(4913, 24, 34))
    assert ((c > 0).sum(1) > 64).all() and (c > 0).sum() > 2000


# ---------------------------------------------------------------------------------------------------------------- 4: training
@pytest.fixture(scope="module")
def trained():
    return {name: R.train(*C.train_case(name)) for name in C.TRAIN}


def test_training_case_a_crosses_a_workgroup_and_a_scan_tile(trained):
    v = trained["a"]
    sizes = C.level_sizes(v)
    assert sizes[:3] == [1, 17, 289] and sizes[2] > C.OFFSET_TILE                 # 289 frontier nodes in the last round
    assert len(v["idf"]) > C.SCAN_TILE and len(v["idf"]) % C.SCAN_TILE            # the per-word image count crosses a tile
    assert sizes[2] * 17 > C.SCAN_TILE


def test_training_case_b_crosses_a_workgroup_twice_and_groups_rows_over_a_scan_tile(trained):
    v = trained["b"]
    sizes = C.level_sizes(v)
    assert sizes[:5] == [1, 4, 16, 64, 256] and len(sizes) == 7
    assert sizes[5] > 2 * C.OFFSET_TILE and sizes[6] > sizes[5]                   # frontiers of 256, then past two workgroups
    assert (v["child_count"][sum(sizes[:5]):sum(sizes[:6])] == 0).any()          # ragged: leaves above the depth


def test_training_case_deep_groups_its_rows_by_more_than_4096_nodes(trained):
    sizes = C.level_sizes(trained["deep"])
    assert sizes[:3] == [1, 17, 289] and sizes[3] == len(trained["a"]["idf"]) > C.SCAN_TILE     # the frontier of the fourth round
    assert len(sizes) == 5 and len(trained["deep"]["idf"]) > C.SCAN_TILE


def test_half_case_sees_an_exact_half_in_the_reference():
    d, off, k, depth = C.half_case()
    assert not d[:2].any() and (d[2] == 255).all() and np.unpackbits(d[3]).sum() == 156
    cent, cc = R.seed_level(d, np.zeros(4, np.int64), 1, k)
    assert cc.tolist() == [2] and not cent[0, 0].any() and (cent[0, 1] == 255).all()
    a = R.iterate_level(d, np.zeros(4, np.int64), cent, cc)
    assert a.tolist() == [0, 0, 1, 1]
    bits = np.unpackbits(d[2:], axis=1).sum(0)
    assert (bits == 1).sum() == 100 and (bits == 2).sum() == 156                  # 100 bits set in exactly half of the two rows
    assert (cent[0, 1] == 255).all() and (R.majority(d[2:]) == 255).all()        # 2 * 1 >= 2: set
    v = R.train(d, off, k, depth)
    assert np.array_equal(v["node_desc"][1:], np.stack([np.zeros(32, np.uint8), np.full(32, 255, np.uint8)]))
    assert v["idf"].tolist() == [np.log(2.0)] * 2


def test_everywhere_case_has_a_word_of_idf_zero():
    d, off, k, depth = C.everywhere_case()
    v = R.train(d, off, k, depth)
    assert v["word_of_node"].tolist() == [-1, 0, 1] and v["idf"].tolist() == [0.0, np.log(2.0)]
    ro, rw, rv, rq = R.vectors(v, d, off)
    assert ro.tolist() == [0, 1, 1] and rw.tolist() == [1] and rv.tolist() == [1.0] and rq.tolist() == [1 << 31]
