"""The numpy statement of the bag-of-words specification (tests/bow_ref.py) against answers derived by hand,
and the host side of slamhip.bow (validation, the text form).  No GPU."""
import os

import numpy as np
import pytest

import bow_ref as R
from hamming_families import prefix_rows
from slamhip import bow

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def prefix_tree():
    """k = 3, depth = 2 over prefix rows (every distance is |a - b|): the root's children 40 / 120 / 200; 40 has the two
    children 20 / 60 (ragged), 120 is a leaf above the depth, 200 has 180 / 200 / 240.  Word ids are a table."""
    a = [0, 40, 120, 200, 20, 60, 180, 200, 240]
    return {"k": 3, "depth": 2, "node_desc": prefix_rows(a), "child_begin": np.array([1, 4, 0, 6, 0, 0, 0, 0, 0], np.int32),
            "child_count": np.array([3, 2, 0, 3, 0, 0, 0, 0, 0], np.int32),
            "word_of_node": np.array([-1, -1, 3, -1, 0, 1, 2, 5, 4], np.int32), "idf": np.array([1.0, 2.0, 0.5, 0.25, 3.0, 1.5])}


PREFIX_QUERIES = [80, 160, 250, 190, 40]      # midway 40|120; midway 120|200 (a leaf at depth 1); plain; tie 180|200; a centre
PREFIX_WORDS = [1, 3, 4, 2, 0]
PREFIX_NODES = {0: [5, 2, 8, 6, 4], 1: [1, 2, 3, 3, 1], 2: [0] * 5, 5: [0] * 5}


def test_descent_on_prefix_tree():
    v = prefix_tree()
    for up, nodes in PREFIX_NODES.items():
        w, n = R.transform(v, prefix_rows(PREFIX_QUERIES), up)
        assert w.tolist() == PREFIX_WORDS and n.tolist() == nodes, up
    bow.Vocabulary.from_arrays(**v)


def test_vector_of_identical_descriptors_is_one_word():
    v = prefix_tree()
    w, val, q = R.vector([4] * 37, v["idf"])
    assert w.tolist() == [4] and val.tolist() == [1.0] and q.tolist() == [1 << 31]


def test_vector_of_zero_idf_words_is_empty():
    w, val, q = R.vector([0, 2, 2, 1], np.zeros(3))
    assert len(w) == len(val) == len(q) == 0
    assert all(len(x) == 0 for x in R.vector([], np.ones(3)))


def test_vector_weights_and_order():
    w, val, q = R.vector([5, 1, 5, 3, 5, 1], np.array([9.0, 0.5, 9.0, 0.0, 9.0, 0.25]))
    assert w.tolist() == [1, 5]                                  # word 3 has idf 0 and leaves
    assert val.tolist() == [1.0 / 1.75, 0.75 / 1.75]
    assert q.tolist() == [int(np.floor(v * 2.0 ** 31)) for v in val]
    with pytest.raises(ValueError):
        R.vector(np.zeros(8193, np.int64), np.ones(1))


def test_ordered_sum_is_the_stated_order():
    rng = np.random.default_rng(5)
    t = rng.uniform(0, 1, 200) * 10.0 ** rng.integers(-8, 8, 200)
    p = [0.0] * 64
    for j, x in enumerate(t):
        p[j % 64] = p[j % 64] + x
    s = p[0]
    for l in range(1, 64):
        s = s + p[l]
    assert R.ordered_sum(t) == s


def test_min_sum_scores_by_hand():
    assert R.score_int([1, 3, 5], [10, 20, 30], [3, 5, 7], [25, 5, 100]) == (25, 2)
    assert R.score_int([1, 2], [7, 7], [3, 4], [9, 9]) == (0, 0)
    assert R.score_int([], [], [3], [9]) == (0, 0)
    s = np.array([[5, 9, 9, 0, 7]], np.uint32)
    c = np.array([[1, 2, 1, 0, 3]], np.int32)
    ids, sc, cm = R.query(s, c, 4)
    assert ids.tolist() == [[1, 2, 4, 0]] and cm.tolist() == [[2, 1, 3, 1]]      # equal scores by ascending id; entry 3 shares nothing
    assert sc[0, 0] == 9 / 2.0 ** 31
    ids, sc, cm = R.query(s, c, 4, max_id=2)
    assert ids.tolist() == [[1, 0, -1, -1]] and sc[0, 2:].tolist() == [0.0, 0.0] and cm[0, 2:].tolist() == [0, 0]


def test_fixed_point_bound_against_f64_score():
    rng = np.random.default_rng(11)
    idf = rng.uniform(0.1, 8.0, 400)
    worst = 0.0
    for _ in range(60):
        a = R.vector(rng.integers(0, 400, rng.integers(1, 300)), idf)
        b = R.vector(rng.integers(0, 400, rng.integers(1, 300)), idf)
        s, common = R.score_int(a[0], a[2], b[0], b[2])
        err = R.score_l1(a[0], a[1], b[0], b[1]) - s / 2.0 ** 31
        assert -1e-12 <= err < common * 2.0 ** -31 + 1e-12
        worst = max(worst, err * 2.0 ** 31 / max(common, 1))
    assert worst < 1.0


def test_majority_at_an_exact_half():
    ones, zeros = np.full((1, 32), 255, np.uint8), np.zeros((1, 32), np.uint8)
    assert R.majority(np.r_[ones, zeros]).tolist() == [255] * 32              # 2 * 1 >= 2: set
    assert R.majority(np.r_[ones, zeros, zeros]).tolist() == [0] * 32           # 2 * 1 < 3
    assert R.majority(np.r_[ones, ones, zeros, zeros, prefix_rows([8])]).tolist() == [255] + [0] * 31   # 3 of 5, then 2 of 5


def test_maximin_stops_at_distance_zero():
    same = prefix_rows([7] * 5)
    cent, cc = R.seed_level(same, np.zeros(5, np.int64), 1, 4)
    assert cc.tolist() == [1]
    two = prefix_rows([7, 90, 7, 90, 90])
    cent, cc = R.seed_level(two, np.zeros(5, np.int64), 1, 4)
    assert cc.tolist() == [2] and np.array_equal(cent[0, :2], prefix_rows([7, 90]))
    # two nodes at once; ties on the distance go to the first row
    rows = prefix_rows([0, 100, 50, 200, 10, 10, 30])
    cent, cc = R.seed_level(rows, np.array([0, 0, 0, 0, 1, 1, 1]), 2, 3)
    assert cc.tolist() == [3, 2]
    assert np.array_equal(cent[0], prefix_rows([0, 200, 100])) and np.array_equal(cent[1, :2], prefix_rows([10, 30]))


def test_training_by_hand():
    v = R.train(prefix_rows([0, 0, 100, 100, 250]), [0, 2, 5], k=3, depth=1)
    assert np.array_equal(v["node_desc"][1:], prefix_rows([0, 250, 100]))       # centre order: first row, farthest, next farthest
    assert v["child_begin"].tolist() == [1, 0, 0, 0] and v["child_count"].tolist() == [3, 0, 0, 0]
    assert v["word_of_node"].tolist() == [-1, 0, 1, 2]
    assert v["idf"].tolist() == [np.log(2.0)] * 3
    one = R.train(prefix_rows([9]), [0, 1], k=4, depth=3)
    assert one["child_count"].tolist() == [0] and one["word_of_node"].tolist() == [0] and one["idf"].tolist() == [0.0]
    bow.Vocabulary.from_arrays(**v)
    bow.Vocabulary.from_arrays(**one)


def test_scene_of_64_places():
    base, off, qd, qoff = R.scene()
    v = R.train(base, off, 8, 3)
    assert len(v["node_desc"]) == 585 and len(v["idf"]) == 512 and (v["idf"] > 0).all()
    eo, ew, ev, eq = R.vectors(v, base, off)
    qo, qw, qv, qq = R.vectors(v, qd, qoff)
    rows = lambda o, w, x, q: [(w[o[i]:o[i + 1]], x[o[i]:o[i + 1]], q[o[i]:o[i + 1]]) for i in range(len(o) - 1)]
    s, c = R.dense(rows(eo, ew, ev, eq), rows(qo, qw, qv, qq))
    ids, sc, _ = R.query(s, c, 2)
    assert (ids[:, 0] == np.arange(64)).sum() == 64
    assert sc[:, 0].min() > sc[:, 1].max()


# ---- the host side of slamhip.bow -------------------------------------------------------------------------------------------

def test_text_form_golden_file():
    v = bow.read_dbow2_text(os.path.join(GOLDEN, "bow_vocab_small.txt"))
    # file ids 1 (inner), 2, 3 (its leaves), 4 (a leaf of the root) -> breadth first 1, 4, 2, 3; words by file order
    assert (v.k, v.depth) == (2, 2)
    assert v.child_begin.tolist() == [1, 3, 0, 0, 0] and v.child_count.tolist() == [2, 2, 0, 0, 0]
    assert v.word_of_node.tolist() == [-1, -1, 2, 0, 1] and v.idf.tolist() == [0.5, 1.25, 0.0]
    assert v.node_desc[:, 0].tolist() == [0, 10, 40, 20, 250] and v.node_desc[4, 6] == 0
    with pytest.raises(ValueError):
        bow.write_dbow2_text(v, os.devnull)                     # word ids do not ascend with the node id


def test_text_form_round_trip_and_npz(tmp_path):
    base, off, _, _ = R.scene(places=6, per_place=40)
    ref = R.train(base, off, 4, 3)
    v = bow.Vocabulary.from_arrays(**ref)
    bow.write_dbow2_text(v, tmp_path / "voc.txt")
    v.save(tmp_path / "voc.npz")
    for w in (bow.read_dbow2_text(tmp_path / "voc.txt"), bow.Vocabulary.load(tmp_path / "voc.npz")):
        for name in ("node_desc", "child_begin", "child_count", "word_of_node", "idf"):
            a, b = getattr(w, name), ref[name]
            assert a.dtype == b.dtype and np.array_equal(a, b), name
    (tmp_path / "bad.txt").write_text("4 3 1 0\n")
    with pytest.raises(NotImplementedError):
        bow.read_dbow2_text(tmp_path / "bad.txt")
    (tmp_path / "bad2.txt").write_text("4 3 0 2\n")
    with pytest.raises(NotImplementedError):
        bow.read_dbow2_text(tmp_path / "bad2.txt")


MALFORMED = {
    "k too small": dict(k=1),
    "depth too large": dict(depth=11),
    "tree deeper than depth": dict(depth=1),
    "row width": dict(node_desc=np.zeros((9, 31), np.uint8)),
    "row dtype": dict(node_desc=np.zeros((9, 32), np.int32)),
    "array length": dict(child_count=np.zeros(8, np.int32)),
    "more than k children": dict(child_count=np.array([4, 2, 0, 3, 0, 0, 0, 0, 0], np.int32)),
    "children overlap": dict(child_begin=np.array([1, 3, 0, 6, 0, 0, 0, 0, 0], np.int32)),
    "children out of range": dict(child_begin=np.array([1, 4, 0, 7, 0, 0, 0, 0, 0], np.int32)),
    "a gap between sibling groups": dict(child_count=np.array([3, 1, 0, 3, 0, 0, 0, 0, 0], np.int32)),
    "inner node with a word": dict(word_of_node=np.array([-1, 6, 3, -1, 0, 1, 2, 5, 4], np.int32)),
    "leaf without a word": dict(word_of_node=np.array([-1, -1, -1, -1, 0, 1, 2, 5, 4], np.int32)),
    "word twice": dict(word_of_node=np.array([-1, -1, 3, -1, 0, 1, 2, 4, 4], np.int32)),
    "idf length": dict(idf=np.ones(5)),
    "idf negative": dict(idf=np.array([1.0, 2.0, -0.5, 0.25, 3.0, 1.5])),
    "idf not finite": dict(idf=np.array([1.0, 2.0, np.inf, 0.25, 3.0, 1.5])),
    "idf dtype": dict(idf=np.ones(6, np.int64)),
    "a cycle beside the tree": dict(child_begin=np.array([1, 4, 0, 0, 0, 0, 6, 0, 0], np.int32),
                                    child_count=np.array([3, 2, 0, 0, 0, 0, 3, 0, 0], np.int32)),
}


@pytest.mark.parametrize("what", sorted(MALFORMED))
def test_from_arrays_rejects(what):
    args = prefix_tree()
    args.update(MALFORMED[what])
    with pytest.raises(ValueError):
        bow.Vocabulary.from_arrays(**args)


def test_argument_errors_before_the_library(monkeypatch):
    v = bow.Vocabulary.from_arrays(**prefix_tree())
    monkeypatch.setattr(bow, "default_context", lambda: pytest.fail("the library was reached"))
    with pytest.raises(ValueError):
        bow.bow_vectors(v, np.zeros((4, 31), np.uint8), [0, 4])
    with pytest.raises(ValueError):
        bow.bow_transform(v, np.zeros((4, 32), np.float32))
    with pytest.raises(ValueError):
        bow.bow_transform(v, np.zeros((4, 32), np.uint8), levels_up=-1)
    with pytest.raises(ValueError):
        bow.train_vocabulary(np.zeros((4, 32), np.uint8), [0, 3], k=3, depth=2)
    with pytest.raises(ValueError):
        bow.train_vocabulary(np.zeros((4, 32), np.uint8), [0, 4], k=33, depth=2)
    with pytest.raises(ValueError):
        bow.train_vocabulary(np.zeros((0, 32), np.uint8), [0], k=3, depth=2)
