"""Case builders of the bag-of-words edge tests: trees whose child groups sit on either side of the row where
the one-lane transform stops serving children from LDS, one-level trees with planted ties, malformed tables inside a larger
allocation for the raw entry, word-id lists for the vectors kernel, keys for the counting sort, database entries around word
4096 and the training sets that cross a scan tile and a workgroup.  tests/test_bow_edges_cpu.py asserts on tests/bow_ref.py
alone that every case has the property it is here for; tests/test_bow_edges_gpu.py compares the device with the reference on
the same cases.  Builders only: nothing runs on import."""
import numpy as np

import bow_ref as R

STAGE = 1152                        # BOW_STAGE_NODES: a group of children is served from LDS iff first + count <= 1152
SCAN_TILE = 4096                    # keys per tile of bow_scan_kernel
OFFSET_TILE = 256                   # images per tile of bow_offsets_kernel (and rows / nodes per workgroup elsewhere)


def random_rows(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def flip_bits(rng, row, bits):
    """``row`` with ``bits`` distinct random bits flipped."""
    out = row.copy()
    at = rng.permutation(256)[:bits]
    np.bitwise_xor.at(out, at >> 3, (128 >> (at & 7)).astype(np.uint8))
    return out


def level_sizes(vocab):
    """Nodes per depth of a breadth-first tree: entry d is the frontier of training round d."""
    cb, cc = vocab["child_begin"], vocab["child_count"]
    sizes, lo, hi = [], 0, 1
    while hi > lo:
        sizes.append(hi - lo)
        inner = np.flatnonzero(cc[lo:hi] > 0) + lo
        lo, hi = hi, hi + int(cc[inner].sum())
        assert len(inner) == 0 or cb[inner[0]] == lo
    return sizes


# ---- 1a: the staging line of the one-lane transform --------------------------------------------------------------------------
# k = 10, depth 4: the root, 10, 100 and 1000 nodes fill rows 0 .. 1110; the ten nodes 111 .. 120 carry the depth-4 groups from row
# 1111 on, every other node of depth 3 is a leaf.  Four groups of ten end at row 1150; the fifth group starts at row 1151.
STAGED_COUNTS = {"ends on the line": [10, 10, 10, 10, 1, 10, 10, 10, 10, 8],        # rows 1151..1151, then 1152..1161
                 "straddles the line": [10, 10, 10, 10, 5, 10, 10, 10, 10, 4]}      # rows 1151..1155
STAGED_FIRST_LEAF = 121             # every node from 121 on is a leaf; word = n_nodes - 1 - node


def staged_tree(which, seed=1152):
    counts = STAGED_COUNTS[which]
    n = 1111 + sum(counts)
    begin, count = np.zeros(n, np.int32), np.zeros(n, np.int32)
    begin[0], count[0] = 1, 10
    for v in range(1, 11):
        begin[v], count[v] = 11 + 10 * (v - 1), 10
    for v in range(11, 111):
        begin[v], count[v] = 111 + 10 * (v - 11), 10
    at = 1111
    for g, c in enumerate(counts):
        begin[111 + g], count[111 + g] = at, c
        at += c
    rng = np.random.default_rng(seed)
    won = np.full(n, -1, np.int32)
    won[STAGED_FIRST_LEAF:] = n - 1 - np.arange(STAGED_FIRST_LEAF, n)
    return {"k": 10, "depth": 4, "node_desc": random_rows(rng, n), "child_begin": begin, "child_count": count, "word_of_node": won,
            "idf": rng.uniform(0.5, 9.0, n - STAGED_FIRST_LEAF)}


def staged_groups(tree):
    """(parent, first, count) of the depth-4 groups."""
    return [(v, int(tree["child_begin"][v]), int(tree["child_count"][v])) for v in range(111, 121)]


def staged_targets(tree):
    """(leaf, parent) of every leaf of the group that ends on row 1150, the group that starts at row 1151 and the group after."""
    out = []
    for parent, first, count in staged_groups(tree)[3:6]:
        out += [(first + c, parent) for c in range(count)]
    return out


def staged_queries(tree, seed=7):
    """One random query per target, then random rows up to 70."""
    return random_rows(np.random.default_rng(seed), 70)


def staged_plant(tree, leaf, parent, query):
    """The tree with ``query`` written into every centre of the path root -> 1 -> 11 -> parent -> leaf: distance 0 all the way."""
    out = dict(tree)
    out["node_desc"] = tree["node_desc"].copy()
    out["node_desc"][[1, 11, parent, leaf]] = query
    return out


# ---- 1b: ties and extremes on one-level trees ---------------------------------------------------------------------------------
TIE_KS = (8, 9, 16, 17, 31, 32)
TIE_N = 65                          # 4 descriptors per wave of the sixteen-lane kernel: the 17th wave holds one live group


def one_level_tree(children, rng):
    k = len(children)
    won = np.full(k + 1, -1, np.int32)
    won[1:] = rng.permutation(k).astype(np.int32)
    return {"k": k, "depth": 1, "node_desc": np.concatenate([np.zeros((1, 32), np.uint8), children]),
            "child_begin": np.array([1] + [0] * k, np.int32), "child_count": np.array([k] + [0] * k, np.int32), "word_of_node": won,
            "idf": np.ones(k)}


def tie_cases(k, seed=0):
    """[(name, tree, queries uint8 [65, 32], winners int [65])]: the child (0-based) every query must descend to."""
    rng = np.random.default_rng(1000 * k + seed)
    near = lambda row: np.stack([flip_bits(rng, row, 3) for _ in range(TIE_N)])
    out = []
    x = random_rows(rng, 1)
    same = one_level_tree(np.repeat(x, k, 0), rng)
    out.append(("all children equal", same, random_rows(rng, TIE_N), np.zeros(TIE_N, np.int64)))
    out.append(("distance 256 everywhere", same, np.repeat(~x, TIE_N, 0), np.zeros(TIE_N, np.int64)))
    ch = random_rows(rng, k)
    out.append(("only the last child equals the query", one_level_tree(ch, rng), np.repeat(ch[k - 1:], TIE_N, 0),
                np.full(TIE_N, k - 1, np.int64)))
    for lo in (7, 15):
        if k > lo + 1:
            ch = random_rows(rng, k)
            ch[lo + 1] = ch[lo]
            out.append((f"children {lo} and {lo + 1} equal and nearest", one_level_tree(ch, rng), near(ch[lo]), np.full(TIE_N, lo, np.int64)))
    if k > 16:
        ch = random_rows(rng, k)
        ch[16:] = ch[:k - 16]
        win = np.arange(TIE_N) % (k - 16)
        out.append(("children c and c + 16 equal", one_level_tree(ch, rng), np.stack([flip_bits(rng, ch[c], 3) for c in win]), win))
    return out


# ---- 1c: malformed tables for the raw entry, inside a larger allocation -------------------------------------------------------
RAW_FRONT, RAW_BACK, RAW_NODES, RAW_DEPTH = 32, 64, 44, 3
RAW_WORD_OUTSIDE = -999
# node: (child_begin, child_count), what is wrong with it
RAW_MALFORMED = {1: ((-8, 8), "a negative child_begin"),
                 2: ((44, 12), "child_begin = n_nodes"),
                 3: ((51, 12), "child_begin above n_nodes"),
                 4: ((8, 40), "child_count 40: the cap of 32 binds before n_nodes - first = 36 does"),
                 5: ((36, 16), "a child range that runs past n_nodes"),
                 6: ((0, 2), "a child range that points back at the root"),
                 7: ((8, 1), "the head of a chain 7 -> 8 -> 9 -> 10 under a depth of 3")}


def raw_case(seed=44):
    """Tables of 44 nodes that ``from_arrays`` refuses, each in the middle of an allocation with 32 spare rows in front and 64
    behind.  The root's children 1 .. 7 are the malformed nodes; query type i (0-based) is the centre of node i + 1, so it goes
    there at distance 0.  Every spare node row is a copy of a query type (spare row j in front holds type j % 7, spare row j
    behind holds type (j + 3) % 7, so rows 44 .. 47 hold types 3 .. 6), the spare child rows are leaves and the spare words are
    -999: a kernel that left out a clamp would find distance 0 in a spare row, inside the allocation, and answer differently.
    Row 41, past the 32nd child of node 4, is a copy of type 3 inside the view."""
    rng = np.random.default_rng(seed)
    n, total = RAW_NODES, RAW_FRONT + RAW_NODES + RAW_BACK
    rows = random_rows(rng, n)
    child = np.zeros((n, 2), np.int32)
    child[0] = (1, 7)
    for v, (c, _) in RAW_MALFORMED.items():
        child[v] = c
    child[8], child[9] = (9, 1), (10, 1)
    types = rows[1:8].copy()
    rows[41] = types[3]
    won = (1000 + np.arange(n)).astype(np.int32)
    won[[0, 8, 9]] = -1
    rows_full = np.zeros((total, 32), np.uint8)
    rows_full[:RAW_FRONT] = types[np.arange(RAW_FRONT) % 7]
    rows_full[RAW_FRONT:RAW_FRONT + n] = rows
    rows_full[RAW_FRONT + n:] = types[(np.arange(RAW_BACK) + 3) % 7]
    child_full = np.zeros((total, 2), np.int32)
    child_full[RAW_FRONT:RAW_FRONT + n] = child
    won_full = np.full(total, RAW_WORD_OUTSIDE, np.int32)
    won_full[RAW_FRONT:RAW_FRONT + n] = won
    kind = np.arange(65) % 8                                    # type 7: a random row
    desc = np.where((kind < 7)[:, None], types[np.minimum(kind, 6)], random_rows(rng, 65))
    return {"rows_full": rows_full, "child_full": child_full, "won_full": won_full, "front": RAW_FRONT, "back": RAW_BACK, "n_nodes": n,
            "depth": RAW_DEPTH, "desc": np.ascontiguousarray(desc), "kind": kind, "types": types}


def raw_views(case):
    f, n = case["front"], case["n_nodes"]
    return case["rows_full"][f:f + n], case["child_full"][f:f + n], case["won_full"][f:f + n]


def raw_unclamped(case, levels_up=0):
    """What a kernel without the three clamps (but with the depth bound and the stop at count <= 0) would answer, reading the
    allocation: (words, nodes, lowest row read, highest row read) with rows counted from the view's start."""
    f, depth = case["front"], case["depth"]
    rows, child, won = case["rows_full"], case["child_full"], case["won_full"]
    target = max(0, depth - levels_up)
    words, nodes, lo, hi = [], [], 0, 0
    for q in case["desc"]:
        cur = at = 0
        for level in range(1, depth + 1):
            first, count = (int(x) for x in child[f + cur])
            if count <= 0:
                break
            lo, hi = min(lo, first), max(hi, first + count - 1)
            d = R.hamming(q[None, :], rows[f + first:f + first + count])
            cur = first + int(np.argmin(d))
            if level <= target:
                at = cur
        words.append(int(won[f + cur]))
        nodes.append(at)
    return np.asarray(words, np.int32), np.asarray(nodes, np.int32), lo, hi


# ---- 2: word ids for the vectors kernel ----------------------------------------------------------------------------------------
def _offsets_of(sizes):
    off = np.zeros(len(sizes) + 1, np.int64)
    np.cumsum(sizes, out=off[1:])
    return off


def _idf(rng, n_words, zero_share=0.1):
    return rng.uniform(0.1, 9.0, n_words) * (rng.random(n_words) >= zero_share)


IMAGE_SIZES = (1, 2, 3, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097)


def vector_sizes_case(seed=21):
    """(words, offsets, idf, n_words): the sizes around the powers of two of the bitonic padding and around the 256-thread
    partition, an empty image before, between and after them."""
    rng = np.random.default_rng(seed)
    sizes = [0]
    for s in IMAGE_SIZES:
        sizes += [s, 0]
    n_words = 3000
    return rng.integers(0, n_words, sum(sizes)).astype(np.int32), _offsets_of(sizes), _idf(rng, n_words), n_words


FULL_WORDS = 10000
FULL_ZERO_BELOW = 1808              # the even ids below 1808 have idf 0; every id from 1808 on has idf > 0
FULL_TINY = 1                       # idf 1e-10: beside a weight of a few units its q is floor(~1e-11 * 2^31) = 0


def vector_full_case(seed=22):
    """(words, offsets, idf, n_words, names): images at the limit of 8192 ids over 10 000 words."""
    rng = np.random.default_rng(seed)
    idf = rng.uniform(0.5, 9.0, FULL_WORDS)
    idf[0:FULL_ZERO_BELOW:2] = 0.0
    idf[FULL_TINY] = 1e-10
    zero_ids = np.arange(0, FULL_ZERO_BELOW, 2)
    images = [("8192 distinct ids, descending", np.arange(FULL_WORDS - 1, FULL_WORDS - 1 - 8192, -1)),
              ("8192 copies of one id", np.full(8192, 4321)),
              ("idf 0 and idf > 0 alternate", rng.permutation(np.concatenate([np.arange(FULL_ZERO_BELOW)] * 5)[:8192])),
              ("every word has idf 0", rng.choice(zero_ids, 300)),
              ("weights more than 2^31 apart", np.array([5, 5, FULL_TINY, 5, 7, 9]))]
    words = np.concatenate([w for _, w in images]).astype(np.int32)
    return words, _offsets_of([len(w) for _, w in images]), idf, FULL_WORDS, [name for name, _ in images]


KEPT_LENGTHS = (1, 63, 64, 65, 128, 129)


def vector_kept_case(seed=23):
    """(words, offsets, idf, n_words): image i keeps exactly KEPT_LENGTHS[i] words (and holds 20 words of idf 0 that leave);
    the idf values are not dyadic and the counts differ, so the order of the sum shows in the last bit."""
    rng = np.random.default_rng(seed)
    n_words = 400
    idf = rng.uniform(0.1, 8.0, n_words)
    idf[::5] = 0.0
    good, zero = np.flatnonzero(idf > 0), np.flatnonzero(idf == 0)
    images = []
    for K in KEPT_LENGTHS:
        ids = np.concatenate([rng.choice(good, K, replace=False), rng.choice(zero, 20, replace=False)])
        images.append(rng.permutation(np.repeat(ids, rng.integers(1, 5, len(ids)))))
    return np.concatenate(images).astype(np.int32), _offsets_of([len(w) for w in images]), idf, n_words


MANY_IMAGES = (255, 256, 257, 513)


def vector_many_case(B, seed=24):
    """(words, offsets, idf, n_words): B images of 0 to 3 ids; the images 255, 256 and 511 (where they exist) are empty, so
    at B = 256 and 257 the last image is."""
    rng = np.random.default_rng(seed + B)
    sizes = rng.integers(0, 4, B)
    sizes[[0, 254]] = 2                                         # the first image and the one before the empty ones are not empty
    for b in (255, 256, 511):
        if b < B:
            sizes[b] = 0
    n_words = 50
    return rng.integers(0, n_words, int(sizes.sum())).astype(np.int32), _offsets_of(sizes), _idf(rng, n_words, 0.2), n_words


def vector_outside_case(seed=25):
    """(words, offsets, idf, n_words): ids -1, n_words and 2^31 - 1 among good ids, and an image of nothing else."""
    rng = np.random.default_rng(seed)
    n_words = 100
    bad = np.array([-1, n_words, (1 << 31) - 1], np.int64)
    images = [rng.permutation(np.concatenate([rng.integers(0, n_words, 40), np.repeat(bad, 3)])),
              np.repeat(bad, 2),
              rng.permutation(np.concatenate([rng.integers(0, n_words, 300), np.repeat(bad, 30)])),
              np.array([n_words - 1, n_words, 0, -1])]
    idf = rng.uniform(0.1, 9.0, n_words)
    return np.concatenate(images).astype(np.int32), _offsets_of([len(w) for w in images]), idf, n_words


# ---- 3: the counting sort, the database ----------------------------------------------------------------------------------------
GROUP_KEYS = (1, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 3 * SCAN_TILE + 5)
GROUP_ROWS = (0, 1, 20000)


def group_keys_case(n_keys, n, seed=31):
    """int32 [n]: keys in [0, n_keys) with -1 and n_keys (left out by the sort) among them."""
    rng = np.random.default_rng(seed + 7 * n_keys + n)
    keys = rng.integers(0, n_keys, n).astype(np.int32)
    if n > 1:
        out = rng.random(n) < 0.05
        keys[out] = np.where(rng.random(int(out.sum())) < 0.5, -1, n_keys)
        keys[[0, n - 1]] = [n_keys - 1, 0]                      # the last key and the first are used
    return keys


def group_reference(keys, n_keys):
    """(key_off int32 [n_keys + 1], rows of every key as a list of sorted arrays) by numpy."""
    ok = (keys >= 0) & (keys < n_keys)
    hist = np.bincount(keys[ok], minlength=n_keys)
    off = np.zeros(n_keys + 1, np.int32)
    np.cumsum(hist, out=off[1:])
    order = np.flatnonzero(ok)[np.argsort(keys[ok], kind="stable")]
    return off, order


def full_tree(k, depth, seed=0):
    """The full k-ary tree of ``depth`` levels, breadth first, random centres, a shuffled word table."""
    rng = np.random.default_rng(seed)
    level = [k ** d for d in range(depth + 1)]
    n, inner = sum(level), sum(level[:-1])
    begin, count = np.zeros(n, np.int32), np.zeros(n, np.int32)
    begin[:inner] = 1 + k * np.arange(inner)
    count[:inner] = k
    won = np.full(n, -1, np.int32)
    won[inner:] = rng.permutation(n - inner).astype(np.int32)
    return {"k": k, "depth": depth, "node_desc": random_rows(rng, n), "child_begin": begin, "child_count": count, "word_of_node": won,
            "idf": rng.uniform(0.1, 9.0, n - inner)}


def crafted_vector(rng, words):
    """(words int32 ascending, values f64, q uint32) with random weights, normalised like a BoW vector."""
    words = np.unique(np.asarray(words, np.int64))
    t = rng.uniform(0.1, 9.0, len(words))
    v = t / R.ordered_sum(t)
    return words.astype(np.int32), v, np.floor(v * float(R.Q_ONE)).astype(np.uint32)


def crafted_entries(n_words, count, seed):
    """``count`` vectors of 3 to 40 words on both sides of word 4096: most words within 60 of it, a few anywhere, and words
    4095 / 4096 themselves in three entries out of four."""
    rng = np.random.default_rng(seed)
    out = []
    for e in range(count):
        m = int(rng.integers(3, 41))
        forced = [[SCAN_TILE - 1], [SCAN_TILE], [SCAN_TILE - 1, SCAN_TILE], [0, n_words - 1]][e % 4]
        pool = np.setdiff1d(np.concatenate([np.arange(SCAN_TILE - 60, SCAN_TILE + 60), rng.integers(0, n_words, 30)]), forced)
        out.append(crafted_vector(rng, np.concatenate([forced, rng.choice(pool, m - len(forced), replace=False)])))
    return out


def score_ends_case():
    """(entries, queries) for the two ends of the score.  s_int = 0 with common >= 1: entries 1, 2 and 7 share a word with query 0
    only where the stored q or the query's q is 0, entry 6 does so with query 1.  s_int = 2^31: entries 3 and 5 are the one-word
    query 1 itself."""
    u = lambda words, q: (np.asarray(words, np.int32), np.zeros(len(words)), np.asarray(q, np.uint32))
    entries = [u([10, 20, 30], [1 << 29, 1 << 29, 1 << 30]),         # 0: ordinary
               u([10, 500], [5000, 1 << 30]),                        # 1: shares word 10, where the query's q is 0
               u([40, 600], [0, (1 << 31) - 1]),                     # 2: shares word 40, where the stored q is 0
               u([77], [1 << 31]),                                   # 3: the one-word query itself
               u([20, 77, 900], [1 << 28, 1 << 20, 1 << 30]),        # 4: ordinary for both queries
               u([77], [1 << 31]),                                   # 5: the one-word query again
               u([30, 77], [100, 0]),                                # 6: score 100 for query 0; shares 77 with a stored q of 0
               u([10, 40], [7, 0]),                                  # 7: two shared words, both minima 0
               u([4000], [1 << 31]),                                 # 8: shares nothing
               u([30, 4096], [1 << 29, 1 << 29])]                    # 9: ordinary
    queries = [u([10, 20, 30, 40], [0, 1 << 30, 1 << 29, 1 << 29]), u([77], [1 << 31])]
    return entries, queries


# ---- 4: training ------------------------------------------------------------------------------------------------------------
TRAIN = {"a": dict(n=6000, off=[0, 2000, 4100, 6000], k=17, depth=3, seed=61),      # a frontier of 289, 4766 words
         "b": dict(n=3000, off=[0, 1000, 1900, 3000], k=4, depth=6, seed=62),       # frontiers of 256 and 1022
         "deep": dict(n=6000, off=[0, 2000, 4100, 6000], k=17, depth=4, seed=61)}   # a with one more round: its frontier is a's words


def train_case(name):
    c = TRAIN[name]
    return random_rows(np.random.default_rng(c["seed"]), c["n"]), np.asarray(c["off"], np.int64), c["k"], c["depth"]


def half_case():
    """k = 2, depth 1: two zero rows, a row of ones, a row of ones with 100 bits cleared.  Centre 1 ends with the last two
    rows: each cleared bit is set in exactly one of two rows."""
    rng = np.random.default_rng(63)
    ones = np.full(32, 255, np.uint8)
    dented = ones.copy()
    at = rng.permutation(256)[:100]
    np.bitwise_and.at(dented, at >> 3, (~(128 >> (at & 7))).astype(np.uint8))
    return np.stack([np.zeros(32, np.uint8), np.zeros(32, np.uint8), ones, dented]), np.array([0, 2, 4], np.int64), 2, 1


def everywhere_case():
    """k = 2, depth 1, two images: the zero row is in both (idf ln 1 = 0), the row of ones in the first only (idf ln 2)."""
    z, o = np.zeros(32, np.uint8), np.full(32, 255, np.uint8)
    return np.stack([z, o, z, z]), np.array([0, 2, 4], np.int64), 2, 1
