"""Bag-of-words place recognition restated in numpy: the word and direct-index node of a descriptor, the
tf-idf vector of an image, the fixed-point score and the query order of the database, and the hierarchical k-majority
training.  A helper module of tests/test_bow_cpu.py, tests/test_bow_gpu.py and the edge tests (tests/bow_cases.py), like
sim3_ref.py.

Everything is vectorised over whole levels of the tree: all descriptors take one step of the descent together, all nodes of
a depth are seeded and iterated together.  Nothing here follows one descriptor through a loop the way the kernels do."""
import numpy as np

MAX_IMAGE = 8192
MAX_RESULTS = 64
Q_ONE = 1 << 31
_POP = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1).astype(np.int64)


def hamming(a, b):
    """Distances of the rows of a to the rows of b (uint8 [..., 32], broadcast)."""
    return _POP[np.bitwise_xor(a, b)].sum(-1)


# ---- descent ----------------------------------------------------------------------------------------------------------------

def transform(vocab, desc, levels_up=0):
    """(words, nodes) int32 [n] of descriptors uint8 [n, 32]; ``vocab`` is a dict of the flat arrays plus k and depth."""
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    nd, cb, cn = vocab["node_desc"], vocab["child_begin"].astype(np.int64), vocab["child_count"].astype(np.int64)
    n = len(desc)
    cur = np.zeros(n, np.int64)
    node = np.zeros(n, np.int64)
    target = max(0, int(vocab["depth"]) - int(levels_up))
    for level in range(1, int(vocab["depth"]) + 1):
        moving = cn[cur] > 0
        if not moving.any():
            break
        best = np.full(n, 1 << 30, np.int64)
        arg = np.zeros(n, np.int64)
        for c in range(int(cn.max())):
            ok = moving & (c < cn[cur])
            child = np.where(ok, cb[cur] + c, 0)
            d = np.where(ok, hamming(desc, nd[child]), 1 << 30)
            better = d < best                                   # strict: a tie stays with the lower child
            best = np.where(better, d, best)
            arg = np.where(better, child, arg)
        cur = np.where(moving, arg, cur)
        if level <= target:
            node = cur.copy()
    assert (cn[cur] == 0).all(), "a descent ended above a leaf: the tree is deeper than its depth"
    return vocab["word_of_node"][cur].astype(np.int32), node.astype(np.int32)


def transform_raw(desc, rows, child, word_of_node, n_nodes, depth, levels_up=0):
    """What ``slam_bow_transform`` promises for any tables, malformed ones included: ``rows`` uint8 [n_nodes, 32],
    ``child`` int [n_nodes, 2] = (child_begin, child_count).  A descent stops at ``child_count <= 0``; otherwise the children are
    the rows ``first .. first + count`` with ``first = clamp(child_begin, 0, n_nodes - 1)`` and ``count = min(child_count, 32,
    n_nodes - first)``; it takes at most ``depth`` steps; the word is ``word_of_node[cur]``, whatever that holds.  Only the first
    ``n_nodes`` rows of the three tables are read.  On a valid tree this is ``transform``."""
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    n_nodes, depth = int(n_nodes), int(depth)
    nd = np.asarray(rows, np.uint8).reshape(-1, 32)[:n_nodes]
    ch = np.asarray(child, np.int64).reshape(-1, 2)[:n_nodes]
    won = np.asarray(word_of_node, np.int64).reshape(-1)[:n_nodes]
    n = len(desc)
    cur = np.zeros(n, np.int64)
    node = np.zeros(n, np.int64)
    target = max(0, depth - int(levels_up))
    for level in range(1, depth + 1):
        moving = ch[cur, 1] > 0
        first = np.clip(ch[cur, 0], 0, n_nodes - 1)
        count = np.where(moving, np.minimum(np.minimum(ch[cur, 1], 32), n_nodes - first), 0)
        best = np.full(n, 1 << 30, np.int64)
        arg = cur.copy()
        for c in range(int(count.max()) if n else 0):
            ok = c < count
            at = np.where(ok, first + c, 0)
            d = np.where(ok, hamming(desc, nd[at]), 1 << 30)
            better = d < best                                   # strict: a tie stays with the lower child
            best = np.where(better, d, best)
            arg = np.where(better, at, arg)
        cur = arg
        if level <= target:
            node = np.where(moving, cur, node)
    return won[cur].astype(np.int32), node.astype(np.int32)


# ---- vectors ----------------------------------------------------------------------------------------------------------------

def ordered_sum(t):
    """The sum of t in the order of the specification: 64 partial sums over j = l (mod 64), then left to right."""
    t = np.asarray(t, np.float64)
    pad = np.zeros((-len(t)) % 64)
    rows = np.concatenate([t, pad]).reshape(-1, 64)             # (x + 0.0 == x for the x >= 0 met here)
    p = np.zeros(64)
    for r in rows:
        p = p + r
    s = p[0]
    for l in range(1, 64):
        s = s + p[l]
    return s


def vector(words, idf, n_words=None):
    """(words int32, values f64, q uint32) of one image's word ids.  With ``n_words`` (what ``slam_bow_vectors`` is given) an id
    outside ``[0, n_words)`` weighs nothing and leaves the list like a word of idf 0; it still counts towards the 8192."""
    words = np.asarray(words, np.int64).reshape(-1)
    if len(words) > MAX_IMAGE:
        raise ValueError("more than 8192 descriptors in one image")
    if n_words is not None:
        words = words[(words >= 0) & (words < int(n_words))]
    w, cnt = np.unique(words, return_counts=True)
    t = cnt.astype(np.float64) * np.asarray(idf, np.float64)[w]
    keep = t > 0
    w, t = w[keep], t[keep]
    if len(w) == 0:
        return np.zeros(0, np.int32), np.zeros(0), np.zeros(0, np.uint32)
    v = t / ordered_sum(t)
    q = np.floor(v * float(Q_ONE)).astype(np.uint32)
    return w.astype(np.int32), v, q


def vectors(vocab, desc, offsets):
    """(offsets int64 [B+1], words, values, q) of a batch: image b owns rows [offsets[b], offsets[b+1])."""
    words, _ = transform(vocab, desc)
    return vectors_of_words(words, offsets, vocab["idf"])


def vectors_of_words(words, offsets, idf, n_words=None):
    """``vectors`` from the word ids themselves (what ``slam_bow_vectors`` takes): image b owns ids [offsets[b], offsets[b+1])."""
    out = [vector(words[offsets[b]:offsets[b + 1]], idf, n_words) for b in range(len(offsets) - 1)]
    off = np.zeros(len(out) + 1, np.int64)
    np.cumsum([len(o[0]) for o in out], out=off[1:])
    cat = lambda i, dt: np.concatenate([o[i] for o in out]).astype(dt) if out else np.zeros(0, dt)
    return off, cat(0, np.int32), cat(1, np.float64), cat(2, np.uint32)


# ---- scores -----------------------------------------------------------------------------------------------------------------

def score_int(wa, qa, wb, qb):
    """(s_int, common) of two vectors given as (sorted words, q)."""
    _, ia, ib = np.intersect1d(wa, wb, assume_unique=True, return_indices=True)
    return int(np.minimum(np.asarray(qa, np.int64)[ia], np.asarray(qb, np.int64)[ib]).sum()), len(ia)


def score_l1(wa, va, wb, vb):
    """DBoW2's L1 score in f64: 1 - 0.5 * |v - w|_1 over the union of the words."""
    words = np.union1d(wa, wb)
    a, b = np.zeros(len(words)), np.zeros(len(words))
    a[np.searchsorted(words, wa)] = va
    b[np.searchsorted(words, wb)] = vb
    return 1.0 - 0.5 * np.abs(a - b).sum()


def dense(entries, queries):
    """(s_int uint32 [Q, E], common int32 [Q, E]) of lists of (words, values, q) triples."""
    s = np.zeros((len(queries), len(entries)), np.uint32)
    c = np.zeros((len(queries), len(entries)), np.int32)
    for i, qv in enumerate(queries):
        for j, e in enumerate(entries):
            s[i, j], c[i, j] = score_int(qv[0], qv[2], e[0], e[2])
    return s, c


def dense_from_tables(entries, queries):
    """``dense`` for vectors given as full tables uint32 [E, n_words] / [Q, n_words] (0 = the word is absent)."""
    e, q = np.asarray(entries, np.int64), np.asarray(queries, np.int64)
    s = np.stack([np.minimum(e, row[None, :]).sum(1) for row in q])
    c = np.stack([((e > 0) & (row[None, :] > 0)).sum(1) for row in q])
    return s.astype(np.uint32), c.astype(np.int32)


def query(s_int, common, max_results=10, max_id=None):
    """(ids int32 [Q, R], scores f64 [Q, R], common int32 [Q, R]) from the dense tables: entries below max_id that share a
    word, by (score descending, id ascending); fillers (-1, 0.0, 0)."""
    Q, E = s_int.shape
    max_id = E if max_id is None else min(int(max_id), E)
    ids = np.full((Q, max_results), -1, np.int32)
    sc = np.zeros((Q, max_results))
    cm = np.zeros((Q, max_results), np.int32)
    for i in range(Q):
        cand = np.flatnonzero(common[i, :max_id] > 0)
        order = cand[np.lexsort((cand, -s_int[i, cand].astype(np.int64)))][:max_results]
        ids[i, :len(order)] = order
        sc[i, :len(order)] = s_int[i, order].astype(np.float64) / float(Q_ONE)
        cm[i, :len(order)] = common[i, order]
    return ids, sc, cm


# ---- training ---------------------------------------------------------------------------------------------------------------

def majority(rows):
    """The bitwise majority of uint8 [m, 32] rows: a bit is set iff 2 * count >= m (DBoW2's meanValue)."""
    bits = np.unpackbits(np.asarray(rows, np.uint8).reshape(-1, 32), axis=1).astype(np.int64)
    return np.packbits((2 * bits.sum(0) >= len(bits)).astype(np.uint8))


def _assign(desc, cent, cc, f):
    """Nearest centre (lowest index on ties) of row i among cent[f[i], :cc[f[i]]]."""
    best = np.full(len(desc), 1 << 30, np.int64)
    arg = np.zeros(len(desc), np.int64)
    for c in range(cent.shape[1]):
        d = np.where(c < cc[f], hamming(desc, cent[f, c]), 1 << 30)
        better = d < best
        best = np.where(better, d, best)
        arg = np.where(better, c, arg)
    return arg


def seed_level(desc, f, F, k):
    """Maximin seeding of F nodes at once: row i belongs to node f[i].  Returns (centres uint8 [F, k, 32], counts [F])."""
    n = len(desc)
    rows = np.arange(n, dtype=np.int64)
    first = np.full(F, n, np.int64)
    np.minimum.at(first, f, rows)
    cent = np.zeros((F, k, 32), np.uint8)
    cent[:, 0] = desc[first]
    cc = np.ones(F, np.int64)
    alive = np.ones(F, bool)
    mind = hamming(desc, cent[f, 0])
    for j in range(1, k):
        best = np.full(F, -1, np.int64)
        np.maximum.at(best, f, mind * n + (n - 1 - rows))      # largest distance, then the first row
        add = alive & (best // n > 0)
        pick = n - 1 - best % n
        cent[add, j] = desc[pick[add]]
        cc[add] = j + 1
        alive = add
        mind = np.where(add[f], np.minimum(mind, hamming(desc, cent[f, j])), mind)
    return cent, cc


def iterate_level(desc, f, cent, cc, max_iters=16):
    """k-majority on F nodes at once; returns the final assignment and leaves the centres updated in place."""
    F, k = cent.shape[:2]
    flat = cent.reshape(F * k, 32)
    prev = None
    for _ in range(max_iters):
        a = _assign(desc, cent, cc, f)
        if prev is not None and np.array_equal(a, prev):
            break
        prev = a
        g = f * k + a
        order = np.argsort(g, kind="stable")
        gs = g[order]
        starts = np.flatnonzero(np.r_[True, gs[1:] != gs[:-1]])
        bits = np.unpackbits(desc[order], axis=1).astype(np.int64)
        cnt = np.add.reduceat(bits, starts, axis=0)
        m = np.diff(np.r_[starts, len(gs)])
        flat[gs[starts]] = np.packbits((2 * cnt >= m[:, None]).astype(np.uint8), axis=1)
    return _assign(desc, cent, cc, f)


def train(desc, image_offsets, k=10, depth=6, max_iters=16):
    """The vocabulary of the specification as a dict of flat arrays (node ids breadth first, words = leaves in id order)."""
    desc = np.ascontiguousarray(np.asarray(desc, np.uint8).reshape(-1, 32))
    image_offsets = np.asarray(image_offsets, np.int64)
    n = len(desc)
    if n == 0:
        raise ValueError("no descriptors to train on")
    node_desc, child_begin, child_count = [np.zeros(32, np.uint8)], [0], [0]
    frontier = [0]                                              # node ids of the current depth, in id order
    f = np.zeros(n, np.int64)                                   # frontier index of every row still above a leaf, else -1
    for d in range(depth):
        live = np.flatnonzero(f >= 0)
        if len(live) == 0:
            break
        F = len(frontier)
        cent, cc = seed_level(desc[live], f[live], F, k)
        a = iterate_level(desc[live], f[live], cent, cc, max_iters)
        own = np.bincount(f[live] * k + a, minlength=F * k).reshape(F, k) > 0
        nxt, relabel = [], np.full((F, k), -1, np.int64)
        for i, node in enumerate(frontier):
            if cc[i] == 1:
                continue                                        # a single centre: the node is a leaf
            child_begin[node] = len(node_desc)
            for c in np.flatnonzero(own[i]):
                relabel[i, c] = len(nxt)
                nxt.append(len(node_desc))
                node_desc.append(cent[i, c].copy())
                child_begin.append(0)
                child_count.append(0)
            child_count[node] = len(node_desc) - child_begin[node]
        f[live] = relabel[f[live], a]
        frontier = nxt
    child_count = np.asarray(child_count, np.int32)
    word_of_node = np.full(len(node_desc), -1, np.int32)
    leaves = np.flatnonzero(child_count == 0)
    word_of_node[leaves] = np.arange(len(leaves), dtype=np.int32)
    vocab = {"k": int(k), "depth": int(depth), "node_desc": np.asarray(node_desc, np.uint8).reshape(-1, 32),
             "child_begin": np.asarray(child_begin, np.int32), "child_count": child_count, "word_of_node": word_of_node,
             "idf": np.zeros(len(leaves))}
    words, _ = transform(vocab, desc)
    n_img = len(image_offsets) - 1
    img = np.repeat(np.arange(n_img), np.diff(image_offsets))
    pairs = np.unique(words.astype(np.int64) * n_img + img)
    vocab["idf"] = np.log(float(n_img) / np.bincount(pairs // n_img, minlength=len(leaves)).astype(np.float64))
    return vocab


# ---- the 64-place scene of the specification --------------------------------------------------------------------------------

def scene(places=64, per_place=120, seed=228):
    """(descriptors [places * per_place, 32], offsets, query descriptors, query offsets): every query is its place with 20 %
    of the rows replaced by random rows and 10 random bits flipped in every other row."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (places * per_place, 32), dtype=np.uint8)
    off = np.arange(places + 1, dtype=np.int64) * per_place
    q = base.copy()
    for p in range(places):
        rows = q[off[p]:off[p + 1]]
        swap = rng.permutation(per_place)[:per_place // 5]
        mask = np.zeros(per_place, bool)
        mask[swap] = True
        rows[mask] = rng.integers(0, 256, (len(swap), 32), dtype=np.uint8)
        for r in np.flatnonzero(~mask):
            bits = rng.permutation(256)[:10]
            np.bitwise_xor.at(rows[r], bits >> 3, (128 >> (bits & 7)).astype(np.uint8))
    return base, off, q, off.copy()
