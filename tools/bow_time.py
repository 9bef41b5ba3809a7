"""Time of the bag-of-words calls (slam_bow_*).  Device calls are bracketed by HIP events (slam_timer_start/stop) around one
call on device-resident arrays, after a warm-up call; the median and the spread (min - max) over the rounds are reported.
Training and the host-side context lines are wall clock (they contain read-backs or run on the host) and say so.

    python tools/bow_time.py [--rounds R]

  * transform  slam_bow_transform of 1 x 2000 and 64 x 2000 descriptors through a full k = 10, L = 6 tree of random centres
               (1 111 111 nodes, 35.5 MB of rows), us per call and ns per descriptor, for both lane mappings (one lane per
               descriptor with the tree's top in LDS; sixteen lanes per descriptor, one child per lane), alternating;
  * vectors    slam_bow_vectors of the same batches (sort, runs, weights, norm, compaction);
  * index      slam_bow_index_build of 10^4 entries of 1500 words each (1.5 * 10^7 postings over 10^6 words);
  * query      slam_bow_query of Q = 1 and Q = 256 vectors of 1500 words against those entries, top 10, and dense for Q = 1;
  * training   train_vocabulary of 2^20 random descriptors in 1024 images at k = 10, L = 4 (wall clock, one core drives it);
  * context    tests/bow_ref.py (numpy, one host core) on the 1 x 2000 transform + vector, and KeyframeDatabase.query of 2000
               rows against 10^3 keyframes x 2000 rows: the brute-force path that ranks nothing (wall clock, with its copies).
Random descriptors are the worst case for the descent's locality and for the training's convergence.  The values are a
record, not a gate."""
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "slam-experiments_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import slamhip  # noqa: E402
from slamhip import bow  # noqa: E402


def opt(name, default):
    if name in sys.argv:
        i = sys.argv.index(name)
        v = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        return type(default)(v)
    return default


def spread(v):
    return f"{np.median(v) * 1e3:10.1f} us  [{min(v) * 1e3:9.1f} - {max(v) * 1e3:9.1f}]"


def full_tree(rng, k, depth):
    counts = k ** np.arange(depth + 1)
    n, inner = int(counts.sum()), int(counts[:-1].sum())
    begin, count = np.zeros(n, np.int32), np.zeros(n, np.int32)
    begin[:inner], count[:inner] = 1 + k * np.arange(inner), k
    won = np.full(n, -1, np.int32)
    won[inner:] = np.arange(n - inner)
    return bow.Vocabulary.from_arrays(k, depth, rng.integers(0, 256, (n, 32), dtype=np.uint8), begin, count, won,
                                      rng.uniform(0.5, 9.0, n - inner))


def main():
    rounds = opt("--rounds", 7)
    ctx = slamhip.default_context()
    lib, h = ctx.lib, ctx.handle
    rng = np.random.default_rng(1906)

    def timed(fn):
        ctx.timer_start()
        fn()
        return ctx.timer_stop()

    def run(call):
        timed(call)
        return [timed(call) for _ in range(rounds)]

    print(slamhip.load().slam_version().decode())
    vocab = full_tree(rng, 10, 6)
    dv = vocab.upload(ctx)
    desc = rng.integers(0, 256, (64 * 2000, 32), dtype=np.uint8)
    d_desc = ctx.upload(desc)
    for B in (1, 64):
        n = B * 2000
        dw, dn = ctx.malloc(4 * n), ctx.malloc(4 * n)

        both = {}
        for lanes in (1, 16, 1, 16):                      # the two lane mappings, alternating in one session
            def transform():
                assert lib.slam_bow_transform(h, d_desc.ptr, n, dv.node_desc.ptr, dv.child.ptr, dv.word_of_node.ptr, vocab.n_nodes, 6, 0, lanes, dw.ptr,
                                              dn.ptr) == 0

            both.setdefault(lanes, []).extend(run(transform))
            both.setdefault((lanes, "words"), dw.download(np.int32, (n,)))
        assert np.array_equal(both[(1, "words")], both[(16, "words")])
        for lanes in (1, 16):
            v = both[lanes]
            print(f"transform  {B:3d} x 2000, {lanes:2d} lane(s) per descriptor: {spread(v)}  {np.median(v) * 1e6 / n:8.2f} ns / descriptor")
        need = ctypes.c_uint64(0)
        assert lib.slam_bow_vectors_workspace(B, n, ctypes.byref(need)) == 0
        ws, off = ctx.malloc(need.value), ctx.upload(np.arange(B + 1, dtype=np.int64) * 2000)
        out = [ctx.malloc(8 * (B + 1)), ctx.malloc(4 * n), ctx.malloc(8 * n), ctx.malloc(4 * n)]

        def vectors():
            assert lib.slam_bow_vectors(h, dw.ptr, off.ptr, B, n, dv.idf.ptr, vocab.n_words, ws.ptr, ws.nbytes, *(o.ptr for o in out)) == 0

        v = run(vectors)
        kept = out[0].download(np.int64, (B + 1,))[-1]
        print(f"vectors    {B:3d} x 2000: {spread(v)}  {np.median(v) * 1e3 / B:8.2f} us / image, {kept / B:.0f} words / image")
        for o in [dw, dn, ws, off] + out:
            o.free()
    # where the two lane mappings cross (the rule of slam_bow_transform's lanes = 0: bow.limits()['lanes16_up_to'])
    dw, dn = ctx.malloc(4 * len(desc)), ctx.malloc(4 * len(desc))
    for n in (250, 1000, 4000, 16000, 64000):
        med = {}
        for lanes in (1, 16, 1, 16):
            def transform():
                assert lib.slam_bow_transform(h, d_desc.ptr, n, dv.node_desc.ptr, dv.child.ptr, dv.word_of_node.ptr, vocab.n_nodes, 6, 0, lanes, dw.ptr,
                                              dn.ptr) == 0

            med.setdefault(lanes, []).extend(run(transform))
        print(f"transform  n = {n:6d}: 1 lane {np.median(med[1]) * 1e3:8.1f} us, 16 lanes {np.median(med[16]) * 1e3:8.1f} us")
    dw.free()
    dn.free()
    t0 = time.perf_counter()
    import bow_ref
    ref = vocab.arrays()
    w, _ = bow_ref.transform(ref, desc[:2000])
    bow_ref.vector(w, ref["idf"])
    print(f"context    bow_ref transform + vector of 1 x 2000 on one host core: {(time.perf_counter() - t0) * 1e3:10.1f} ms wall clock")

    E, W = 10000, 1500
    words = (np.sort(rng.integers(0, vocab.n_words - W, (E, W)), axis=1) + np.arange(W)).astype(np.int32)
    q = rng.integers(1, (1 << 31) // W, (E, W)).astype(np.uint32)
    db = bow.BowDatabase(vocab, ctx, capacity=E * W)
    db.add_vectors(bow.BowVectors(np.arange(E + 1, dtype=np.int64) * W, words.reshape(-1), np.zeros(E * W), q.reshape(-1)))
    pw, pe, pq = db._parts(db._store, db._cap)
    off, post = ctx.malloc(4 * (vocab.n_words + 1)), ctx.malloc(8 * E * W)
    cursor, perm = ctx.malloc(4 * vocab.n_words), ctx.malloc(4 * E * W)

    def build():
        assert lib.slam_bow_index_build(h, pw.ptr, pe.ptr, pq.ptr, E * W, vocab.n_words, off.ptr, cursor.ptr, perm.ptr, post.ptr) == 0

    v = run(build)
    print(f"index      {E} entries x {W} words: {spread(v)}  {np.median(v) * 1e6 / (E * W):8.2f} ns / posting")
    for Q in (1, 256):
        pick = rng.integers(0, E, Q)
        qo, qw, qq = ctx.upload(np.arange(Q + 1, dtype=np.int64) * W), ctx.upload(words[pick]), ctx.upload(q[pick])
        di, ds, dc = ctx.malloc(40 * Q), ctx.malloc(40 * Q), ctx.malloc(40 * Q)

        def query():
            assert lib.slam_bow_query(h, qo.ptr, qw.ptr, qq.ptr, Q, off.ptr, post.ptr, vocab.n_words, E, E, 10, di.ptr, ds.ptr, dc.ptr, None, None) == 0

        v = run(query)
        ids = di.download(np.int32, (Q, 10))
        print(f"query      Q = {Q:3d}, top 10 of {E}: {spread(v)}  {np.median(v) * 1e3 / Q:8.2f} us / query, own entry first {np.mean(ids[:, 0] == pick):.3f}")
        if Q == 1:
            dds, ddc = ctx.malloc(4 * E), ctx.malloc(4 * E)

            def dense():
                assert lib.slam_bow_query(h, qo.ptr, qw.ptr, qq.ptr, Q, off.ptr, post.ptr, vocab.n_words, E, E, 1, None, None, None, dds.ptr, ddc.ptr) == 0

            print(f"query      Q = {Q:3d}, dense over {E}: {spread(run(dense))}")
            dds.free()
            ddc.free()
        for o in (qo, qw, qq, di, ds, dc):
            o.free()
    for o in (off, post, cursor, perm):
        o.free()
    db.free()
    vocab.free()
    d_desc.free()

    n = 1 << 20
    train = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    toff = np.arange(1025, dtype=np.int64) * 1024
    bow.train_vocabulary(train[:1 << 14], toff[:17], 10, 4, ctx=ctx).free()
    wall = []
    for _ in range(min(rounds, 3)):
        t0 = time.perf_counter()
        tv = bow.train_vocabulary(train, toff, 10, 4, ctx=ctx)
        wall.append(time.perf_counter() - t0)
    print(f"training   2^20 descriptors, k = 10, L = 4: {np.median(wall) * 1e3:10.1f} ms  [{min(wall) * 1e3:9.1f} - {max(wall) * 1e3:9.1f}]  wall clock with "
          f"upload and read-backs, {tv.n_nodes} nodes, {tv.n_words} words")

    kf = slamhip.KeyframeDatabase(ctx, capacity_rows=2000 * 1000)
    for i in range(1000):
        kf.add(train[(i * 1000) % (n - 2000):][:2000])
    kf.query(desc[:2000])
    wall = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        kf.query(desc[:2000])
        wall.append(time.perf_counter() - t0)
    print(f"context    KeyframeDatabase.query of 2000 rows against 10^3 keyframes x 2000 rows: {np.median(wall) * 1e3:10.1f} ms  "
          f"[{min(wall) * 1e3:9.1f} - {max(wall) * 1e3:9.1f}]  wall clock (per-feature neighbours, no ranking of places)")
    kf.free()


if __name__ == "__main__":
    main()
