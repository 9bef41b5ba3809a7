"""Time of the loop-candidate stage (slam_loop_*) at Q in {1, 256} queries x E in {10^4, 65 536} database
entries with nb = 10, in ONE session, on tables that are resident:

  * stage      slam_loop_candidates + slam_loop_fill on preallocated blocks, bracketed by HIP events (slam_timer_start/stop):
               the parameter copy, the kernels, the count read-back the first call ends with, the fill;
  * call       slamhip.loop_candidates_tables on the same resident tables and a resident BestTable, the same bracket around the
               whole Python call: its allocations, the upload of the lists, the downloads of the results, the frees; and once
               more with the best table as a host array, uploaded by the call;
  * query      BowDatabase.scores_dense_device for the same vectors, the same bracket: what feeds the stage;
  * host       slamhip.loop_candidates_host on the downloaded tables, wall clock on one host core;
  * parent     for Q = 1, slamhip.detect_loop_candidates - the dense download and the numpy filter that were all there was -
               wall clock, beside query + call, which is what replaces it.
One warm-up, then the median of 7 with the spread.  The database: places of 8 consecutive keyframes that share their 200 words
(of 10^4), so that a query meets a handful of candidates with full rows of neighbours; the graph joins keyframes up to 5 apart.
The values are a record, not a gate.  Needs the GPU; writes to stdout (kept as profiles/loop_detect_time.log)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-experiments_amd"))

import slamhip  # noqa: E402
from slamhip import bow, loop_detect as L  # noqa: E402
from slamhip._lib import addr  # noqa: E402

REPS, W, PLACE, NB = 7, 200, 8, 10


def spread(v, unit=1e3, name="us"):
    return f"{np.median(v) * unit:10.1f} {name}  [{min(v) * unit:9.1f} - {max(v) * unit:9.1f}]"


def full_tree(rng, k, depth):
    counts = k ** np.arange(depth + 1)
    n, inner = int(counts.sum()), int(counts[:-1].sum())
    begin, count = np.zeros(n, np.int32), np.zeros(n, np.int32)
    begin[:inner], count[:inner] = 1 + k * np.arange(inner), k
    won = np.full(n, -1, np.int32)
    won[inner:] = np.arange(n - inner)
    return bow.Vocabulary.from_arrays(k, depth, rng.integers(0, 256, (n, 32), dtype=np.uint8), begin, count, won, rng.uniform(0.5, 9.0, n - inner))


def database(ctx, vocab, rng, E):
    places = (np.sort(rng.integers(0, vocab.n_words - W, (E // PLACE + 1, W)), axis=1) + np.arange(W)).astype(np.int32)
    words = places[np.arange(E) // PLACE]
    q = rng.integers(1, (1 << 31) // W, (E, W)).astype(np.uint32)
    db = bow.BowDatabase(vocab, ctx, capacity=E * W)
    db.add_vectors(bow.BowVectors(np.arange(E + 1, dtype=np.int64) * W, words.reshape(-1), np.zeros(E * W), q.reshape(-1)))
    edges = np.concatenate([np.stack([np.arange(E - d), np.arange(d, E)], 1) for d in range(1, 6)])
    weights = np.concatenate([np.full(E - d, 60 - 10 * d) for d in range(1, 6)])
    return db, words, q, slamhip.CovisibilityGraph(E, edges, weights)


def main():
    ctx = slamhip.default_context()
    lib, h = ctx.lib, ctx.handle
    rng = np.random.default_rng(2210)
    print(slamhip.load().slam_version().decode())
    print(f"limits: {L.limits()}")

    def timed(fn):
        ctx.timer_start()
        fn()
        return ctx.timer_stop()

    def run(fn):
        timed(fn)
        return [timed(fn) for _ in range(REPS)]

    def wall(fn):
        fn()
        out = []
        for _ in range(REPS):
            t = time.perf_counter()
            fn()
            out.append((time.perf_counter() - t) * 1e3)
        return out

    vocab = full_tree(rng, 10, 4)
    for E in (10000, 65536):
        db, words, q, graph = database(ctx, vocab, rng, E)
        table = graph.best_table(NB)
        db.rebuild_index()
        for Q in (1, 256):
            pick = np.sort(rng.choice(np.arange(E // 2, E), Q, replace=False))
            vec = bow.BowVectors(np.arange(Q + 1, dtype=np.int64) * W, words[pick].reshape(-1), np.zeros(Q * W), q[pick].reshape(-1))
            connected = [graph.connected(int(k)) for k in pick]
            args = dict(connected=connected, own_ids=pick, limit=pick, nb=NB)
            print(f"== Q = {Q}, E = {E}, nb = {NB}: each query a keyframe of the second half that sees the entries before it ==")

            def query():
                d = db.scores_dense_device(vec)
                d[0].free()
                d[1].free()

            tq = run(query)
            d_s, d_c, _, _ = db.scores_dense_device(vec)
            s, c = d_s.download(np.uint32, (Q, E)), d_c.download(np.int32, (Q, E))
            want = L.loop_candidates_host(s, c, table, keep_stages=False, **args)
            got = L.loop_candidates_tables(d_s, d_c, table, shape=(Q, E), **args)
            equal = all(np.array_equal(getattr(got, k), getattr(want, k)) for k in ("offsets", "ids", "scores")) and got.skipped == want.skipped == 0
            resident = L.BestTable(table, ctx=ctx)
            tc = run(lambda: L.loop_candidates_tables(d_s, d_c, resident, shape=(Q, E), **args))
            tu = run(lambda: L.loop_candidates_tables(d_s, d_c, table, shape=(Q, E), **args))
            resident.free()
            # the library calls alone, on blocks made once
            a = L._Args(Q, E, table, connected, pick, pick, None, NB, "loop")
            Wd = (E + 31) // 32
            blocks = [ctx.upload(a.best), ctx.upload(a.excl), ctx.malloc(L.workspace_bytes(Q, E)), ctx.malloc(8 * Q * E),
                      ctx.malloc(4 * Q * E), ctx.malloc(4 * Q * Wd), ctx.malloc(4 * max(len(want.ids), 4)), ctx.malloc(4 * max(len(want.ids), 4))]
            d_best, d_excl, ws, d_acc, d_gb, d_bm, d_ids, d_sc = blocks
            counts, off = np.zeros(Q, np.int64), np.zeros(Q + 1, np.int64)

            def stage():
                assert lib.slam_loop_candidates(h, Q, E, d_s.ptr, d_c.ptr, a.nb, d_best.ptr, d_excl.ptr, addr(a.excl_off), addr(a.own), addr(a.limit),
                                                addr(a.min_s), 0, ws.ptr, d_acc.ptr, d_gb.ptr, d_bm.ptr, addr(counts), None) == 0
                off[1:] = np.cumsum(counts)
                assert off[-1] == len(want.ids)
                assert lib.slam_loop_fill(h, Q, E, d_s.ptr, d_bm.ptr, ws.ptr, addr(off), d_ids.ptr, d_sc.ptr) == 0

            ts = run(stage)
            equal = equal and np.array_equal(d_ids.download(np.int32, (len(want.ids),)), want.ids) if len(want.ids) else equal
            th = wall(lambda: L.loop_candidates_host(s, c, table, keep_stages=False, **args))
            print(f"members per query {len(want.ids) / Q:.2f}; device equal to the numpy statement in every bit: {equal}")
            print(f"stage   (library calls, HIP events)       : {spread(ts)}  {np.median(ts) * 1e3 / Q:9.2f} us / query")
            print(f"call    (loop_candidates_tables, events)  : {spread(tc)}")
            print(f"call    (the same, best table uploaded)   : {spread(tu)}")
            print(f"query   (scores_dense_device, events)     : {spread(tq)}")
            print(f"host    (loop_candidates_host, one core)  : {spread(th)}  -> the stage is {np.median(th) / np.median(ts):.2f} x the numpy statement's speed, "
                  f"the call {np.median(th) / np.median(tc):.2f} x")
            if Q == 1:
                conn = connected[0][connected[0] < E]
                tp = wall(lambda: bow.detect_loop_candidates(db, vec, conn))
                both = np.median(tq) + np.median(tc)
                verdict = "WINS over" if both < np.median(tp) else "LOSES to"
                print(f"parent  (detect_loop_candidates, wall)    : {spread(tp)}  -> query + call = {both * 1e3:.1f} us {verdict} the parent's path, "
                      f"{np.median(tp) / both:.2f} x (the parent stops after the first stage and sees the whole database)")
            sys.stdout.flush()
            for b in blocks + [d_s, d_c]:
                b.free()
        db.free()
    vocab.free()


if __name__ == "__main__":
    main()
