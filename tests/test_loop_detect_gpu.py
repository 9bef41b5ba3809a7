"""Loop and relocalisation candidates on the device (csrc/loop_detect.hip) against the numpy statement
slamhip.loop_candidates_host, bit for bit on acc, gbest, the bitmap, the counts, the ids and the scores of every scene of
tests/loop_detect_cases.py.  Every call runs twice: on a workspace filled with 0xFF and outputs filled with 0xA5, then on what
the first run left in the same blocks.  Then one run through a real BowDatabase: the resident dense tables against the
downloaded ones, and a LoopDetector over a sequence that comes back to where it began."""
import ctypes
import os

import numpy as np
import pytest

import bow_ref
import loop_detect_cases as C

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class Blocks:
    """Stands in for ``loop_detect._new``: every block a call takes is remembered and filled - a workspace with 0xFF, an output
    with 0xA5 - and handed out as a view, so that it outlives the call; ``twice`` hands the same blocks out once more, in the
    same order, as the first run left them."""

    def __init__(self, monkeypatch):
        from slamhip import loop_detect

        self.blocks, self.replay = [], []
        monkeypatch.setattr(loop_detect, "_new", self.new)

    def new(self, ctx, held, nbytes, role):
        n = max(int(nbytes), 16)
        if self.replay:
            b, was, size = self.replay.pop(0)
            assert (was, size) == (role, n)
        else:
            b = ctx.malloc(n)
            b.upload(np.full(n, 0xFF if role == "ws" else 0xA5, np.uint8))
        self.blocks.append((b, role, n))
        return b.view(0, n)


def twice(blocks, fn):
    """``fn()`` on poisoned blocks and again on the leftovers -> both results; the blocks of the two runs are freed."""
    base = len(blocks.blocks)
    try:
        first = fn()
        blocks.replay = blocks.blocks[base:]
        del blocks.blocks[base:]
        second = fn()
        assert not blocks.replay                                     # the second run took the blocks of the first, all of them
        return first, second
    finally:
        for b, _, _ in blocks.blocks[base:] + blocks.replay:
            b.free()
        del blocks.blocks[base:]
        blocks.replay = []


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_candidates(got, want):
    gs, ws = got.stages(), want.stages()
    return (_same(got.offsets, want.offsets) and _same(got.ids, want.ids) and _same(got.scores, want.scores) and got.skipped == want.skipped
            and all(_same(gs[k], ws[k]) for k in ("acc", "gbest", "bitmap")))


def index_errors(ctx):
    n = ctypes.c_int64(0)
    assert ctx.lib.slam_index_errors(ctx.handle, ctypes.byref(n)) == 0
    return n.value


@pytest.mark.parametrize("name", C.names())
def test_scene_equals_host_statement(gpu_ctx, monkeypatch, name):
    from slamhip import loop_candidates_host, loop_candidates_tables

    s = C.scenes()[name]
    want = loop_candidates_host(s.s, s.common, **s.kwargs())
    blocks = Blocks(monkeypatch)
    index_errors(gpu_ctx)                                            # clear
    for got in twice(blocks, lambda: loop_candidates_tables(s.s, s.common, keep_stages=True, ctx=gpu_ctx, **s.kwargs())):
        assert same_candidates(got, want), name
        assert [got[q][0].tolist() for q in range(s.Q)] == [want[q][0].tolist() for q in range(s.Q)]
    assert index_errors(gpu_ctx) == 2 * want.skipped == 2 * s.expect.get("skipped", want.skipped)


def test_resident_tables_and_results_without_stages(gpu_ctx, monkeypatch):
    """The same call on tables that are device buffers already, and without the stages kept."""
    from slamhip import BestTable, loop_candidates_host, loop_candidates_tables

    s = C.scenes()["random-7-3"]                                     # E = T + 1, Q = 3, nb = 16
    want = loop_candidates_host(s.s, s.common, **s.kwargs())
    d_s, d_c = gpu_ctx.upload(s.s), gpu_ctx.upload(s.common)
    try:
        blocks = Blocks(monkeypatch)
        for got in twice(blocks, lambda: loop_candidates_tables(d_s, d_c, shape=(s.Q, s.E), **s.kwargs())):
            assert _same(got.offsets, want.offsets) and _same(got.ids, want.ids) and _same(got.scores, want.scores)
            with pytest.raises(ValueError):
                got.stages()
        assert _same(d_s.download(np.uint32, s.s.shape), s.s) and _same(d_c.download(np.int32, s.common.shape), s.common)
        with pytest.raises(ValueError):
            loop_candidates_tables(d_s, d_c, **s.kwargs())             # no shape
        with pytest.raises(ValueError):
            loop_candidates_tables(d_s, d_c, shape=(s.Q + 1, s.E), **s.kwargs())
        # the best table resident as well: only the lists and the results cross
        wide = np.concatenate([s.best, np.full((7, s.nb), -1)])      # a table of more keyframes than the database has entries
        table = BestTable(wide, ctx=gpu_ctx)
        try:
            kw = dict(s.kwargs(), best_table=table)
            for got in twice(blocks, lambda: loop_candidates_tables(d_s, d_c, shape=(s.Q, s.E), keep_stages=True, **kw)):
                assert same_candidates(got, want)
            with pytest.raises(ValueError):
                loop_candidates_tables(d_s, d_c, shape=(s.Q, s.E), **dict(kw, nb=s.nb - 1))
        finally:
            table.free()
        with pytest.raises(ValueError):
            loop_candidates_tables(d_s, d_c, shape=(s.Q, s.E), **kw)       # freed
        for bad in (np.zeros((4, 0), np.int32), np.zeros((4, 17), np.int32), np.zeros((4, 2))):
            with pytest.raises(ValueError):
                BestTable(bad, ctx=gpu_ctx)
    finally:
        d_s.free()
        d_c.free()
    none = loop_candidates_tables(np.zeros((0, 5), np.uint32), np.zeros((0, 5), np.int32), np.zeros((5, 2), np.int32), connected=[], ctx=gpu_ctx)
    assert len(none) == 0 and none.offsets.tolist() == [0] and len(none.ids) == 0


# ---- through a real database ----------------------------------------------------------------------------------------------------
def _world():
    """25 keyframes of 200 descriptors over the two weighted words of the small vocabulary: 0 .. 5 a place (mostly word 0, the
    share rising), 6 .. 19 a way elsewhere (mostly word 1, the share of word 0 rising from a tenth), 20 .. 24 the place again.
    The share moves one way inside each part, so a keyframe is nearer to the two before it than to anything earlier."""
    from slamhip import CovisibilityGraph, bow

    vocab = bow.read_dbow2_text(os.path.join(GOLDEN, "bow_vocab_small.txt"))
    rows = np.random.default_rng(1).integers(0, 256, (64, 32), dtype=np.uint8)
    words = bow_ref.transform(vocab.arrays(), rows)[0]
    d0, d1 = rows[np.flatnonzero(words == 0)[0]], rows[np.flatnonzero(words == 1)[0]]
    n0 = [180 + 2 * k for k in range(6)] + [20 + 8 * k for k in range(14)] + [181 + 2 * k for k in range(5)]
    images = [np.concatenate([np.repeat(d0[None], n, 0), np.repeat(d1[None], 200 - n, 0)]) for n in n0]
    K = len(images)
    edges = [(k, k + 1) for k in range(K - 1)] + [(k, k + 2) for k in range(K - 2)]
    graph = CovisibilityGraph(K, edges, [50] * (K - 1) + [20] * (K - 2))
    return vocab, images, graph


def test_database_tables_stay_resident_and_the_loop_closes_at_the_third_consistent_keyframe(gpu_ctx):
    from backend import Backend
    from slamhip import CovisibilityGraph, LoopDetector, bow, loop_candidates_host

    vocab, images, graph = _world()
    K = len(images)
    db = bow.BowDatabase(vocab, gpu_ctx)
    off = np.concatenate([[0], np.cumsum([len(i) for i in images])])
    vectors = bow.bow_vectors(vocab, np.concatenate(images), off, ctx=gpu_ctx)
    try:
        assert all(vectors[k].words.tolist() == [0, 1] for k in range(K))
        # the whole trajectory replayed in one call: keyframe k sees the entries below k, without those it was connected to then
        db.add_vectors(vectors)
        connected = [graph.connected(k)[graph.connected(k) < k] for k in range(K)]
        own, limit = np.arange(K), np.arange(K)
        d_s, d_c, Q, E = db.scores_dense_device(vectors)
        try:
            s, c = db.scores_dense(vectors)
            assert (Q, E) == (K, K) and _same(d_s.download(np.uint32, (K, K)), s) and _same(d_c.download(np.int32, (K, K)), c)
        finally:
            d_s.free()
            d_c.free()
        got = Backend().detect_loop(db, vectors, graph, connected, own, limit)
        want = loop_candidates_host(s, c, graph, connected, own, limit)
        assert _same(got.offsets, want.offsets) and _same(got.ids, want.ids) and _same(got.scores, want.scores) and got.skipped == 0
        for k in range(20, K):                                       # back at the place: its first keyframes, and nothing from the way there
            assert len(got[k][0]) and set(got[k][0].tolist()) <= set(range(6)), k
        assert all(len(got[k][0]) == 0 for k in list(range(6)) + list(range(8, 20)))
        reloc = Backend().detect_relocalization_candidates(db, vectors[21], graph.best_table(10))
        want = loop_candidates_host(s[21:22], c[21:22], graph.best_table(10), mode="relocalization")
        assert _same(reloc.ids, want.ids) and _same(reloc.scores, want.scores) and len(reloc.ids)
        assert index_errors(gpu_ctx) == 0
        # one keyframe at a time
        db.free()
        db = bow.BowDatabase(vocab, gpu_ctx)
        det = LoopDetector(db, threshold=3, min_gap=10, nb=10)
        accepted = [det.step(vectors[k], graph) for k in range(K)]
        assert len(db) == K and index_errors(gpu_ctx) == 0
        # 20 starts the group at 0, 21 and 22 continue it, 23 is the third consistent keyframe
        assert all(a == [] for a in accepted[:23]) and accepted[23] and set(accepted[23]) <= set(range(6))
        assert det.last.ids.tolist() == got[24][0].tolist() and len(det.last.ids)       # the last step saw what the replay saw
        # the gate: a loop closed at 23 keeps 24 .. 32 from detecting
        db.free()
        db = bow.BowDatabase(vocab, gpu_ctx)
        det = LoopDetector(db, threshold=0, min_gap=10, nb=10)
        for k in range(21):
            det.step(vectors[k], graph)
        det.loop_closed(20)
        assert det.step(vectors[21], graph) == [] and det.last is None and len(db) == 22
        det.loop_closed(11)
        assert det.step(vectors[22], graph) and det.last is not None
        with pytest.raises(ValueError):                              # a graph that does not know the database's keyframes
            det.step(vectors[23], CovisibilityGraph(3, [(0, 1)], [1]))
        assert len(db) == 23
    finally:
        vectors.free()
        db.free()
        vocab.free()
