"""GPU: the 32x32x64 matrix-core top-2 search fed from the prepared image of the train set (engine 3, slam_bf_set_mx_feed 2:
bf_mx_image_kernel, then bf_mx32_image_top2_kernel) against the VALU kernel (engine 1) - tables bit for bit and the merge state
idle after every search: ragged train and query counts around a group, a stage and a chunk, nearest rows planted on both sides
of a stage and of a chunk boundary (one worker per query block, and many) and in the ragged tail, a smaller search after a
larger one (the stale image is never read), a train buffer overwritten in place (the image is rebuilt), the buffer grown between
two small searches, the buffer poisoned before a search, the fused selection, and the two feeds alternating on one context.

No test here provokes a fault, and every shape is memory-safe by construction: the image holds the train set padded to whole
stages of 128 rows, every stage the search copies starts on a multiple of 128 rows below M, and the image kernel writes the
whole padded image in front of every search that reads it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ONE_WORKER_N = 513 * 256       # more query blocks than 4 x 256 CUs hold: one worker per query block


@pytest.fixture(scope="module")
def fctx(built):
    """One context for the file: the image buffer and the feed setting live on it from test to test."""
    import slamhip

    ctx = slamhip.Context()
    yield ctx
    ctx.close()


def _rows(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def _search(ctx, q, t, engine, feed=0, dev=None):
    import slamhip

    ctx.set_engine(engine)
    ctx.set_mx_feed(feed)
    dq, dt = dev or (slamhip.DeviceDescriptors(ctx, q), slamhip.DeviceDescriptors(ctx, t))
    tab = slamhip.Top2Table(ctx, len(q))
    try:
        slamhip.knn2_device(ctx, dq.buf, len(q), dt.buf, len(t), tab.idx, tab.dist)
        out = tab.download()
    finally:
        ctx.set_engine(0)
        ctx.set_mx_feed(0)
        for o in (tab,) + (() if dev else (dq, dt)):
            o.free()
    assert ctx.state_dirty() == 0, "the search left its merge state dirty"
    return out


def _agree(ctx, q, t, what=""):
    a = _search(ctx, q, t, 1)
    b = _search(ctx, q, t, 3, 2)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), what
    return b


def _flip(row, d, rng):
    """`row` with d distinct bits flipped."""
    bits = np.unpackbits(row)
    bits[rng.permutation(256)[:d]] ^= 1
    return np.packbits(bits)


@pytest.mark.parametrize("n", [33, 64, 65, 300])
@pytest.mark.parametrize("m", [1, 31, 32, 33, 127, 128, 129, 160, 287, 1057, 16461])
def test_ragged_shapes(fctx, m, n):
    rng = np.random.default_rng(1000 * m + n)
    q, t = _rows(rng, n), _rows(rng, m)
    t[m - 1] = q[n - 1]                                          # the last row is the last query's nearest
    if m > 40:
        t[m // 2] = _flip(q[0], 3, rng)
    idx, dist = _agree(fctx, q, t, (m, n))
    assert idx[n - 1, 0] == m - 1 and dist[n - 1, 0] == 0
    assert fctx.mx_image_bytes() >= (m + 127) // 128 * 128 * 128


def _boundaries(ctx, n, m):
    """(chunk boundaries, stage starts inside a chunk) of the plan the search of n x m runs on this device."""
    import slamhip

    plan, tbl = slamhip.mx_plan_describe(n, m, num_cu=ctx.plan_info(n, m)["cus"])
    tbl = [int(v) for v in tbl]
    assert tbl[0] == 0 and tbl[-1] == m and all(v % 128 == 0 for v in tbl[:-1])
    inner = [s for a, b in zip(tbl[:-1], tbl[1:]) for s in range(a + 128, b, 128)]
    return plan, tbl[1:-1], inner


@pytest.mark.parametrize("n,m,workers", [(300, 16461, "many"), (16385, 16461, "several"), (ONE_WORKER_N, 1057, "one")])
def test_planted_pairs_at_stage_and_chunk_boundaries_and_in_the_tail(fctx, n, m, workers):
    rng = np.random.default_rng(n + m)
    plan, chunks, inner = _boundaries(fctx, n, m)
    assert (plan["workers"] == 1) == (workers == "one") and chunks
    if workers != "many":
        assert inner, "this shape is here for its chunks of more than one stage"
    q, t = _rows(rng, n), _rows(rng, m)
    tail0 = (m - 1) // 128 * 128                                 # first row of the ragged last stage
    assert tail0 + 32 <= m - 1 and m % 32 != 0
    pairs = [(c - 1, c) for c in (chunks[0], chunks[len(chunks) // 2], chunks[-1])]
    pairs += [(s - 1, s) for s in (inner[:1] + inner[-1:])]      # last group of a stage, first group of the next
    pairs += [(tail0 - 1, tail0), (tail0 + 31, tail0 + 32), (m - 2, m - 1)]
    pairs = list(dict.fromkeys(pairs))
    assert len({r for p in pairs for r in p}) == 2 * len(pairs) or workers == "one"
    # query k has its two nearest rows at pair k: nearest below the boundary, nearest above it, a tie (the lower row first).
    # The variants share their rows, so each is a search of its own
    for da, db in ((4, 9), (9, 4), (6, 6)):
        tv, want, used = t.copy(), {}, set()
        for k, (a, b) in enumerate(pairs):
            if a in used or b in used:                           # (the one-worker shape's tail is short: two pairs share a row)
                continue
            used |= {a, b}
            tv[a], tv[b] = _flip(q[k], da, rng), _flip(q[k], db, rng)
            want[k] = ([a, b], [da, db]) if da <= db else ([b, a], [db, da])
        idx, dist = _agree(fctx, q, tv, (workers, da, db))
        for k, (wi, wd) in want.items():
            assert idx[k].tolist() == wi and dist[k].tolist() == wd, (workers, k, idx[k], dist[k], wi, wd)


def test_a_smaller_search_never_reads_the_larger_one_s_image(fctx):
    rng = np.random.default_rng(7)
    n = 300
    q = _rows(rng, n)
    big = _rows(rng, 1057)
    big[300:] = q[np.arange(757) % n]                            # under the old image every query's best rows lie in 300 .. 1056
    idx, dist = _agree(fctx, q, big)
    assert (dist[:, 0] == 0).all() and (idx[:, 0] >= 300).all()
    small = _rows(rng, 300)
    idx, dist = _agree(fctx, q, small)
    assert (idx < 300).all() and (dist[:, 0] > 0).all()


def test_a_train_buffer_overwritten_in_place_is_expanded_again(fctx):
    import slamhip

    rng = np.random.default_rng(8)
    n, m = 300, 1057
    q, t1, t2 = _rows(rng, n), _rows(rng, m), _rows(rng, m)
    t1[1000], t2[17] = q[5], q[5]
    dev = (slamhip.DeviceDescriptors(fctx, q), slamhip.DeviceDescriptors(fctx, t1))
    try:
        first = _search(fctx, q, t1, 3, 2, dev)
        dev[1].buf.upload(t2)                                    # same pointer, same size, other rows
        second = _search(fctx, q, t2, 3, 2, dev)
    finally:
        for o in dev:
            o.free()
    for got, t in ((first, t1), (second, t2)):
        ref = _search(fctx, q, t, 1)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    assert first[0][5, 0] == 1000 and second[0][5, 0] == 17


def test_the_buffer_grows_between_two_small_searches(built):
    import slamhip

    rng = np.random.default_rng(9)
    q = _rows(rng, 65)
    small, large = _rows(rng, 129), _rows(rng, 16461)
    ctx = slamhip.Context()
    try:
        assert ctx.mx_image_bytes() == 0
        a = _agree(ctx, q, small)
        b0 = ctx.mx_image_bytes()
        assert 256 * 128 <= b0 < 16461 * 128
        _agree(ctx, q, large)
        b1 = ctx.mx_image_bytes()
        assert b1 >= 16512 * 128                                  # it grew: freed and allocated again
        c = _agree(ctx, q, small)
        assert ctx.mx_image_bytes() == b1
        assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
    finally:
        ctx.close()


@pytest.mark.parametrize("byte", [0xFF, 0x00])
def test_a_poisoned_image_buffer_changes_nothing(fctx, byte):
    rng = np.random.default_rng(10)
    q, t = _rows(rng, 300), _rows(rng, 1057)
    want = _agree(fctx, q, t)
    assert fctx.mx_image_bytes() > 0
    fctx.fill_mx_image(byte)
    got = _search(fctx, q, t[:287], 3, 2)                        # a ragged search right behind the poison
    ref = _search(fctx, q, t[:287], 1)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    fctx.fill_mx_image(byte)
    got = _search(fctx, q, t, 3, 2)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_select_and_train_base_through_the_image(fctx):
    import slamhip

    ctx = fctx
    rng = np.random.default_rng(77)
    n, m, base = 777, 5000, 123456
    q, t = _rows(rng, n), _rows(rng, m)
    t[4097] = q[17]
    res = {}
    for engine, feed in ((1, 0), (3, 2)):
        ctx.set_engine(engine)
        ctx.set_mx_feed(feed)
        dq, dt = slamhip.DeviceDescriptors(ctx, q), slamhip.DeviceDescriptors(ctx, t)
        tab = slamhip.Top2Table(ctx, n)
        keep = ctx.malloc(n)
        try:
            out = []
            for mode in (0, 2):
                cnt = slamhip.knn2_select_device(ctx, dq.buf, n, dt.buf, m, tab.idx, tab.dist, keep, mode=mode, param=0.8,
                                                 train_base=base)
                out += [np.asarray(cnt), keep.download(np.uint8, (n,))] + list(tab.download())
        finally:
            ctx.set_engine(0)
            ctx.set_mx_feed(0)
            for o in (tab, dq, dt, keep):
                o.free()
        assert ctx.state_dirty() == 0
        res[engine] = out
    for x, y in zip(res[1], res[3]):
        assert np.array_equal(x, y)
    assert res[3][2][17, 0] == base + 4097 and res[3][3][17, 0] == 0


def test_the_two_feeds_alternate_on_one_context(fctx):
    rng = np.random.default_rng(11)
    q = _rows(rng, 300)
    for k, m in enumerate((1057, 129, 1057, 16461, 33, 1057)):
        t = _rows(rng, m)
        t[m - 1] = q[k]
        ref = _search(fctx, q, t, 1)
        for feed in (1, 2, 1, 2):
            got = _search(fctx, q, t, 3, feed)
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (m, feed)
        assert ref[0][k, 0] == m - 1


def test_the_setter_refuses_other_values(fctx):
    from slamhip._lib import SLAM_ERR_INVALID

    for feed in (-1, 3, 4, 1 << 20):
        assert fctx.lib.slam_bf_set_mx_feed(fctx.handle, feed) == SLAM_ERR_INVALID
        assert b"feed must be" in fctx.lib.slam_last_error()
    assert fctx.lib.slam_bf_set_mx_feed(None, 1) == SLAM_ERR_INVALID
    for feed in (0, 1, 2, 0):
        fctx.set_mx_feed(feed)
