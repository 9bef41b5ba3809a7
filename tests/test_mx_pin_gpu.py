"""GPU: pinned train sets (slam_bf_train_pin / _refresh / _unpin; DESIGN.md 3c "Pinned train sets").  The image path is forced at
small shapes (engine 3, slam_bf_set_mx_feed 2) and every table is compared bit for bit with the VALU kernel (engine 1) on the
same arrays: pinned = unpinned = engine 1 on ragged shapes, the image-launch counter still over pinned searches and moving by
one per unpinned one, rows rewritten in place seen after a refresh and at once after an unpin, two pinned sets alternating, the
ninth pin refused, a pin replaced under another M, a freed and reallocated buffer never meeting the old image, engines 1 and 2,
a train_base, the select and keep entry points, two threads on one pinned set, and the context's own image buffer poisoned.
The merge state is idle after every search.

No test here provokes a fault, and every shape is memory-safe by construction: a pinned image is allocated for exactly M padded
to whole stages of 128 rows and written whole by the image kernel before any search is queued behind it, every stage the search
copies starts on a multiple of 128 rows below M, and an image is freed only behind a stream synchronisation."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MS = (1, 127, 128, 129, 1057, 16461)
NS = (33, 300)


@pytest.fixture(scope="module")
def pctx(built):
    """One context for the file: registrations, the launch counter and the feed setting live on it from test to test."""
    import slamhip

    ctx = slamhip.Context()
    yield ctx
    assert ctx.train_pins() == 0, "a test left a train set pinned"
    ctx.close()


def _rows(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def _search(ctx, dq, n, dt, m, engine, feed=0, base=0):
    """One top-2 search on device rows under (engine, feed): (idx, dist, image launches it issued)."""
    import slamhip

    tab = slamhip.Top2Table(ctx, n)
    ctx.set_engine(engine)
    ctx.set_mx_feed(feed)
    try:
        before = ctx.mx_image_launches()
        slamhip.knn2_device(ctx, dq.buf, n, dt.buf, m, tab.idx, tab.dist, base)
        launches = ctx.mx_image_launches() - before
        idx, dist = tab.download()
    finally:
        ctx.set_engine(0)
        ctx.set_mx_feed(0)
        tab.free()
    assert ctx.state_dirty() == 0, "the search left its merge state dirty"
    return idx, dist, launches


def _pin(ctx, dt):
    """Pin with feed 2 forced, as a caller that forces the image would: an M outside the pinned rule gets its image then."""
    ctx.set_mx_feed(2)
    try:
        dt.pin()
    finally:
        ctx.set_mx_feed(0)


def _same(a, b, what=""):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), what


@pytest.fixture(scope="module")
def cases():
    """(query rows, train rows) for every shape: built once, left unchanged."""
    out = {}
    for m in MS:
        for n in NS:
            rng = np.random.default_rng(5000 * m + n)
            q, t = _rows(rng, n), _rows(rng, m)
            t[m - 1] = q[n - 1]                                  # the last row is the last query's nearest
            out[m, n] = (q, t)
    return out


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("m", MS)
def test_pinned_equals_unpinned_equals_valu_and_the_counter_tells_them_apart(pctx, cases, m, n):
    import slamhip

    q, t = cases[m, n]
    dq, dt = slamhip.DeviceDescriptors(pctx, q), slamhip.DeviceDescriptors(pctx, t)
    try:
        ref = _search(pctx, dq, n, dt, m, 1)
        assert ref[2] == 0 and ref[0][n - 1, 0] == m - 1 and ref[1][n - 1, 0] == 0
        for _ in range(2):
            un = _search(pctx, dq, n, dt, m, 3, 2)
            _same(un, ref, "unpinned")
            assert un[2] == 1                                    # one image launch per unpinned feed-2 search
        c0 = pctx.mx_image_launches()
        _pin(pctx, dt)
        assert pctx.mx_image_launches() == c0 + 1 and pctx.train_pins() == 1
        for _ in range(3):
            pin = _search(pctx, dq, n, dt, m, 3, 2)
            _same(pin, ref, "pinned")
            assert pin[2] == 0                                   # ... and none over pinned ones
        dt.unpin()
        assert pctx.train_pins() == 0
        assert _search(pctx, dq, n, dt, m, 3, 2)[2] == 1
    finally:
        for o in (dq, dt):
            o.free()


def test_rows_rewritten_in_place_are_seen_after_a_refresh_and_at_once_after_an_unpin(pctx):
    import slamhip

    rng = np.random.default_rng(21)
    n, m = 300, 1057
    q, t1, t2, t3 = _rows(rng, n), _rows(rng, m), _rows(rng, m), _rows(rng, m)
    t1[1000], t2[17], t3[640] = q[5], q[5], q[5]
    dq, dt = slamhip.DeviceDescriptors(pctx, q), slamhip.DeviceDescriptors(pctx, t1)
    try:
        _pin(pctx, dt)
        a = _search(pctx, dq, n, dt, m, 3, 2)
        dt.buf.upload(t2)                                        # same pointer, same size, other rows
        c0 = pctx.mx_image_launches()
        dt.refresh()
        assert pctx.mx_image_launches() == c0 + 1
        b = _search(pctx, dq, n, dt, m, 3, 2)
        assert a[2] == 0 and b[2] == 0
        dt.unpin()
        dt.buf.upload(t3)
        c = _search(pctx, dq, n, dt, m, 3, 2)                    # unpinned: the default contract, rebuilt by the search itself
        assert c[2] == 1
        for got, t, row in ((a, t1, 1000), (b, t2, 17), (c, t3, 640)):
            dt.buf.upload(t)
            _same(got, _search(pctx, dq, n, dt, m, 1))
            assert got[0][5, 0] == row and got[1][5, 0] == 0
        with pytest.raises(slamhip.SlamHipError, match="not a pinned train set"):
            dt.refresh()
        with pytest.raises(slamhip.SlamHipError, match="not a pinned train set"):
            dt.unpin()
    finally:
        for o in (dq, dt):
            o.free()


def test_two_pinned_sets_alternate_on_one_context(pctx):
    import slamhip

    rng = np.random.default_rng(22)
    n = 300
    q = _rows(rng, n)
    ta, tb = _rows(rng, 1057), _rows(rng, 16461)
    ta[1056], tb[9000] = q[3], q[3]
    dq, da, db = (slamhip.DeviceDescriptors(pctx, x) for x in (q, ta, tb))
    try:
        ra, rb = _search(pctx, dq, n, da, 1057, 1), _search(pctx, dq, n, db, 16461, 1)
        _pin(pctx, da)
        _pin(pctx, db)
        assert pctx.train_pins() == 2
        for _ in range(3):
            for d, m, ref, row in ((da, 1057, ra, 1056), (db, 16461, rb, 9000)):
                got = _search(pctx, dq, n, d, m, 3, 2)
                _same(got, ref)
                assert got[2] == 0 and got[0][3, 0] == row
        # a search of a sub-range of a pinned set is a search of an unpinned one: exact match of pointer and M only
        sub = _search(pctx, dq, n, db, 1057, 3, 2)
        db_sub = slamhip.DeviceDescriptors(pctx, tb[:1057])
        try:
            _same(sub, _search(pctx, dq, n, db_sub, 1057, 1))
        finally:
            db_sub.free()
        assert sub[2] == 1
    finally:
        for o in (dq, da, db):                                   # free() of a pinned buffer unpins it
            o.free()
    assert pctx.train_pins() == 0


def test_a_ninth_pin_is_refused_and_a_pin_again_replaces_the_registration(pctx):
    import slamhip
    from slamhip._lib import check

    rng = np.random.default_rng(23)
    n, m = 33, 300
    q, t = _rows(rng, n), _rows(rng, m)
    dq = slamhip.DeviceDescriptors(pctx, q)
    sets = [slamhip.DeviceDescriptors(pctx, t) for _ in range(9)]
    try:
        for d in sets[:8]:
            _pin(pctx, d)
        assert pctx.train_pins() == 8
        with pytest.raises(slamhip.SlamHipError, match="already holds 8 pinned train sets"):
            sets[8].pin()
        assert pctx.train_pins() == 8
        # the same pointer again, with another M: no new slot, and only the new M meets the image
        pctx.set_mx_feed(2)
        try:
            pctx.pin_train(sets[0].buf, 129)
        finally:
            pctx.set_mx_feed(0)
        assert pctx.train_pins() == 8
        ref_all, ref_129 = _search(pctx, dq, n, sets[0], m, 1), _search(pctx, dq, n, sets[0], 129, 1)
        got_all, got_129 = _search(pctx, dq, n, sets[0], m, 3, 2), _search(pctx, dq, n, sets[0], 129, 3, 2)
        _same(got_all, ref_all)
        _same(got_129, ref_129)
        assert got_all[2] == 1 and got_129[2] == 0
        sets[1].unpin()
        _pin(pctx, sets[8])                                      # a slot is free again
        assert _search(pctx, dq, n, sets[8], m, 3, 2)[2] == 0
    finally:
        for o in [dq] + sets:
            o.free()
    assert pctx.train_pins() == 0
    # rows that lie in no allocation of the context are refused (the pointer is compared, never read): slam_free could not
    # drop such a registration
    with pytest.raises(slamhip.SlamHipError, match="not inside one slam_malloc allocation"):
        check(pctx.lib.slam_bf_train_pin(pctx.handle, 0x1000, 128))


def test_a_freed_pinned_buffer_takes_its_registration_along(pctx):
    import slamhip

    rng = np.random.default_rng(24)
    n, m = 300, 1057
    q, t1, t2 = _rows(rng, n), _rows(rng, m), _rows(rng, m)
    t1[1000], t2[17] = q[5], q[5]
    dq = slamhip.DeviceDescriptors(pctx, q)
    held = []
    try:
        count = pctx.train_pins()
        d1 = slamhip.DeviceDescriptors(pctx, t1)
        ptr = d1.buf.ptr
        _pin(pctx, d1)
        assert _search(pctx, dq, n, d1, m, 3, 2)[0][5, 0] == 1000
        d1.free()
        assert pctx.train_pins() == count
        # the allocator usually hands the same address out again for the same size: search whatever it gives, and say which
        for _ in range(4):
            held.append(slamhip.DeviceDescriptors(pctx, t2))
            if held[-1].buf.ptr == ptr:
                break
        d2 = held[-1]
        got = _search(pctx, dq, n, d2, m, 3, 2)
        _same(got, _search(pctx, dq, n, d2, m, 1))
        assert got[2] == 1 and got[0][5, 0] == 17, ("same address" if d2.buf.ptr == ptr else "another address")
        assert pctx.train_pins() == count
    finally:
        for o in [dq] + held:
            o.free()


def test_other_engines_a_train_base_and_the_select_and_keep_forms(pctx):
    import slamhip
    from slamhip.matching import MODE_ALL, _match_host

    rng = np.random.default_rng(25)
    n, m, base = 300, 16461, 123456
    q, t = _rows(rng, n), _rows(rng, m)
    t[4097] = q[17]
    dq, dt = slamhip.DeviceDescriptors(pctx, q), slamhip.DeviceDescriptors(pctx, t)
    tab, keep, qkeep = slamhip.Top2Table(pctx, n), pctx.malloc(n), pctx.malloc(n * 32)
    try:
        ref = _search(pctx, dq, n, dt, m, 1)
        ref_base = _search(pctx, dq, n, dt, m, 1, base=base)

        def forms(engine, feed):
            """The select form (all, ratio) with a train_base, and the keep form (slam_bf_match_host on device train rows)."""
            pctx.set_engine(engine)
            pctx.set_mx_feed(feed)
            try:
                c0, out = pctx.mx_image_launches(), []
                for mode in (0, 2):
                    cnt = slamhip.knn2_select_device(pctx, dq.buf, n, dt.buf, m, tab.idx, tab.dist, keep, mode=mode, param=0.8,
                                                     train_base=base)
                    out += [np.asarray(cnt), keep.download(np.uint8, (n,))] + list(tab.download())
                pctx.lib.slam_memset(pctx.handle, qkeep.ptr, 0xEE, n * 32)
                out += list(_match_host(pctx, q, None, dt.buf, m, qkeep, MODE_ALL, 0.0))
                out.append(qkeep.download(np.uint8, (n, 32)))
                return out, pctx.mx_image_launches() - c0
            finally:
                pctx.set_engine(0)
                pctx.set_mx_feed(0)

        want, _ = forms(1, 0)
        assert np.array_equal(want[-1], q) and want[2][17, 0] == base + 4097
        unpinned, launches = forms(3, 2)
        assert launches == 3                                     # the three forms reach the matrix-core pass: an image each
        _pin(pctx, dt)
        # engines 1 and 2 and feed 1 leave the image unused, engine 3 under feed 2 reads it: no launch either way
        for engine, feed in ((1, 0), (2, 0), (2, 2), (3, 1), (3, 2), (0, 0)):
            got = _search(pctx, dq, n, dt, m, engine, feed)
            _same(got, ref, (engine, feed))
            _same(_search(pctx, dq, n, dt, m, engine, feed, base=base), ref_base, (engine, feed, "base"))
            out, launches = forms(engine, feed)
            assert launches == 0 == got[2], (engine, feed)
            for x, y in zip(out, want):
                assert np.array_equal(x, y), (engine, feed)
            assert pctx.state_dirty() == 0
        for x, y in zip(unpinned, want):
            assert np.array_equal(x, y)
    finally:
        for o in (tab, keep, qkeep, dq, dt):
            o.free()


def test_two_threads_search_one_pinned_set(pctx):
    import slamhip

    rng = np.random.default_rng(26)
    n, m, rounds = 300, 16461, 6
    qs = [_rows(rng, n) for _ in range(2)]
    t = _rows(rng, m)
    t[77], t[m - 1] = qs[0][1], qs[1][1]
    dt = slamhip.DeviceDescriptors(pctx, t)
    dqs = [slamhip.DeviceDescriptors(pctx, q) for q in qs]
    tabs = [slamhip.Top2Table(pctx, n) for _ in range(2)]
    try:
        serial = [_search(pctx, dq, n, dt, m, 1) for dq in dqs]
        _pin(pctx, dt)
        pctx.set_engine(3)
        pctx.set_mx_feed(2)
        c0 = pctx.mx_image_launches()
        got, errors = [[], []], []

        def work(k):
            try:
                for _ in range(rounds):
                    slamhip.knn2_device(pctx, dqs[k].buf, n, dt.buf, m, tabs[k].idx, tabs[k].dist)
                    got[k].append(tabs[k].download())
            except Exception as exc:   # noqa: BLE001 - reported by the main thread
                errors.append(exc)

        threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors
        assert pctx.mx_image_launches() == c0 and pctx.state_dirty() == 0
        for k in range(2):
            assert len(got[k]) == rounds
            for tabk in got[k]:
                _same(tabk, serial[k], k)
    finally:
        pctx.set_engine(0)
        pctx.set_mx_feed(0)
        for o in tabs + dqs + [dt]:
            o.free()


def test_the_context_s_own_image_buffer_poisoned_changes_nothing(pctx):
    import slamhip

    rng = np.random.default_rng(27)
    n, m = 300, 1057
    q, t = _rows(rng, n), _rows(rng, m)
    dq, dt = slamhip.DeviceDescriptors(pctx, q), slamhip.DeviceDescriptors(pctx, t)
    try:
        ref = _search(pctx, dq, n, dt, m, 1)
        assert _search(pctx, dq, n, dt, m, 3, 2)[2] == 1 and pctx.mx_image_bytes() > 0    # the context's buffer exists
        _pin(pctx, dt)
        grown = pctx.mx_image_bytes()
        pctx.fill_mx_image(0xFF)
        got = _search(pctx, dq, n, dt, m, 3, 2)
        _same(got, ref)
        assert got[2] == 0 and pctx.mx_image_bytes() == grown    # the pinned image is a block of its own
    finally:
        for o in (dq, dt):
            o.free()


def test_a_set_no_search_would_take_the_image_for_is_recorded_without_one(pctx):
    """Feed 0 at pin time and an M outside the pinned rule's range: a registration, no allocation, no launch; a forced feed 2
    then builds the context's image per search, as for an unpinned set."""
    import slamhip

    rng = np.random.default_rng(28)
    n, m = 33, 1057
    assert all(slamhip.mx_feed_describe_pinned(k, m) == 1 for k in (1, 8192, 65536, 131072, 1 << 20))
    q, t = _rows(rng, n), _rows(rng, m)
    dq, dt = slamhip.DeviceDescriptors(pctx, q), slamhip.DeviceDescriptors(pctx, t)
    try:
        c0 = pctx.mx_image_launches()
        dt.pin()
        dt.refresh()
        assert pctx.mx_image_launches() == c0 and pctx.train_pins() == 1
        got = _search(pctx, dq, n, dt, m, 3, 2)
        _same(got, _search(pctx, dq, n, dt, m, 1))
        assert got[2] == 1
    finally:
        for o in (dq, dt):
            o.free()
    assert pctx.train_pins() == 0
