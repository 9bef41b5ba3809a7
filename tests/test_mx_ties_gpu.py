"""GPU: the matrix-core top-2 search (bf_mx.hip) on tie-heavy train sets - rows drawn from a few byte values, so that dozens of
rows tie at the 1st and 2nd distance; exact duplicates in lower and in higher chunks than the row they tie with; all rows
equal - with engine 2 against the VALU kernel (engine 1), bit for bit: both chunk regimes, one worker and 256 workers per
query block, the bf_select modes, two passes beyond 2^23 rows, and mixed MX / VALU traffic on one context with the merge
state (bound[] included) checked idle after every call.  Each case runs once.

This module shows AGREEMENT.  The kernel lets a distance tie into its update path only where the tie could win on the row
index, and whether a worker meets the one case where it can - another worker's bound from a higher row - depends on which
worker reads which bound, that is on timing.  What pins the rule is tests/test_mx_ties_cpu.py, where the schedule is chosen."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PASS = 1 << 23


@contextlib.contextmanager
def engine(ctx, e):
    ctx.set_engine(e)
    try:
        yield
    finally:
        ctx.set_engine(0)


def plan(ctx, n, m):
    import slamhip

    return slamhip.mx_plan_describe(n, m, num_cu=ctx.plan_info(n, m)["cus"])


def search(ctx, dq, n, dt, m, e, train_base=0):
    import slamhip

    tab = slamhip.Top2Table(ctx, n)
    try:
        with engine(ctx, e):
            slamhip.knn2_device(ctx, dq.buf, n, dt.buf, m, tab.idx, tab.dist, train_base)
            out = tab.download()
    finally:
        tab.free()
    assert ctx.state_dirty() == 0, "the search left its merge state dirty"
    return out


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- the tie-heavy families ---------------------------------------------------------------------------------------------

def few_values(rng, n, m):
    """Four bytes from {0x00, 0x0F}, the rest zero: every distance is 0, 4, 8, 12 or 16, and thousands of rows share each."""
    vals = np.array([0x00, 0x0F], np.uint8)
    q, t = np.zeros((n, 32), np.uint8), np.zeros((m, 32), np.uint8)
    q[:, :4] = vals[rng.integers(0, 2, (n, 4))]
    t[:, :4] = vals[rng.integers(0, 2, (m, 4))]
    return q, t


def duplicates(rng, n, m):
    """Random rows; up to 2048 queries get six exact copies of a row one bit away, spread over the whole train set: the top-2
    are the two lowest copies, and the others tie with them from higher chunks."""
    q = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    if m >= 64:
        who = rng.choice(n, min(n, 2048, m // 16), replace=False)
        v = q[who].copy()
        v[np.arange(len(who)), rng.integers(0, 32, len(who))] ^= np.uint8(1) << rng.integers(0, 8, len(who)).astype(np.uint8)
        rows = rng.choice(m, (len(who), 6), replace=False)
        for j in range(6):
            t[rows[:, j]] = v
    return q, t


def all_equal(rng, n, m):
    v = rng.integers(0, 256, 32, dtype=np.uint8)
    return np.tile(v, (n, 1)), np.tile(v, (m, 1))


FAMILIES = [few_values, duplicates, all_equal]

# (n, m, chunk rows, workers per query block; None: several, whatever the device holds)
REGIMES = [
    (1000, 150001, 256, 256),
    (65537, 30001, 1024, None),
    ((1 << 18) + 3, 16384, 1024, 1),
    ((1 << 18) + 3, 4000, 256, 1),
    (256, (1 << 21) + 130, 1024, 256),
]


@pytest.mark.parametrize("fam", FAMILIES, ids=lambda f: f.__name__)
@pytest.mark.parametrize("n,m,chunk,workers", REGIMES)
def test_tie_families_agree_with_the_valu_kernel(gpu_ctx, fam, n, m, chunk, workers):
    import slamhip

    ctx = gpu_ctx
    p, _ = plan(ctx, n, m)
    assert p["chunk"] == chunk
    assert p["workers"] == workers if workers else 1 < p["workers"] < 256
    rng = np.random.default_rng(n + m + FAMILIES.index(fam))
    q, t = fam(rng, n, m)
    dq, dt = slamhip.DeviceDescriptors(ctx, q), slamhip.DeviceDescriptors(ctx, t)
    try:
        mx = search(ctx, dq, n, dt, m, 2)
        valu = search(ctx, dq, n, dt, m, 1)
    finally:
        dq.free()
        dt.free()
    assert same(mx, valu)
    idx, dist = mx
    tie = dist[:, 0] == dist[:, 1]
    want = min(n, 2048, m // 16) if fam is duplicates else n    # the family does what it is for
    assert tie.sum() >= want and (idx[tie, 0] < idx[tie, 1]).all()
    if fam is all_equal:
        assert (idx == np.array([0, 1])).all() and (dist == 0).all()


@pytest.mark.parametrize("fam", [few_values, duplicates], ids=lambda f: f.__name__)
def test_selection_modes_on_ties(gpu_ctx, fam):
    """bf_select fused into the decode: has-a-neighbour and the ratio test (its own ties included: 4 / 8 = 0.5) on tie-heavy rows."""
    import slamhip

    ctx = gpu_ctx
    n, m = 8192 + 37, 65536 + 5
    rng = np.random.default_rng(41 + FAMILIES.index(fam))
    q, t = fam(rng, n, m)
    dq, dt = slamhip.DeviceDescriptors(ctx, q), slamhip.DeviceDescriptors(ctx, t)
    tab = slamhip.Top2Table(ctx, n)
    flags = ctx.malloc(n)
    try:
        for mode, param in ((0, 0.0), (2, 0.5), (2, 0.75)):
            got = {}
            for e in (2, 1):
                with engine(ctx, e):
                    cnt = slamhip.knn2_select_device(ctx, dq.buf, n, dt.buf, m, tab.idx, tab.dist, flags, mode=mode, param=param)
                    got[e] = (cnt, flags.download(np.uint8, (n,)), tab.download())
                assert ctx.state_dirty() == 0
            assert got[2][0] == got[1][0] and np.array_equal(got[2][1], got[1][1]) and same(got[2][2], got[1][2]), (mode, param)
            assert got[2][0] == got[2][1].sum()
    finally:
        for o in (tab, flags, dq, dt):
            o.free()


def test_two_passes_beyond_the_key_range(gpu_ctx):
    """2^23 + 777 tie-heavy rows: two passes in one call (both on the MX kernel with engine 2), copies on both sides of the
    pass boundary; the keys of a pass - and the bound[] of its launch - count rows from the pass's own start."""
    import slamhip

    ctx = gpu_ctx
    n, m = 130, PASS + 777
    rng = np.random.default_rng(23)
    q, t = few_values(rng, n, m)
    t[PASS + 9] = t[5] = q[1] = 0xFF                            # a pair of copies across the passes, far from every other row
    t[PASS] = t[PASS - 1] = q[2] = 0xF0
    p0, tbl0 = plan(ctx, n, PASS)
    assert p0["chunk"] == 1024 and p0["workers"] == 256 and tbl0[-1] == PASS
    dq, dt = slamhip.DeviceDescriptors(ctx, q), slamhip.DeviceDescriptors(ctx, t)
    try:
        for base in (0, 1000003):
            mx = search(ctx, dq, n, dt, m, 2, train_base=base)
            assert same(mx, search(ctx, dq, n, dt, m, 1, train_base=base)), base
            assert mx[0][1].tolist() == [5 + base, PASS + 9 + base] and mx[0][2].tolist() == [PASS - 1 + base, PASS + base]
            assert (mx[1][1:3] == 0).all()
    finally:
        dq.free()
        dt.free()


def test_mixed_traffic_leaves_bound_idle(gpu_ctx):
    """MX and VALU launches in turn on one context: bound[] holds keys during an MX launch and distances during a VALU one,
    and the idle pattern between any two - search() asserts the state idle after every call."""
    import slamhip

    ctx = gpu_ctx
    rng = np.random.default_rng(77)
    shapes = [(8192 + 5, 65536, few_values), (1000, 70001, duplicates), (3000, 40000, all_equal), (8192 + 5, 65536, duplicates)]
    for n, m, fam in shapes:
        q, t = fam(rng, n, m)
        dq, dt = slamhip.DeviceDescriptors(ctx, q), slamhip.DeviceDescriptors(ctx, t)
        try:
            assert plan(ctx, n, m)[0]["auto"] == 1
            tables = [search(ctx, dq, n, dt, m, e) for e in (2, 1, 0, 1, 2)]
        finally:
            dq.free()
            dt.free()
        assert all(same(tables[0], x) for x in tables[1:]), (n, m, fam.__name__)
