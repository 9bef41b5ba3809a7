"""GPU: the top-k, radius and window searches (bf_topk.hip, bf_radius.hip, bf_window.hip) on descriptor sets whose distances
are known by construction (tests/hamming_families.py): distance 0 and 256, every k, train sets that make every row or no row
enter a list, plateaus of ties across the 16-row group, the 128 cold rows, row 256 and the chunk boundaries, waves whose
lanes disagree, radius lists of every length at the edges of the counting sort with long and short lists mixed over two
query blocks, every distance bin at once, and window searches whose tie order is decided by the index alone over several
candidate chunks.

Every result is compared bit for bit, over all rows, with the integer expectation (a sort of |a - b| by (distance, index));
every call must leave the merge state idle.  Cases that aim at a plan regime take it from plan_describe_* with the
context's CU count and assert that it is reached (tests/test_search_edges_cpu.py checks the same at 256 CUs)."""
import numpy as np
import pytest

import hamming_families as hf
from test_radius_gpu import Csr, assert_csr
from test_topk_gpu import Tables
from test_window_gpu import run_device

pytestmark = pytest.mark.gpu


def cus(ctx, n, m):
    return ctx.plan_info(n, m)["cus"]


def assert_tables(got, want, what):
    """(idx, dist) against the expectation; names the first differing row as test_topk_gpu.assert_oracle does."""
    idx, dist = got
    ridx, rdist = want
    assert idx.shape == ridx.shape and dist.shape == rdist.shape and idx.dtype == np.int32 and dist.dtype == np.int32, what
    bad = np.nonzero((idx != ridx).any(1) | (dist != rdist).any(1))[0]
    assert bad.size == 0, f"{what}: {bad.size} rows differ, first {bad[0]}: {idx[bad[0]]} {dist[bad[0]]} vs {ridx[bad[0]]} {rdist[bad[0]]}"


def with_base(idx, base):
    return np.where(idx >= 0, idx + base, idx).astype(np.int32)


class TopkPair:
    """One query / train pair on the device and on the host: both entry points for any k, each against the expectation
    (computed once for k = 32; a shorter list is its prefix)."""

    BASE = 4242

    def __init__(self, ctx, a, b):
        import slamhip

        self.ctx, self.a, self.b = ctx, a, b
        self.q, self.t = hf.prefix_rows(b), hf.prefix_rows(a)
        self.want = hf.expected_topk(a, b, 32)
        self.dq, self.dt = slamhip.DeviceDescriptors(ctx, self.q), slamhip.DeviceDescriptors(ctx, self.t)

    def check(self, k, what, host=True):
        import slamhip

        n, m = self.q.shape[0], self.t.shape[0]
        want = (np.ascontiguousarray(self.want[0][:, :k]), np.ascontiguousarray(self.want[1][:, :k]))
        if host:
            assert_tables(slamhip.topk_match_arrays(self.q, self.t, k, ctx=self.ctx), want, f"{what} k={k} host")
            assert self.ctx.state_dirty() == 0, what
        tab = Tables(self.ctx, n, k)
        try:
            slamhip.knn_topk_device(self.ctx, self.dq.buf, n, self.dt.buf, m, k, tab.idx, tab.dist, train_base=self.BASE)
            got = tab.download()
        finally:
            tab.free()
        assert self.ctx.state_dirty() == 0, what
        assert_tables(got, (with_base(want[0], self.BASE), want[1]), f"{what} k={k} device")
        return want

    def free(self):
        self.dq.free()
        self.dt.free()


def topk_check(ctx, a, b, ks, what, host=True):
    pair = TopkPair(ctx, a, b)
    try:
        return [pair.check(k, what, host) for k in ks]
    finally:
        pair.free()


# ---- top-k -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", hf.TOPK_N)
def test_topk_every_k(gpu_ctx, n):
    import slamhip

    for m in hf.TOPK_M_SINGLE + hf.TOPK_M_MULTI:
        plan = slamhip.plan_describe_topk(n, m, 32, num_cu=cus(gpu_ctx, n, m))
        assert (plan["chunks"] == 1) == (m <= 256) and (m <= 256 or plan["chunks"] >= 4), plan
        topk_check(gpu_ctx, hf.ladder(m, "perm"), hf.queries_ramp(n), range(1, 33), f"every k {n}x{m}")


@pytest.mark.parametrize("v", [0, 256])
def test_topk_constants(gpu_ctx, v):
    for n, m in ((65, 1), (65, 5), (65, 31), (257, 256), (65, hf.TOPK_M)):
        want = topk_check(gpu_ctx, hf.constant(m, v), hf.queries_equal(n), (1, 3, 6, 17, 32), f"constant {v} {n}x{m}")
        idx, dist = want[-1]                                        # the expectation itself, stated by hand for k = 32
        kk = min(32, m)
        assert (idx[:, :kk] == np.arange(kk)).all() and (dist[:, :kk] == v).all()
        assert (idx[:, kk:] == hf.NONE_IDX).all() and (dist[:, kk:] == hf.NONE_DIST).all()


@pytest.mark.parametrize("m", [200, hf.TOPK_M])
def test_topk_query_equal_to_train_row_0(gpu_ctx, m):
    """Key 0 (distance 0 at train row 0) next to the pad slots pinned to key 0, for every k on a wider instantiation."""
    a = hf.ladder(m, "perm")
    b = np.r_[a[0], hf.queries_ramp(64)]                           # query 0 is train row 0; the others are not
    for want in topk_check(gpu_ctx, a, b, hf.WIDE_KS, f"key 0 M={m}"):
        assert want[0][0, 0] == 0 and want[1][0, 0] == 0
    a0 = np.r_[0, 1 + hf.ladder(m - 1, "asc") % 256]               # the only row at distance 0 from the value 0 is row 0
    for want in topk_check(gpu_ctx, a0, hf.queries_equal(65), hf.WIDE_KS, f"key 0 alone M={m}"):
        assert (want[0][:, 0] == 0).all() and (want[1][:, 0] == 0).all()


@pytest.mark.parametrize("kind", ["asc", "desc", "perm"])
@pytest.mark.parametrize("queries", ["alternating", "ramp"])
def test_topk_ladders(gpu_ctx, kind, queries):
    import slamhip

    n, m = 130, hf.TOPK_M
    assert slamhip.plan_describe_topk(n, m, 32, num_cu=cus(gpu_ctx, n, m))["chunks"] >= 4
    b = hf.queries_alternating(n) if queries == "alternating" else hf.queries_ramp(n)
    topk_check(gpu_ctx, hf.ladder(m, kind), b, (1, 2, 3, 5, 8, 13, 17, 31, 32), f"ladder {kind} {queries}")
    topk_check(gpu_ctx, hf.ladder(256, kind), b, (1, 5, 17, 32), f"ladder {kind} {queries} one chunk")


@pytest.mark.parametrize("k", hf.PLATEAU_KS)
def test_topk_plateaus(gpu_ctx, k):
    import slamhip

    n, m = 65, hf.TOPK_M
    plan = slamhip.plan_describe_topk(n, m, k, num_cu=cus(gpu_ctx, n, m))
    chunk = plan["chunk"]
    assert plan["chunks"] >= 4 and chunk < m // 2, plan
    for boundary in (16, 128, 256, chunk, 2 * chunk):
        for D in hf.PLATEAU_DS:
            a, (closer, at) = hf.plateau_case(m, k, D, boundary)
            assert at.min() < boundary <= at.max()
            for b in (hf.queries_equal(n), hf.queries_alternating(n)):
                (want,) = topk_check(gpu_ctx, a, b, (k,), f"plateau at {boundary} D={D}", host=boundary == chunk)
                if D > 0:                                           # the k-th entry of a query of value 0 is the plateau's first row
                    assert want[0][0, k - 1] == (at.min() if D < 256 else np.setdiff1d(np.arange(m), closer)[0])
                    assert want[1][0, k - 1] == D


def test_topk_plateau_across_a_tile_inside_one_chunk(gpu_ctx):
    """So many query blocks that the chunks span several 256-row tiles: a plateau across row 256 then lies inside one chunk."""
    import slamhip

    n, m = hf.TOPK_TILE_SHAPE
    for k in (5, 32):
        plan = slamhip.plan_describe_topk(n, m, k, num_cu=cus(gpu_ctx, n, m))
        assert plan["chunk"] > 256 + k and plan["chunks"] >= 2, plan
        for D in (1, 128):
            a, _ = hf.plateau_case(m, k, D, 256)
            topk_check(gpu_ctx, a, hf.queries_alternating(n), (k,), f"tile plateau k={k} D={D}", host=False)


@pytest.mark.parametrize("values", [(7, 250), (0, 128, 256)])
def test_topk_alphabet(gpu_ctx, values):
    rng = np.random.default_rng(len(values))
    for n, m in ((257, hf.TOPK_M), (65, 255)):
        topk_check(gpu_ctx, hf.alphabet(m, values, rng), hf.queries_ramp(n), (1, 2, 5, 8, 17, 32), f"alphabet {values} {n}x{m}")


@pytest.mark.parametrize("sizes", [(1029,), (300, 729), (0, 1029), (5, 0, 300, 1, 17, 256, 200, 16, 234)])
def test_topk_merge_of_expected_parts(gpu_ctx, sizes):
    n, m = 130, sum(sizes)
    a, b = hf.ladder(m, "perm"), hf.queries_ramp(n)
    offs = np.r_[0, np.cumsum(sizes)]
    for k in (1, 3, 8, 17, 32):
        parts = [hf.expected_topk(a[lo:hi], b, k) for lo, hi in zip(offs[:-1], offs[1:])]
        pi = np.ascontiguousarray(np.stack([with_base(p[0], lo) for p, lo in zip(parts, offs)]), np.int32)
        pd = np.ascontiguousarray(np.stack([p[1] for p in parts]), np.int32)
        d_pi, d_pd = gpu_ctx.upload(pi), gpu_ctx.upload(pd)
        tab = Tables(gpu_ctx, n, k)
        try:
            assert gpu_ctx.lib.slam_bf_merge_topk(gpu_ctx.handle, d_pi.ptr, d_pd.ptr, len(sizes), n, k, tab.idx.ptr, tab.dist.ptr) == 0
            got = tab.download()
        finally:
            for o in (tab, d_pi, d_pd):
                o.free()
        assert gpu_ctx.state_dirty() == 0
        assert_tables(got, hf.expected_topk(a, b, k), f"merge of {len(sizes)} parts k={k}")


# ---- radius ----------------------------------------------------------------------------------------------------------------

def radius_check(ctx, a, b, radius, th, what, q=None, t=None):
    import slamhip

    q = hf.prefix_rows(b) if q is None else q
    t = hf.prefix_rows(a) if t is None else t
    want = hf.expected_radius(a, b, th)
    assert_csr(slamhip.radius_match_arrays(q, t, radius, ctx=ctx), want, what)
    assert ctx.state_dirty() == 0, what
    return want


@pytest.fixture(scope="module")
def lengths_case():
    a, b, L = hf.radius_lengths_case()
    return a, b, L, hf.prefix_rows(b), hf.prefix_rows(a)


@pytest.mark.parametrize("radius,th", hf.RADIUS_TH)
def test_radius_list_lengths(gpu_ctx, lengths_case, radius, th):
    import slamhip

    a, b, L, q, t = lengths_case
    plan = slamhip.plan_describe_radius(len(b), len(a), num_cu=cus(gpu_ctx, len(b), len(a)))
    assert plan["qblocks"] == 2 and plan["chunks"] >= 8 and plan["short_max"] == 4096, plan
    off, _, _ = radius_check(gpu_ctx, a, b, radius, th, f"lengths r={radius}", q, t)
    got = np.diff(off)
    long = got > plan["short_max"]
    if th == 1:
        assert np.array_equal(got, L) and not long[257:299].any()  # short lists between the long ones of the second block
    else:                                                           # the same rows, two or three adjacent bins: longer lists
        assert (got >= L).all() and (got > L).sum() > len(L) // 2
    for block in (long[:256], long[256:]):                          # long and short lists in both query blocks
        assert block.any() and not block.all()


def test_radius_device_path_with_a_train_base_and_the_capacity_protocol(gpu_ctx, lengths_case):
    import slamhip

    a, b, L, q, t = lengths_case
    n, m, base = len(b), len(a), 1 << 20
    want = hf.expected_radius(a, b, 1)
    total = int(want[0][-1])
    dq, dt = slamhip.DeviceDescriptors(gpu_ctx, q), slamhip.DeviceDescriptors(gpu_ctx, t)
    small, big = Csr(gpu_ctx, n, 0), Csr(gpu_ctx, n, total)
    try:
        assert slamhip.radius_device(gpu_ctx, dq.buf, n, dt.buf, m, 0.0, small.off, 0, None, None, train_base=base) == total
        assert np.array_equal(small.download(0)[0], want[0])       # too small: the exact total and the offsets, nothing else
        assert gpu_ctx.state_dirty() == 0
        assert slamhip.radius_device(gpu_ctx, dq.buf, n, dt.buf, m, 0.0, big.off, total, big.idx, big.dist, train_base=base) == total
        got = big.download(total)
        assert gpu_ctx.state_dirty() == 0
    finally:
        for o in (small, big, dq, dt):
            o.free()
    assert_csr(got, (want[0], want[1] + base, want[2]), "device path")


@pytest.mark.parametrize("m", hf.RADIUS_BIN_M)
def test_radius_every_bin(gpu_ctx, m):
    a = hf.ladder(m, "perm")
    b = np.r_[hf.queries_equal(3, 0), hf.queries_equal(3, 256), hf.queries_alternating(64)]
    for radius, th in hf.RADIUS_BIN_TH:
        off, idx, dist = radius_check(gpu_ctx, a, b, radius, th, f"every bin M={m} r={radius}")
        if th == 257:                                               # all 257 distances in every list, each m // 257 times or once more
            assert (np.diff(off) == m).all()
            assert np.array_equal(np.unique(dist[:m]), np.arange(257))
    for kind in ("asc", "desc"):
        radius_check(gpu_ctx, hf.ladder(m, kind), b, 256.0, 257, f"every bin {kind} M={m}")


def test_radius_one_bin(gpu_ctx):
    n = 70
    for m in hf.RADIUS_CONST_M:
        off, _, dist = radius_check(gpu_ctx, hf.constant(m, 0), hf.queries_equal(n), 0.0, 1, f"constant 0 M={m}")
        assert (np.diff(off) == m).all() and not dist.any()
    for m in (65, 4097):
        off, _, dist = radius_check(gpu_ctx, hf.constant(m, 256), hf.queries_equal(n), 256.0, 257, f"constant 256 M={m}")
        assert (np.diff(off) == m).all() and (dist == 256).all()
        off, _, _ = radius_check(gpu_ctx, hf.constant(m, 256), hf.queries_equal(n), 255.999, 256, f"constant 256 below M={m}")
        assert off[-1] == 0


# ---- window ----------------------------------------------------------------------------------------------------------------

CENTRE = np.array([5.0, 5.0], np.float32)


def window_check(ctx, a, b, in_window, txy, radius, what, cells=(0,)):
    """Host and device paths for k = 1 and 2, every cell cap, against the expectation over the in-window rows."""
    import slamhip

    n, m = len(b), len(a)
    q, t = hf.prefix_rows(b), hf.prefix_rows(a)
    qxy = np.tile(CENTRE, (n, 1))
    for k in (1, 2):
        want = hf.expected_window(a, b, in_window, k)
        for c in cells:
            assert_tables(slamhip.window_match_arrays(q, t, qxy, txy, radius, k, ctx=ctx, cells=c), want, f"{what} k={k} cells={c} host")
            assert ctx.state_dirty() == 0
            assert_tables(run_device(ctx, q, t, qxy, txy, radius, k, cells=c), want, f"{what} k={k} cells={c} device")
            assert ctx.state_dirty() == 0
    return want


@pytest.mark.parametrize("m", hf.WINDOW_M)
def test_window_one_cell(gpu_ctx, m):
    """All centres at one point: one cell, every row a candidate of every query, ties decided by the index alone."""
    import slamhip

    txy = np.tile(CENTRE, (m, 1))
    for n in hf.WINDOW_N:
        assert slamhip.plan_describe_window(n, m, num_cu=cus(gpu_ctx, n, m))["chunk"] == 1024
        for kind in hf.WINDOW_KINDS:
            a, b = hf.window_case(kind, n, m)
            idx, dist = window_check(gpu_ctx, a, b, None, txy, 1.0, f"one cell {kind} {n}x{m}")
            if kind.startswith("const"):
                assert (idx == [0, 1]).all() and (dist == int(kind[5:])).all()
            if kind == "plateau3":
                assert (idx == [m // 3, 1]).all() and (dist == [0, 5]).all()


@pytest.mark.parametrize("how", ["negative", "nan", "outside"])
@pytest.mark.parametrize("m", [65, 1025, 2049])
def test_window_half_excluded(gpu_ctx, how, m):
    """The lower half of the indices is out of every window: the winners are the two lowest IN-WINDOW indices."""
    inside = np.arange(m) >= m // 2
    txy = np.tile(CENTRE, (m, 1))
    radius = np.ones(m, np.float32)
    if how == "negative":
        radius[~inside] = -1.0
    elif how == "nan":
        radius[~inside] = np.nan
    else:
        txy[~inside, 0] = np.nextafter(np.float32(6.0), np.float32(7.0))     # |5 - x| is just above the radius 1
        assert (np.abs(CENTRE[0] - txy[~inside, 0]) > radius[~inside]).all()
    for n in (1, 65, 130):
        for kind in hf.WINDOW_KINDS:
            a, b = hf.window_case(kind, n, m)
            idx, dist = window_check(gpu_ctx, a, b, inside, txy, radius, f"half excluded ({how}) {kind} {n}x{m}")
            if kind.startswith("const"):
                assert (idx == [m // 2, m // 2 + 1]).all() and (dist == int(kind[5:])).all()


def test_window_any_grid(gpu_ctx):
    n, m = 130, 2049
    txy = np.tile(CENTRE, (m, 1))
    for kind in ("alphabet3", "plateau3", "const256"):
        a, b = hf.window_case(kind, n, m)
        window_check(gpu_ctx, a, b, None, txy, 1.0, f"any grid {kind}", cells=(0, 1, 4, 37))
    # the centres spread over many cells, every radius wide enough to hold every query: still every row a candidate
    rng = np.random.default_rng(3)
    txy = (CENTRE + rng.uniform(-40, 40, (m, 2))).astype(np.float32)
    a, b = hf.window_case("alphabet2", n, m)
    window_check(gpu_ctx, a, b, None, txy, 64.0, "any grid spread", cells=(0, 1, 4, 37))
