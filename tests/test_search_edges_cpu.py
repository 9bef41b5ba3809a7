"""CPU: the descriptor families of tests/hamming_families.py and the shapes of tests/test_search_edges_gpu.py, without a
device.  Every generator's rows really sit |a - b| bits apart; the integer expectations agree with the references the GPU
suites already trust (oracle.bf_knn_c for every k, ref_radius, ref_window); and every shape the GPU file uses reaches the
plan regime it aims at (slamhip.plan_describe_* at 256 CUs), with the planted plateaus on both sides of their boundaries."""
import numpy as np
import pytest

import hamming_families as hf

CU = 256


def families():
    """(name, a, b) over every generator and every query set."""
    rng = np.random.default_rng(1)
    out = [(f"constant {v}", hf.constant(40, v), hf.queries_equal(5)) for v in (0, 1, 255, 256)]
    out += [(f"ladder {kind}", hf.ladder(600, kind), b) for kind in ("asc", "desc", "perm")
            for b in (hf.queries_alternating(7), hf.queries_ramp(300), hf.queries_equal(3, 256))]
    for k in hf.PLATEAU_KS:
        for D in hf.PLATEAU_DS:
            out.append((f"plateau k={k} D={D}", hf.plateau_case(hf.TOPK_M, k, D, 208)[0], hf.queries_alternating(4)))
    out += [("alphabet 2", hf.alphabet(500, (7, 250), rng), hf.queries_ramp(70)),
            ("alphabet 3", hf.alphabet(500, (0, 128, 256), rng), hf.queries_ramp(70))]
    a, b, _ = hf.radius_lengths_case()
    out.append(("lengths", a, b))
    out += [(f"window {kind}", *hf.window_case(kind, 5, 65)) for kind in hf.WINDOW_KINDS]
    return out


FAMILIES = families()


@pytest.mark.parametrize("name,a,b", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_distances_are_what_the_construction_says(name, a, b):
    q, t = hf.prefix_rows(b), hf.prefix_rows(a)
    assert q.dtype == np.uint8 and q.shape == (len(b), 32) and t.shape == (len(a), 32)
    assert np.array_equal(np.bitwise_count(t).sum(1), a) and np.array_equal(np.bitwise_count(q).sum(1), b)
    ub = np.unique(b)                                               # (equal query rows are equal: one of each is enough)
    d = np.bitwise_count(hf.prefix_rows(ub)[:, None, :] ^ t[None, :, :]).sum(-1, dtype=np.int64)
    assert np.array_equal(d, hf.distances(a, ub))


def test_generators_build_what_they_promise():
    assert hf.prefix_rows([0, 1, 8, 9, 256]).tolist() == [[0] * 32, [128] + [0] * 31, [255] + [0] * 31, [255, 128] + [0] * 30, [255] * 32]
    assert sorted(hf.ladder(257, "perm").tolist()) == list(range(257))
    assert hf.ladder(300, "asc")[[0, 256, 257]].tolist() == [0, 256, 0] and hf.ladder(300, "desc")[[0, 256, 257]].tolist() == [256, 0, 256]
    assert hf.queries_alternating(4).tolist() == [0, 256, 0, 256]
    for k in hf.PLATEAU_KS:
        for D in hf.PLATEAU_DS:
            for b0 in (0, 256):
                closer, at = hf.plateau_case(500, k, D, 128)[1]
                d = np.abs(hf.plateau(500, k, D, k + 3, (closer, at), b0=b0) - b0)
                assert (d[at] == D).all() and (d[closer] < D).all() and closer.size == (k - 1 if D else 0)
                rest = np.setdiff1d(np.arange(500), np.r_[closer, at])
                assert (d[rest] > D).all() if D < 256 else (d[rest] == D).all()
                assert closer.size == 0 or (closer.min() < at.min() and closer.max() > at.max() or closer.size == 1)
    a, b, L = hf.radius_lengths_case()
    assert np.array_equal((a[None, :] == b[:, None]).sum(1), L)
    assert sorted(L[sorted(hf.RADIUS_LENGTHS)].tolist()) == [0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 8192, 8193]
    assert set(hf.RADIUS_LENGTHS) >= {0, 1, 254, 255, 256, 257, hf.RADIUS_N - 1}
    for q in (1, 254, 255, 256, 299):                               # a long list takes rows from every 256-row chunk
        assert np.unique(np.flatnonzero(a == b[q]) // 256).size == -(-len(a) // 256)


@pytest.mark.parametrize("name,a,b", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_expected_topk_is_the_c_oracle(built, name, a, b):
    from oracle import oracle

    q, t = hf.prefix_rows(b), hf.prefix_rows(a)
    full = hf.expected_topk(a, b, 32)
    for k in range(1, 33):
        idx, dist = hf.expected_topk(a, b, k)
        ridx, rdist = oracle.bf_knn_c(q, t, k, threads=4)
        assert np.array_equal(idx, ridx) and np.array_equal(dist, rdist), k
        assert np.array_equal(idx, full[0][:, :k]) and np.array_equal(dist, full[1][:, :k]), k     # a shorter list is a prefix


def test_expected_topk_fillers_and_order():
    idx, dist = hf.expected_topk([5, 3, 5], [4, 4], 5)
    assert idx.tolist() == [[0, 1, 2, -1, -1]] * 2 and dist.tolist() == [[1, 1, 1, 2**31 - 1, 2**31 - 1]] * 2
    assert idx.dtype == np.int32 and dist.dtype == np.int32
    idx, dist = hf.expected_window([5, 3, 5, 4], [4], [False, True, True, False], 3)
    assert idx.tolist() == [[1, 2, -1]] and dist.tolist() == [[1, 1, 2**31 - 1]]
    off, idx, dist = hf.expected_radius([5, 3, 4, 9], [4, 9, 100], 2)
    assert off.dtype == np.int64 and off.tolist() == [0, 3, 4, 4] and idx.tolist() == [2, 0, 1, 3] and dist.tolist() == [0, 1, 1, 0]


@pytest.mark.parametrize("name,a,b", [f for f in FAMILIES if len(f[1]) <= 2000], ids=lambda v: v if isinstance(v, str) else "")
def test_expected_radius_is_ref_radius(built, name, a, b):
    q, t = hf.prefix_rows(b), hf.prefix_rows(a)
    radii = {0.0: 1, 1.0: 2, 2.5: 3, 127.5: 128, 255.0: 256, 255.999: 256, 256.0: 257, -1.0: 0}
    want = hf.ref_radius(q, t, tuple(radii))
    for r, th in radii.items():
        got = hf.expected_radius(a, b, th)
        assert got[0].dtype == np.int64 and all(np.array_equal(g, w) for g, w in zip(got, want[r])), r


def test_expected_radius_is_ref_radius_on_the_list_lengths(built):
    a, b, _ = hf.radius_lengths_case()
    q, t = hf.prefix_rows(b), hf.prefix_rows(a)
    want = hf.ref_radius(q, t, tuple(r for r, _ in hf.RADIUS_TH))
    for r, th in hf.RADIUS_TH:
        assert all(np.array_equal(g, w) for g, w in zip(hf.expected_radius(a, b, th), want[r])), r


@pytest.mark.parametrize("kind", hf.WINDOW_KINDS)
def test_expected_window_is_ref_window(built, kind):
    for n, m in ((1, 63), (65, 1025)):
        a, b = hf.window_case(kind, n, m)
        q, t = hf.prefix_rows(b), hf.prefix_rows(a)
        qxy, txy = np.full((n, 2), 5.0, np.float32), np.full((m, 2), 5.0, np.float32)
        inside = np.arange(m) >= m // 2
        outside = txy.copy()
        outside[~inside, 0] = np.nextafter(np.float32(6.0), np.float32(7.0))
        for k in (1, 2):
            for in_window, centres, radius in ((None, txy, 1.0), (inside, txy, np.where(inside, 1.0, -1.0)),
                                               (inside, txy, np.where(inside, 1.0, np.nan)), (inside, outside, 1.0)):
                got, want = hf.expected_window(a, b, in_window, k), hf.ref_window(q, t, qxy, centres, radius, k)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (n, m, k)


# ---- the regimes the GPU shapes aim at ---------------------------------------------------------------------------------

def test_topk_shapes_reach_their_regimes(built):
    import slamhip

    tails = set()
    for n in hf.TOPK_N:
        for k in range(1, 33):
            for m in hf.TOPK_M_SINGLE:
                p = slamhip.plan_describe_topk(n, m, k, num_cu=CU)
                assert p["chunks"] == 1 and p["merge"] == 0 and p["workspace_bytes"] == 0, (n, m, k, p)   # part == null
            for m in hf.TOPK_M_MULTI:
                p = slamhip.plan_describe_topk(n, m, k, num_cu=CU)
                last = m - (p["chunks"] - 1) * p["chunk"]
                assert p["chunks"] >= 4 and p["merge"] == 1 and 0 < last < p["chunk"], (n, m, k, p)       # a shorter last chunk
                tails.add(last % 16)
    assert 15 in tails and {m % 16 for m in hf.TOPK_M_SINGLE + hf.TOPK_M_MULTI} >= {0, 1, 15}
    assert hf.TOPK_M in hf.TOPK_M_MULTI
    assert set(hf.WIDE_KS) == {k for k in range(1, 33) if slamhip.plan_describe_topk(64, 200, k, num_cu=CU)["K"] != k}
    n, m = hf.TOPK_TILE_SHAPE
    for k in (5, 32):
        p = slamhip.plan_describe_topk(n, m, k, num_cu=CU)
        assert p["chunk"] > 256 + k and p["chunks"] >= 2, p


@pytest.mark.parametrize("k", hf.PLATEAU_KS)
def test_plateaus_fall_on_both_sides_of_their_boundaries(built, k):
    import slamhip

    m = hf.TOPK_M
    p = slamhip.plan_describe_topk(65, m, k, num_cu=CU)
    chunk = p["chunk"]
    assert p["chunks"] >= 4 and chunk >= 128 + k and 2 * chunk + k < m, p          # rows 16 and 128 lie inside chunk 0
    for boundary in (16, 128, 256, chunk, 2 * chunk):
        for D in hf.PLATEAU_DS:
            a, (closer, at) = hf.plateau_case(m, k, D, boundary)
            assert at.size == k + 3 and at.min() < boundary <= at.max() and at.max() < m
            assert (at.min() // chunk != at.max() // chunk) == (boundary % chunk == 0)   # a chunk boundary: in two chunks
            want = hf.expected_topk(a, [0], k)
            assert want[1][0, k - 1] == D                                           # the k-th distance is the plateau's
            tied = np.flatnonzero(a == D)
            assert tied.size >= k + 3 and want[0][0, k - 1] == tied[k - 1 - closer.size]   # more ties than places: lowest indices
            if closer.size and boundary >= chunk:
                assert closer.min() < min(chunk, at.min())                               # the plateau lies behind closer rows
    n, m = hf.TOPK_TILE_SHAPE                                                       # row 256 inside one chunk of several tiles
    p = slamhip.plan_describe_topk(n, m, k, num_cu=CU)
    at = hf.plateau_case(m, k, 1, 256)[1][1]
    assert at.min() < 256 <= at.max() < p["chunk"]


def test_radius_shapes_reach_their_regimes(built):
    import slamhip

    a, b, L = hf.radius_lengths_case()
    p = slamhip.plan_describe_radius(len(b), len(a), num_cu=CU)
    assert p["short_max"] == 4096 and p["bins"] == 257 and p["qblocks"] == 2 and p["chunks"] >= 8, p
    short = p["short_max"]
    assert {short - 1, short, short + 1, 2 * short, 2 * short + 1, 0, 1, 2, 63, 64, 65} <= set(L.tolist())
    long = L > short
    assert long[:256].any() and long[256:].any() and not long[257:299].any() and long[299]    # short lists between long ones
    for radius, th in hf.RADIUS_TH + hf.RADIUS_BIN_TH:
        assert slamhip.radius_threshold(radius) == th
    assert slamhip.radius_threshold(255.999) == 256
    # every bin: lists of M entries on the short path, and on the long path at the largest M
    assert [m > short for m in hf.RADIUS_BIN_M] == [False, False, True]
    for m in hf.RADIUS_BIN_M:
        for row in hf.distances(hf.ladder(m, "perm"), [0, 256]):
            assert np.array_equal(np.unique(row), np.arange(257))   # all 257 distances in one list
        assert slamhip.plan_describe_radius(70, m, num_cu=CU)["chunks"] == -(-m // 256)
    assert {m - short for m in hf.RADIUS_CONST_M} >= {0, 1} and {1, 2, 64, 65} <= set(hf.RADIUS_CONST_M)


def test_window_shapes_reach_their_regimes(built):
    import slamhip

    chunks = set()
    for m in hf.WINDOW_M:
        for n in hf.WINDOW_N:
            p = slamhip.plan_describe_window(n, m, num_cu=CU)
            assert p["chunk"] == 1024 and p["queries_per_item"] == 64, p
        chunks.add(-(-m // 1024))
    assert chunks == {1, 2, 3}                                      # one, two and three candidate chunks of one tile
    assert {m % 64 for m in hf.WINDOW_M} >= {63, 0, 1} and {n - 64 for n in hf.WINDOW_N} >= {-1, 0, 1}
    for kind in hf.WINDOW_KINDS:                                    # every level of the window lists is a tie or a known row
        a, b = hf.window_case(kind, 65, 2049)
        idx, dist = hf.expected_window(a, b, None, 2)
        assert (idx >= 0).all() and (dist <= 256).all()
