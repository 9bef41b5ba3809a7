"""The node-constrained search without a device: the numpy reference against a plain double loop on pairs whose
distances are known by construction, the limits and the plan of the library, and the argument errors that are raised before a
context exists."""
import numpy as np
import pytest

import bow_match_ref as R
from hamming_families import prefix_rows


@pytest.fixture(scope="module")
def bm(built):
    from slamhip import bow_match as module
    return module


# ---- the reference against its definition ----------------------------------------------------------------------------------

def tiny_pairs():
    rng = np.random.default_rng(41)
    # prefix rows: the distance of two rows is the difference of their prefix lengths
    yield [10, 20, 30, 40], [0, 0, 1, 1], [12, 31, 19, 45, 10], [0, 1, 0, 1, 0], None, None
    yield [5, 5, 5, 100], [3, 3, 3, 3], [5, 5, 200], [3, 3, 3], None, None                  # duplicates: one side-2 row, three claims
    yield [0, 256, 128], [-1, 7, 2**31 - 1], [1, 255, 127, 64], [7, -1, 2**31 - 1, -1], None, None
    yield [], [], [3], [0], None, None
    yield [3], [0], [], [], None, None
    for _ in range(6):
        n1, n2 = int(rng.integers(1, 14)), int(rng.integers(1, 14))
        yield (rng.integers(0, 257, n1), rng.integers(-1, 3, n1), rng.integers(0, 257, n2), rng.integers(-1, 3, n2),
               rng.integers(0, 32, n1), rng.integers(0, 32, n2))


@pytest.mark.parametrize("th_low,ratio", [(50, 0.75), (256, 10.0), (3, 0.9), (-1, 0.75), (256, 0.0)])
def test_reference_equals_the_double_loop(th_low, ratio):
    for a1, n1, a2, n2, b1, b2 in tiny_pairs():
        d1, d2 = prefix_rows(a1), prefix_rows(a2)
        n1, n2 = np.asarray(n1, np.int64), np.asarray(n2, np.int64)
        for bins in ((None, None), (b1, b2)):
            got = R.search(d1, n1, d2, n2, bins[0], bins[1], th_low, ratio)
            want = R.search_loops(d1, n1, d2, n2, bins[0], bins[1], th_low, ratio)
            assert np.array_equal(got[0], want[0]) and got[1] == want[1]
            assert np.array_equal(got[2][0], want[2][0]) and np.array_equal(got[2][1], want[2][1])


def test_reference_distances_are_the_prefix_differences():
    a1, a2 = [10, 20, 30, 40], [12, 31, 19, 45, 10]
    idx, dist = R.node_top2(prefix_rows(a1), [0, 0, 1, 1], prefix_rows(a2), [0, 1, 0, 1, 0])
    assert idx.tolist() == [[4, 0], [2, 0], [1, 3], [3, 1]] and dist.tolist() == [[0, 2], [1, 8], [1, 15], [5, 9]]
    order, ns = R.group([5, -1, 0, 5, 2**31 - 1, -7, 0])
    assert order.tolist() == [2, 6, 0, 3, 4, 5, 1] and ns.tolist() == [0, 0, 5, 5, 2**31 - 1, -7, -1]


# ---- limits and plan ---------------------------------------------------------------------------------------------------------

def test_limits_agree_with_the_module(bm):
    from slamhip import bow, orb

    lim = bm.limits()
    assert lim["rows_per_image"] == bm.ROWS_MAX == bow.IMAGE_MAX == 8192
    assert lim["pairs_per_call"] == bm.PAIRS_MAX >= 256
    assert lim["bins"] == bm.N_BINS == orb.N_BINS == R.N_BINS and lim["no_second"] == bm.NO_SECOND == R.NO_SECOND
    assert lim["rows_per_image"] <= 1 << 13 < 1 << 23            # the row fields of the claim key and of the distance key
    assert lim["group_threads"] <= 1024 and lim["scan_lanes"] % 64 == 0


def test_plan_fits_the_lds_and_grows_with_the_shape(bm):
    p = bm.plan_describe(256, 8192)
    assert p["sort_length"] == 8192 and p["sort_length"] * 8 <= p["group_lds_bytes"] <= 160 * 1024
    assert p["finish_lds_bytes"] <= 160 * 1024
    assert p["group_blocks"] == 256 and p["finish_blocks"] == 256
    assert p["scan_blocks"] == 256 * (8192 // bm.limits()["scan_lanes"])
    assert bm.plan_describe(1, 5)["sort_length"] == 8 and bm.plan_describe(1, 0)["scan_blocks"] == 0
    assert bm.plan_describe(3, 65)["scan_blocks"] == 3 * 2
    last = -1
    for B in (0, 1, 2, 31, 256, bm.PAIRS_MAX):
        w = bm.plan_describe(B, 2000)["workspace_bytes"]
        assert w >= last
        last = w
    last = -1
    for n in (0, 1, 63, 64, 65, 2000, 8191, 8192):
        w = bm.plan_describe(256, n)["workspace_bytes"]
        assert w >= last
        last = w
    from slamhip import SlamHipError
    for B, n in ((bm.PAIRS_MAX + 1, 10), (1, 8193), (-1, 10), (1, -1)):
        with pytest.raises(SlamHipError):
            bm.plan_describe(B, n)


# ---- errors that need no device ----------------------------------------------------------------------------------------------

def test_argument_errors_are_raised_before_any_context(bm, monkeypatch):
    from slamhip import device

    def no_context(*a, **k):
        raise AssertionError("an invalid call reached the device")

    monkeypatch.setattr(device, "default_context", no_context)
    monkeypatch.setattr(bm, "default_context", no_context)
    d = prefix_rows(np.arange(10))
    nodes = np.zeros(10, np.int32)
    for k in (0, 3, True, 2.0, None):
        with pytest.raises(ValueError):
            bm.node_match_arrays(d, d, nodes, nodes, k=k)
    with pytest.raises(ValueError):
        bm.node_match_arrays(d.astype(np.int32), d, nodes, nodes)              # dtype of the rows
    with pytest.raises(ValueError):
        bm.node_match_arrays(d[:, :16], d, nodes, nodes)                       # shape of the rows
    with pytest.raises(ValueError):
        bm.node_match_arrays(d, d, nodes[:9], nodes)                           # one id per row
    with pytest.raises(ValueError):
        bm.node_match_arrays(d, d, nodes.astype(np.float32), nodes)
    with pytest.raises(ValueError):
        bm.node_match_arrays(d, d, nodes.astype(np.int64) + 2**31, nodes)      # an id beyond 32 bits
    big = np.zeros((bm.ROWS_MAX + 1, 32), np.uint8)
    with pytest.raises(ValueError):
        bm.node_match_arrays(big, d, np.zeros(len(big), np.int32), nodes)      # n > 8192
    with pytest.raises(ValueError):
        bm.FeatureVectors.from_nodes(big, np.zeros(len(big), np.int32))
    with pytest.raises(ValueError):
        bm.FeatureVectors.from_nodes(d, nodes, offsets=[0, 4, 3, 10])          # offsets that descend
    with pytest.raises(ValueError):
        bm.FeatureVectors.from_nodes(d, nodes, offsets=[0, 4])                 # offsets that do not end at n
    with pytest.raises(ValueError):
        bm.node_match_arrays(d, d, nodes, nodes, scan_order=2)


def test_search_argument_errors_need_no_launch(bm):
    off = np.array([0, 4, 10], np.int64)
    fv1, fv2 = bm.FeatureVectors(None, off, None), bm.FeatureVectors(None, off[:2].copy(), None)      # never reaches the device
    ok_bins1, ok_bins2 = np.zeros(10, np.int64), np.zeros(4, np.int64)
    bad = [
        dict(pairs=[(0, 1)]), dict(pairs=[(2, 0)]), dict(pairs=[(-1, 0)]), dict(pairs=[0, 0]), dict(pairs=[(0.0, 0.0)]),
        dict(pairs=np.zeros((bm.PAIRS_MAX + 1, 2), np.int64)),
        dict(pairs=[(0, 0)], bins1=ok_bins1), dict(pairs=[(0, 0)], bins2=ok_bins2),
        dict(pairs=[(0, 0)], bins1=ok_bins1 + 32, bins2=ok_bins2), dict(pairs=[(0, 0)], bins1=ok_bins1, bins2=ok_bins2 - 1),
        dict(pairs=[(0, 0)], bins1=ok_bins1[:9], bins2=ok_bins2), dict(pairs=[(0, 0)], bins1=ok_bins1 * 1.0, bins2=ok_bins2),
        dict(pairs=[(0, 0)], th_low=1.5), dict(pairs=[(0, 0)], ratio=float("nan")), dict(pairs=[(0, 0)], scan_order=3),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            bm.search_by_bow(fv1, fv2, **kw)
    with pytest.raises(ValueError):
        bm.search_by_bow(fv1, "not feature vectors", [(0, 0)])
    with pytest.raises(ValueError):
        bm.node_top2(fv1, fv2, [(1, 1)])
    assert bm.search_by_bow(fv1, fv2, np.zeros((0, 2), np.int64))[0] == []       # no pairs: nothing to do, no device either
