"""tests/covis_edge_cases.py without a device: every case has, through ``covis.plan`` and ``covis.limits``, the property it
exists for; the brute-force statement equals slamhip.covisibility on the masked cases; and the closed-form tables of the hub
construction equal the brute force at small sizes, so that the expectation of the large ones does not rest on the code under
test."""
import numpy as np
import pytest

import covis_edge_cases as X
from covis_ref import covisibility_ref, same_tables


def _plan(K, L, O, P):
    from slamhip import covis

    return covis.plan(K, L, O, P)


def _obs_digits(case, bits):
    """The distinct values of every 8-bit digit of the observation keys (point, fixed, pose)."""
    K, L, op, ol, fixed = case
    pb = X.bitlen(K - 1)
    key = ol.astype(np.int64) << (pb + 1) | fixed[op].astype(np.int64) << pb | op
    return [len(np.unique(key >> s & 255)) for s in range(0, bits, 8)]


def test_scan_levels_around_the_square_of_a_scan_tile(built):
    S = X.limits()["scan_tile"] ** 2
    assert [X.scan_levels(n) for n in (1, X.limits()["scan_tile"], X.limits()["scan_tile"] + 1, S - 1, S, S + 1)] == [1, 1, 2, 2, 2, 3]


def test_the_issue_s_table_of_key_widths(built):
    """The figures derived by hand from cv_lay for 8-bit digits and 32-bit pair keys up to K = 65 536 (which
    tests/test_covis_cpu.py holds the library to)."""
    assert {n: v[2:] for n, v in X.width_sizes().items()} == {
        "K65536-L16383": (31, 4, 4, 32, 4, 4), "K65536-L32767": (32, 4, 4, 32, 4, 4), "K65536-L32768": (33, 8, 5, 32, 4, 4),
        "K65537-L16383": (32, 4, 4, 33, 8, 5), "K65537-L16384": (33, 8, 5, 33, 8, 5), "K16777216-L1048576": (46, 8, 6, 48, 8, 6)}


@pytest.mark.parametrize("name", list(X.width_sizes()))
def test_width_cases_have_the_property_they_exist_for(built, name):
    from slamhip import covisibility

    K, L, obits, obytes, opasses, pbits, pbytes, ppasses = X.width_sizes()[name]
    case = X.width_case(name)
    _, _, op, ol, fixed = case
    tile = X.limits()["sort_tile"]
    for on in (True, False):
        want = X.expected(name, case, on)
        P, p = len(want[3]), _plan(K, L, len(op), len(want[3]))
        assert (p["obs_key_bits"], p["obs_key_bytes"], p["obs_passes"]) == (obits, obytes, opasses), p
        assert (p["pair_key_bits"], p["pair_key_bytes"], p["pair_passes"]) == (pbits, pbytes, ppasses), p
        assert p["obs_tiles"] > 2 and p["pair_tiles"] > 1 and P > tile and len(op) > 2 * tile
        e = want[0].astype(np.int64)
        assert (e[0].tolist(), e[-1].tolist()) == ([0, 1], [K - 2, K - 1]) and (e[:, 0] * K + e[:, 1]).max() == K * K - K - 1
    assert same_tables(X.expected(name, case, True), covisibility(op, ol, K, fixed, L))
    # every digit of every pass varies; both ends of both ranges are there; points at both ends are unobserved
    # (where L is a power of two only the key of an entry out of range, L << (pb + 1), has the top bit: at 33 bits the fifth
    # pass sees one digit until such an entry is there - test_entries_out_of_range_are_counted_and_refused)
    top = _obs_digits(case, obits)[-1]
    assert min(_obs_digits(case, obits)[:-1]) > 64 and (top > 1 if L & (L - 1) or obits % 8 != 1 else top == 1)
    assert (op.min(), op.max()) == (0, K - 1) and 2 <= ol.min() < L // 100 and L - L // 100 < ol.max() <= L - 3
    only_fixed = [l for l in np.unique(ol[fixed[op]]) if fixed[op[ol == l]].all() and (ol == l).sum() > 1]
    assert only_fixed and fixed.any() and not fixed.all()
    lengths = np.bincount(np.unique(ol, return_inverse=True)[1])
    assert ((lengths >= 2) & (lengths <= 4)).sum() >= X.WIDTH_LONG_TRACKS and lengths.max() == 4


def test_entries_out_of_range_leave_the_valid_ones_as_they_were(built):
    case = X.width_case("K65537-L16384")
    (K, L, op, ol, fixed), n = X.with_bad_entries(case, 5)
    bad = (op < 0) | (op >= K) | (ol < 0) | (ol >= L)
    assert n == bad.sum() == 24 and np.array_equal(op[~bad], case[2]) and np.array_equal(ol[~bad], case[3])
    assert {-1, K, 1 << 30} <= set(op[bad].tolist()) and {-1, L, 1 << 30} <= set(ol[bad].tolist())
    assert np.flatnonzero(bad).min() < X.limits()["sort_tile"] < 2 * X.limits()["sort_tile"] < np.flatnonzero(bad).max()


@pytest.mark.parametrize("name", list(X.pair_key_sizes()))
def test_pair_key_cases_have_the_property_they_exist_for(built, name):
    from slamhip import covisibility

    K, P = X.pair_key_sizes()[name]
    (_, L, op, ol, fixed), facts = X.pair_key_case(name)
    tile = X.limits()["sort_tile"]
    p = _plan(K, L, len(op), P)
    assert (p["pair_key_bytes"], p["pair_passes"], p["pair_tiles"]) == (8, 5 if K == 70000 else 6, -(-P // tile)), p
    assert p["obs_key_bytes"] == (4 if K == 70000 else 8) and L == P and len(op) == 2 * P
    for on in (True, False):
        edges, weights, ptr, pa, pb = X.expected(name, (K, L, op, ol, fixed), on)
        assert len(pa) == P                                         # the fixed pose sees nothing: P pairs with the mask too
        e = edges.tolist()
        assert e[0] == [0, 1] and e[-1] == [K - 2, K - 1] and [0, K - 1] in e
        at = e.index(list(facts["long_edge"]))
        assert weights[at] == X.LONG_RUN and ptr[at] == facts["first"]
        assert (np.diff(ol[pa[ptr[at]:ptr[at + 1]]]) > 0).all()     # inside the edge the pairs ascend in the point
        assert len(np.unique(edges[:, 0] >> 8)) > 100               # the upper digits of the key vary
    # the long run crosses the tile boundary of the sorted order wherever enough other pairs exist to put in front of it:
    # with P <= tile + 1 there are at most tile - 2 999 others and (K-2, K-1) is behind every run, so no placement crosses
    assert facts["crosses"] == (P > tile + 1)
    assert same_tables(X.expected(name, (K, L, op, ol, fixed), True), covisibility(op, ol, K, fixed, L))


@pytest.mark.parametrize("n, extra, hub_point", [(40, 30, None), (40, 30, 0), (40, 30, 30), (2, 0, None), (3, 1, 1), (9, 50, 7)])
def test_hub_tables_in_closed_form_equal_the_brute_force(built, n, extra, hub_point):
    from slamhip import covisibility

    case, tables = X.hub_case(n, extra, 60 + n, hub_point)
    K, L, op, ol, fixed = case
    assert (K, L, len(op)) == (n + 1, extra + 1, n + 2 * extra) and len(tables[3]) == n * (n - 1) // 2 + extra
    assert same_tables(tables, covisibility_ref(op, ol, K, fixed)) and same_tables(tables, covisibility_ref(op, ol, K))
    assert same_tables(tables, covisibility(op, ol, K, fixed, L))
    if extra > 1:
        assert tables[1].max() >= 3 and tables[1][-1] == 1 and len(tables[0]) < len(tables[3])


def test_hub_sizes_reach_the_third_scan_level(built):
    lim = X.limits()
    S, n = lim["scan_tile"] ** 2, X.hub_size()
    assert n * (n - 1) // 2 < S - 1 <= (n + 1) * n // 2
    assert (n, n * (n - 1) // 2) == (2896, 4191960) or lim["scan_tile"] != 2048
    levels = []
    for P in X.hub_pairs_sizes():
        extra = P - n * (n - 1) // 2
        p = _plan(n + 1, extra + 1, n + 2 * extra, P)
        assert 0 < extra < 2 * n and (p["pair_key_bytes"], p["pair_passes"], p["pair_tiles"]) == (4, 3, -(-P // lim["sort_tile"])), p
        assert X.scan_levels(p["pair_tiles"] << lim["digit_bits"]) == 2         # the digit counts of a sort pass: two levels
        levels.append(X.scan_levels(P))                                         # the ranks of the run heads
    assert X.hub_pairs_sizes() == (S - 1, S, S + 1, S + lim["scan_tile"] + 1) and levels == [2, 2, 3, 3]
    assert n > 9 * 300                                                          # the list: nine times the longest before


@pytest.mark.parametrize("which", [0, 1, 2])
def test_points_cases_have_the_property_they_exist_for(built, which):
    from slamhip import covisibility

    lim = X.limits()
    S, L = lim["scan_tile"] ** 2, X.points_sizes()[which]
    assert X.points_sizes() == (S - 1, S, S + lim["scan_tile"] + 2)
    assert X.scan_levels(L + 1) == (2, 3, 3)[which]                  # the pair scan over L + 1 entries: two levels, then three
    K, _, op, ol, fixed = case = X.points_case(L)
    assert K == 5 and X.POINT_TRACKS <= len(np.unique(ol)) < X.POINT_TRACKS + 8 and (ol.min(), ol.max()) == (0, L - 1)
    for on in (True, False):
        edges, weights, ptr, pa, pb = X.expected(("points", L), case, on)
        assert ol[pa].min() == 0 and ol[pa].max() == L - 1 and len(pa) > X.POINT_TRACKS // 2
    if which == 2:                                                   # pairs on both sides of the tile boundaries past S
        seen = set(ol[X.expected(("points", L), case, True)[3]].tolist())
        assert {S - 1, S, S + 1, S + lim["scan_tile"] - 1, S + lim["scan_tile"], L - 1} <= seen
    assert same_tables(X.expected(("points", L), case, True), covisibility(op, ol, K, fixed, L))


def test_large_map_has_long_unobserved_runs_at_both_ends(built):
    from slamhip import MapObservations

    K, offsets, obs = X.large_map()
    M, ends = X.MAP_POINTS, X.MAP_EMPTY_ENDS
    assert (M, ends) == (200000, 70000) and len(offsets) == M + 1
    counts = np.diff(offsets)
    assert not counts[:ends].any() and not counts[M - ends:].any() and counts[ends] == 3 and counts[M - ends - 1] == 2
    assert sorted(set(counts[ends:M - ends].tolist())) == list(range(7)) and offsets[-1] == len(obs) > 150000
    mo = MapObservations.from_arrays(offsets, obs)                    # refuses lists that do not ascend strictly
    assert len(mo) == M and mo.nnz == len(obs) and obs[:, 0].max() == K - 1
