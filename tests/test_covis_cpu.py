"""The covisibility graph without a device: the brute-force statement (tests/covis_ref.py) against slamhip.covisibility on every
masked case of tests/covis_cases.py, CovisibilityGraph on graphs whose answers are written out here, and the host-only entries
of csrc/covis.hip."""
import ctypes

import numpy as np
import pytest

import covis_cases as C
from covis_ref import covisibility_ref, same_tables


@pytest.fixture(scope="module")
def lib(built):
    import slamhip

    return slamhip.load()


@pytest.mark.parametrize("name", C.names(masked=True))
def test_reference_equals_host_function(built, name):
    from slamhip import covisibility

    K, L, op, ol, fixed = C.cases()[name]
    want = covisibility(op, ol, K, fixed, L)
    got = covisibility_ref(op, ol, K, fixed)
    assert same_tables(got, want)
    assert want[2][-1] == len(want[3]) == len(want[4]) and (np.diff(want[2]) == want[1]).all()


def test_cases_have_the_property_they_exist_for(built):
    c, lim = C.cases(), C.limits()
    pairs = lambda n: len(covisibility_ref(*[c[n][i] for i in (2, 3, 0, 4)])[3])
    edges = lambda n: len(covisibility_ref(*[c[n][i] for i in (2, 3, 0, 4)])[0])
    assert len(c["empty"][2]) == 0 and len(c["one-observation"][2]) == 1 and c["one-pose"][0] == 1
    assert (edges("two-poses-nomask"), pairs("two-poses-nomask")) == (1, 1) == (edges("two-free-poses"), pairs("two-free-poses"))
    assert pairs("seen-once") == 0 == pairs("seen-once-nomask") and pairs("all-but-one-fixed") == 0 < pairs("all-but-one-fixed-nomask")
    assert pairs("hub300-nomask") == 44850 and pairs("hub300") == 299 * 298 // 2 > lim["threads"]
    assert c["gaps"][1] > c["gaps"][3].max() + 1 and len(np.unique(c["gaps"][3])) < c["gaps"][1] // 2
    for n in (lim["sort_tile"], lim["scan_tile"]):
        for P in (n - 1, n, n + 1):
            assert pairs(f"pairs-{P}") == P == pairs(f"pairs-{P}-nomask")
    for extra in (-1, 0, 1):
        assert len(c[f"observations-{lim['sort_tile'] + extra}"][2]) == lim["sort_tile"] + extra
    for K in (16, 17, 255, 256, 257, 65536, 70000):
        e = covisibility_ref(*[c[f"K{K}-nomask"][i] for i in (2, 3, 0, 4)])[0].astype(np.int64)
        assert c[f"K{K}"][0] == K and len(e)
        if K < 1000:
            assert (e[:, 0] * K + e[:, 1]).max() == (K - 2) * K + K - 1            # the largest key a graph of K poses has
        else:
            key = e[:, 0] * K + e[:, 1]                                             # the top of 32 bits at 65 536, past them at 70 000
            assert (2 ** 31 < key.min() and key.max() < 2 ** 32) if K == 65536 else key.min() > 2 ** 32
            assert len(c[f"K{K}"][2]) == 120
    assert covisibility_ref(*[c["long-edge"][i] for i in (2, 3, 0, 4)])[1].max() >= 5000
    assert edges("configs4-scaled-nomask") == 780 and pairs("configs4-scaled-nomask") == 1500 * 66
    assert np.array_equal(c["gaps-sorted"][3], np.sort(c["gaps-sorted"][3]))


# ---- CovisibilityGraph: the answers are written out -------------------------------------------------------------------------
#   0 --7-- 1 --7-- 2      3 --2-- 4        vertex 5 alone
#   0 --3-- 2   1 --9-- 6   2 --7-- 6   0 --7-- 6
TWO_PARTS = ([(0, 1), (0, 2), (0, 6), (1, 2), (1, 6), (2, 6), (3, 4)], [7, 3, 7, 7, 9, 7, 2])


def _graph(K, edges, weights):
    from slamhip import CovisibilityGraph

    return CovisibilityGraph(K, np.array(edges).reshape(-1, 2), weights)


def test_graph_neighbours_and_best_tie_rules(built):
    g = _graph(7, *TWO_PARTS)
    assert g.neighbours(6, min_weight=1).tolist() == [1, 0, 2]                        # 9, then 7 and 7 by index
    ids, w = g.neighbours(6, min_weight=1, with_weights=True)
    assert w.tolist() == [9, 7, 7] and ids.dtype == np.int32
    assert g.neighbours(0, min_weight=1).tolist() == [1, 6, 2]                        # 7 and 7 by index, then 3
    assert g.neighbours(0, min_weight=7).tolist() == [1, 6] and g.neighbours(0, min_weight=8).tolist() == []
    assert g.neighbours(0).tolist() == []                                             # the default bar of 15 common points
    assert g.neighbours(5, min_weight=1).tolist() == []
    assert g.best(0, 2).tolist() == [1, 6] and g.best(0, 1).tolist() == [1] and g.best(0, 10).tolist() == [1, 6, 2]
    assert g.best(6, 2).tolist() == [1, 0] and g.best(3, 5).tolist() == [4] and g.best(2, 0).tolist() == []
    assert g.connected(6).tolist() == [0, 1, 2] and g.connected(4).tolist() == [3] and g.connected(5).tolist() == []
    with pytest.raises(ValueError):
        g.neighbours(7)


def test_graph_spanning_tree_two_components_and_ties(built):
    g = _graph(7, *TWO_PARTS)
    # 1: only 0.  2: 0 (3) or 1 (7) -> 1.  4: 3.  6: 0 (7), 1 (9), 2 (7) -> 1.  0, 3 and 5 have no lower neighbour.
    assert g.spanning_tree().tolist() == [-1, 0, 1, -1, 3, -1, 1]
    eq = _graph(5, [(0, 1), (0, 2), (1, 2), (0, 3), (1, 3), (2, 3), (2, 4), (3, 4)], [4] * 8)
    assert eq.spanning_tree().tolist() == [-1, 0, 0, 0, 2]                            # every weight equal: the lowest index
    assert _graph(3, [], []).spanning_tree().tolist() == [-1, -1, -1]


def test_graph_essential_edges(built):
    g = _graph(7, *TWO_PARTS)
    tree = [[0, 1], [1, 2], [1, 6], [3, 4]]
    assert g.essential_edges(min_weight=100).tolist() == tree
    assert g.essential_edges(min_weight=8).tolist() == tree                           # the one edge of 9 is a tree edge
    assert g.essential_edges(min_weight=7).tolist() == [[0, 1], [0, 6], [1, 2], [1, 6], [2, 6], [3, 4]]     # keeps 7s, drops (0, 2)
    assert g.essential_edges(min_weight=1).tolist() == [list(e) for e in TWO_PARTS[0]]
    # loop edges: one that duplicates a tree edge in the other orientation, one new, one listed twice
    got = g.essential_edges(min_weight=100, extra=[(6, 1), (5, 0), (0, 5), (4, 6)])
    assert got.tolist() == [[0, 1], [0, 5], [1, 2], [1, 6], [3, 4], [4, 6]] and got.dtype == np.int32
    assert _graph(2, [], []).essential_edges().shape == (0, 2)
    for bad in ([(0, 0)], [(0, 7)], [(-1, 2)]):
        with pytest.raises(ValueError):
            g.essential_edges(extra=bad)


def test_graph_refuses_what_is_not_a_covisibility_graph(built):
    for K, e, w in ((3, [(1, 0)], [1]), (3, [(0, 3)], [1]), (3, [(0, 1), (0, 1)], [1, 2]), (3, [(0, 1)], [0]), (3, [(0, 1)], [1, 2])):
        with pytest.raises(ValueError):
            _graph(K, e, w)


def test_graph_from_the_host_function(built):
    from slamhip import CovisibilityGraph, covisibility

    K, L, op, ol, fixed = C.cases()["configs4-scaled"]
    edges, weights = covisibility(op, ol, K, fixed, L)[:2]
    g = CovisibilityGraph(K, edges, weights)
    parent = g.spanning_tree()
    assert parent[0] == -1 == parent[1] and (parent[2:] >= 1).all()                   # pose 0 is fixed: it has no edge
    dense = np.zeros((K, K), np.int64)
    dense[edges[:, 0], edges[:, 1]] = weights
    dense += dense.T
    for k in (1, 17, 39):
        want = sorted(np.flatnonzero(dense[k]), key=lambda j: (-dense[k, j], j))
        assert g.neighbours(k, 1).tolist() == want and g.best(k, 10).tolist() == want[:10]
        below = [j for j in want if j < k]
        assert parent[k] == (below[0] if below else -1)


# ---- the host-only entries ---------------------------------------------------------------------------------------------------
def test_abi_table_loads(lib):
    from slamhip import _lib

    for name in ("slam_covis_limits", "slam_covis_plan", "slam_covis_workspace", "slam_covis_count", "slam_covis_pairs", "slam_covis_edges",
                 "slam_covis_rows"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]


def test_limits_plan_and_workspace_need_no_device(lib):
    from slamhip import covis
    from slamhip.ba_sparse import MAX_OBS, MAX_PAIRS, MAX_POINTS
    from slamhip.pose_graph import MAX_VERTICES

    lim = covis.limits()
    assert lim["threads"] == 256 and lim["ballot_lanes"] == 64 and lim["sort_tile"] % lim["threads"] == 0
    assert lim["scan_tile"] % lim["threads"] == 0 and lim["digit_bits"] == 8 and lim["key32_max_K"] == 65536 and lim["list_thresholds"] == 0
    # the passes the issue names: two at K = 200, three at K = 2 000; one, two and three around the digit boundaries
    for K, bits, passes, size in ((200, 16, 2, 4), (2000, 22, 3, 4), (16, 8, 1, 4), (17, 9, 2, 4), (255, 16, 2, 4), (256, 16, 2, 4),
                                  (257, 17, 3, 4), (65536, 32, 4, 4), (65537, 33, 5, 8), (70000, 33, 5, 8), (MAX_VERTICES, 48, 6, 8)):
        p = covis.plan(K, 1000, 5000, 7000)
        assert (p["pair_key_bits"], p["pair_passes"], p["pair_key_bytes"]) == (bits, passes, size), (K, p)
        assert p["pair_tiles"] == -(-7000 // lim["sort_tile"]) and p["obs_tiles"] == -(-5000 // lim["sort_tile"])
    p = covis.plan(200, 50000, 1000000, 0)
    assert p["pair_passes"] == 0 and p["obs_key_bytes"] == 4 and p["obs_passes"] == -(-p["obs_key_bits"] // 8)
    assert covis.plan(MAX_VERTICES, MAX_POINTS, 10, 0)["obs_key_bytes"] == 8
    # the workspaces hold what the header says they hold, and grow with what they hold
    c1, p1 = covis.workspace_bytes(200, 50000, 1000000, 9400000)
    assert c1 >= 1000000 * 16 + 50000 * 16 and p1 >= 9400000 * 16 and p1 < 9400000 * 20
    assert covis.workspace_bytes(200, 50000, 1000000, 0)[0] == c1
    assert covis.workspace_bytes(70000, 50000, 1000000, 9400000)[1] > p1 + 9400000 * 8 - 4096          # 64-bit pair keys
    assert covis.workspace_bytes(3, 1, 0, 0)[0] > 0
    n = (ctypes.c_uint64 * 2)()
    for K, L, O, P in ((0, 1, 0, 0), (MAX_VERTICES + 1, 1, 0, 0), (1, 0, 0, 0), (1, MAX_POINTS + 1, 0, 0), (1, 1, -1, 0), (1, 1, MAX_OBS + 1, 0),
                       (1, 1, 0, -1), (1, 1, 0, MAX_PAIRS + 1)):
        assert lib.slam_covis_workspace(K, L, O, P, n) == -1 and lib.slam_covis_plan(K, L, O, P, (ctypes.c_int32 * 8)()) == -1
    assert lib.slam_covis_workspace(1, 1, 0, 0, None) == -1 and lib.slam_covis_limits(None) == -1
    assert lib.slam_covis_workspace(MAX_VERTICES, MAX_POINTS, MAX_OBS, MAX_PAIRS, n) == 0 and n[1] > MAX_PAIRS * 24
