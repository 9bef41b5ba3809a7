"""The fusion search and the map-point refresh without a GPU: csrc/fuse_point.h built by g++ (tests/fuse_twin.py,
a second time under AddressSanitizer and UndefinedBehaviorSanitizer) against tests/fuse_ref.py bit for bit, the edges of the
reprojection gate and of the median rank, the merge rules of apply_fusion, and the argument errors that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import fuse_cases as C
import fuse_ref as F
import fuse_twin as T
import proj_match_cases as PC
import proj_match_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def fz(built):
    from slamhip import fuse as module
    return module


# ---- the gates ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("san", [False, True])
def test_twin_gates_equal_the_numpy_statement_bit_for_bit(san):
    pts, _, pose, _ = PC.make_scene(5, 300, n_levels=8)
    Ow = -pose[:, :3].T @ pose[:, 3]
    g = np.random.default_rng(1)                         # some ranges end inside the margins, some beyond them
    rng = pts["range"] * np.stack([g.choice([1.0, 20.0, 50.0], 300), g.choice([0.2, 0.6, 1.0, 1.3], 300)], 1)
    seen = set()
    for margins in ((0.64, 1.44), (1.0, 1.0), (0.3, 3.0)):
        want = F.gates(pts["xyz"], pose, Ow, 3.0, PC.CAMERA, PC.BOUNDS, *R.scale_tables(8, 1.2), rng, pts["normal"], None, 0.25, margins)
        got = T.gates(pts["xyz"], pose, Ow, 3.0, PC.CAMERA, PC.BOUNDS, *R.scale_tables(8, 1.2), rng, pts["normal"], None, 0.25, margins, san=san)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[3], want[3])
        assert np.array_equal(bits(got[1]), bits(want[1])) and np.array_equal(bits(got[2]), bits(want[2]))
        seen.add(int((want[0] == 3).sum()))
        assert {0, 3} <= set(want[0].tolist())
    assert len(seen) == 3                                # the margins decide


def test_margins_of_one_are_the_gates_of_the_projection_search():
    """(1, 1) is pp_gates exactly - on the edge points, whose statuses are stated from the arithmetic, and on a scene."""
    xyz, rng, nrm, status, lp = PC.edge_points()
    s, s2 = R.scale_tables(4, 2.0)
    got = T.gates(xyz, C.I34, np.zeros(3), 1.0, PC.CAMERA, PC.BOUNDS, s, s2, rng, nrm, None, 0.25, (1.0, 1.0))
    assert np.array_equal(got[0], status) and np.array_equal(got[3], lp)
    pts, _, pose, _ = PC.make_scene(9, 200)
    Ow = -pose[:, :3].T @ pose[:, 3]
    s, s2 = R.scale_tables(8, 1.2)
    want = R.gates(pts["xyz"], pose, Ow, 2.0, PC.CAMERA, PC.BOUNDS, s, s2, pts["range"], pts["normal"])
    got = T.gates(pts["xyz"], pose, Ow, 2.0, PC.CAMERA, PC.BOUNDS, s, s2, pts["range"], pts["normal"], None, 0.25, (1.0, 1.0))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[3], want[3]) and np.array_equal(bits(got[1]), bits(want[1]))


def test_margins_move_the_range_gate_and_never_the_predicted_level():
    """A point at d2 = 16 with dmax2 = 15: out of range at (1, 1), in range at (1, 1.44), and its level is counted against
    15, not against 21.6: 1 * 16 < 15 fails at once -> lp = 0.  With dmax2 = 20 both margins agree on lp = 1."""
    s, s2 = R.scale_tables(4, 2.0)
    xyz = np.array([[0.0, 0.0, 4.0]] * 3)
    rng = np.array([[1.0, 15.0], [1.0, 20.0], [25.0, 4096.0]])
    one = T.gates(xyz, C.I34, np.zeros(3), 1.0, PC.CAMERA, PC.BOUNDS, s, s2, rng, None, None, 0.25, (1.0, 1.0))
    wide = T.gates(xyz, C.I34, np.zeros(3), 1.0, PC.CAMERA, PC.BOUNDS, s, s2, rng, None, None, 0.25, (0.64, 1.44))
    assert one[0].tolist() == [3, 0, 3] and wide[0].tolist() == [0, 0, 0]      # 0.64 * 25 = 16 is not above d2 = 16
    assert wide[3].tolist() == [0, 1, 3] and one[3].tolist() == [-1, 1, -1]
    ref = F.gates(xyz, C.I34, np.zeros(3), 1.0, PC.CAMERA, PC.BOUNDS, s, s2, rng, None, None, 0.25, (0.64, 1.44))
    assert np.array_equal(ref[0], wide[0]) and np.array_equal(ref[3], wide[3])


# ---- the reprojection gate ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("san", [False, True])
def test_chi2_gate_keeps_equality_rejects_the_next_double_and_passes_nan(san):
    """e2 = 3^2 + 4^2 = 25 exactly.  lim = 25 keeps the row, the next double below 25 rejects it; a NaN limit, a NaN pixel and
    a NaN projection reject nothing."""
    xy = np.array([[13.0, 24.0]] * 4 + [[np.nan, 24.0]], np.float32)
    lim = np.array([25.0, np.nextafter(25.0, 0.0), np.nextafter(25.0, 30.0), np.nan, 1.0])
    assert T.candidates(10.0, 20.0, xy, lim, san=san).tolist() == [True, False, True, True, True]
    assert T.candidates(np.nan, 20.0, xy[:2], lim[:2], san=san).tolist() == [True, True]
    # the numpy statement's gate, on the same numbers
    ex, ey = 10.0 - xy[:, 0].astype(np.float64), 20.0 - xy[:, 1].astype(np.float64)
    with np.errstate(invalid="ignore"):
        assert (~((ex * ex + ey * ey) > lim)).tolist() == [True, False, True, True, True]


# ---- the median and the choice ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("san", [False, True])
def test_median_rank_for_small_and_full_lists(san):
    rng = np.random.default_rng(2)
    for N in (1, 2, 3, 4, 5, 31, 256):
        rows = rng.integers(0, 256, (N, 32), dtype=np.uint8)
        rows[N // 2:] = C.flip_bits(rng, np.repeat(rows[:1], N - N // 2, 0), 9)       # a cluster: many equal distances
        D = R.hamming(rows, rows)
        med, best = T.medians(D, san=san)
        want_med, want_best = F.median_choice(D)
        assert np.array_equal(med, want_med) and best == want_best, N
        assert np.array_equal(med, [sorted(r)[(N - 1) // 2] for r in D.tolist()])
    assert T.medians(np.zeros((0, 0)), san=san)[1] == -1
    # ranks by hand: N = 2 -> rank 0 is the diagonal zero; N = 4 -> rank 1; N = 3 -> rank 1 (the true median)
    assert T.medians([[0, 7], [7, 0]], san=san)[0].tolist() == [0, 0]
    assert T.medians([[0, 5, 9], [5, 0, 2], [9, 2, 0]], san=san)[0].tolist() == [5, 2, 2]
    assert T.medians([[0, 5, 9, 256], [5, 0, 2, 3], [9, 2, 0, 1], [256, 3, 1, 0]], san=san)[0].tolist() == [5, 2, 1, 1]


def test_median_ties_go_to_the_first_observation():
    med, best = T.medians([[0, 5, 9], [5, 0, 2], [9, 2, 0]])
    assert best == 1                                     # medians 5, 2, 2: rows 1 and 2 tie, the smaller index wins
    assert T.medians([[0, 4], [4, 0]])[1] == 0 and T.medians(np.zeros((256, 256)))[1] == 0
    D = np.full((256, 256), 256)
    np.fill_diagonal(D, 0)
    D[255, :200] = 0
    assert T.medians(D) [1] == 255 and F.median_choice(D)[1] == 255


# ---- normal and range -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("san", [False, True])
def test_twin_normal_and_range_equal_the_numpy_statement(san):
    rng = np.random.default_rng(4)
    for N in (1, 2, 3, 17, 256):
        X, O = rng.normal(0, 3, 3), rng.normal(0, 1, (N, 3))
        ref, level = int(rng.integers(0, N)), int(rng.integers(-2, 10))
        nr, rg = T.normal_range(X, O, ref, level, C.SCALE, san=san)
        lists = [[(b, 0) for b in range(N)]]
        want = F.refresh(X[None], lists, [np.zeros((1, 32), np.uint8)] * N, [np.array([level])] * N, O, C.SCALE, ref=[ref])
        assert np.array_equal(bits(nr), bits(want["normal"][0])) and np.array_equal(bits(rg), bits([want["dmin2"][0], want["dmax2"][0]]))
        assert abs(np.linalg.norm(nr) - 1) < 1e-12 and rg[0] < rg[1]


def test_two_views_give_the_normal_and_range_of_the_triangulation():
    """A point with two observations and ref 0 gets the bits tp_triangulate gave it (tests/tri_match_twin.py)."""
    import tri_match_cases as TC
    import tri_match_twin as TT
    s1, s2, _, truth = TC.make_scene(3, 40, 50)
    got = TT.triangulate(TC.POSES[0], TC.POSES[1], TC.CAMERA, TC.SCALE, TC.SIGMA2, s1["xy"][truth["rows1"]], s2["xy"][truth["rows2"]],
                         s1["level"][truth["rows1"]], s2["level"][truth["rows2"]])
    made = np.flatnonzero(got["status"] == 0)
    assert len(made) >= 30
    O = np.stack([-T_[:, :3].T @ T_[:, 3] for T_ in TC.POSES[:2]])
    for i in made:
        nr, rg = T.normal_range(got["X"][i], O, 0, int(s1["level"][truth["rows1"][i]]), TC.SCALE)
        assert np.array_equal(bits(nr), bits(got["normal"][i])) and np.array_equal(bits(rg), bits([got["dmin2"][i], got["dmax2"][i]]))


def test_degenerate_views_give_nan():
    nr, rg = T.normal_range([1.0, 2.0, 3.0], [[1.0, 2.0, 3.0], [0.0, 0.0, 0.0]], 1, 0, C.SCALE)       # a zero length
    assert np.isnan(nr).all() and np.isnan(rg).all()
    nr, rg = T.normal_range([0.0, 0.0, 0.0], [[0.0, 0.0, 1.0], [0.0, 0.0, -1.0]], 0, 0, C.SCALE)      # a zero sum
    assert np.isnan(nr).all() and np.isnan(rg).all()
    nr, rg = T.normal_range([np.nan, 0.0, 0.0], [[0.0, 0.0, 1.0]], 0, 0, C.SCALE)
    assert np.isnan(nr).all() and np.isnan(rg).all()


# ---- the numpy statement against the scenes' construction --------------------------------------------------------------

def test_reference_search_gives_the_constructed_answer():
    W = C.world(11, 80, n_frames=3, n_dup=10)
    sets = C.keyframe_sets(W)
    for a, b in ((0, 1), (1, 0), (2, 1), (1, 1)):
        got = C.ref_pair(F, W, sets, a, b)
        st, row, ot = C.expected(W, sets[a], b)
        assert np.array_equal(got["status"], st) and np.array_equal(got["row"], row) and np.array_equal(got["other"], ot), (a, b)
    assert (C.ref_pair(F, W, sets, 0, 1)["other"] >= 0).sum() == 10          # the duplicates meet their originals


# ---- apply_fusion ---------------------------------------------------------------------------------------------------------------

def link(frame, rows):
    """A result dict from (id, status, other, row) tuples."""
    a = np.array(rows, np.int32).reshape(-1, 4)
    return dict(frame=frame, id=a[:, 0], status=a[:, 1], other=a[:, 2], row=a[:, 3])


def check_fusion(fz, lists, results):
    obs = fz.MapObservations.from_lists(lists)
    new, alias, upd = fz.apply_fusion(obs, results)
    want = F.apply_fusion(lists, results)
    assert new.lists() == [list(map(tuple, x)) for x in want[0]] and alias.tolist() == want[1] and [tuple(u) for u in upd.tolist()] == want[2]
    new2, alias2, upd2 = fz.apply_fusion(obs, results[::-1])                 # the order of the results does not matter
    assert new2.lists() == new.lists() and np.array_equal(alias2, alias) and np.array_equal(upd2, upd)
    return new.lists(), alias.tolist(), [tuple(u) for u in upd.tolist()]


def test_apply_fusion_chain_merges_into_the_point_with_most_observations(fz):
    lists = [[(0, 1)], [(1, 2), (2, 5)], [(3, 4), (4, 4), (5, 0)], [(9, 9)]]
    res = [link(1, [(0, 0, 1, 2)]), link(3, [(1, 0, 2, 4)])]                # 0 -> 1 -> 2: one class
    new, alias, upd = check_fusion(fz, lists, res)
    assert alias == [2, 2, 2, 3]
    assert new == [[], [], [(0, 1), (1, 2), (2, 5), (3, 4), (4, 4), (5, 0)], [(9, 9)]]
    assert upd == [(0, 1, 2), (1, 2, 2), (2, 5, 2)]


def test_apply_fusion_tie_goes_to_the_smallest_id_and_status_8_links(fz):
    lists = [[(0, 0)], [(1, 1)], [(2, 2)]]
    new, alias, upd = check_fusion(fz, lists, [link(5, [(2, 8, 1, 7), (1, 0, -1, 7)])])
    assert alias == [0, 1, 1] and new == [[(0, 0)], [(1, 1), (2, 2), (5, 7)], []]
    assert upd == [(2, 2, 1), (5, 7, 1)]


def test_apply_fusion_two_rows_in_one_frame(fz):
    """The survivor's own row stays; between two members' rows the smallest stays; the dropped rows lose their point."""
    lists = [[(0, 9), (1, 1), (2, 2)], [(0, 3), (4, 8)], [(4, 6), (5, 5)]]
    new, alias, upd = check_fusion(fz, lists, [link(0, [(1, 0, 0, 9)]), link(4, [(2, 0, 1, 8)])])
    assert alias == [0, 0, 0]
    assert new[0] == [(0, 9), (1, 1), (2, 2), (4, 6), (5, 5)] and new[1] == new[2] == []
    assert upd == [(0, 3, -1), (4, 6, 0), (4, 8, -1), (5, 5, 0)]


def test_apply_fusion_contested_row_between_pairs(fz):
    """Two points of two pairs gain an observation on one row of a shared frame: they are one landmark."""
    lists = [[(0, 0), (1, 0)], [(2, 0)], [(3, 3)]]
    new, alias, upd = check_fusion(fz, lists, [link(7, [(0, 0, -1, 4)]), link(7, [(1, 0, -1, 4), (2, 0, -1, 5)])])
    assert alias == [0, 0, 2] and new == [[(0, 0), (1, 0), (2, 0), (7, 4)], [], [(3, 3), (7, 5)]]
    assert upd == [(2, 0, 0), (7, 4, 0), (7, 5, 2)]


def test_apply_fusion_leaves_an_untouched_map_alone(fz):
    lists = [[(0, 0)], [], [(1, 1)]]
    new, alias, upd = check_fusion(fz, lists, [link(3, [(0, 5, -1, -1), (2, 7, -1, 2), (-1, 0, -1, 1)])])
    assert new == [[(0, 0)], [], [(1, 1)]] and alias == [0, 1, 2] and upd == []


# ---- arguments ------------------------------------------------------------------------------------------------------------------

def test_observation_tables_are_checked_where_they_are_built(fz):
    MO = fz.MapObservations
    assert MO.from_lists([[(0, 1), (3, 0)], [], [(2, 2)]]).nobs.tolist() == [2, 0, 1]
    assert MO.from_lists([]).nnz == 0
    assert MO.from_lists([[(b, 0) for b in range(256)]]).nobs.tolist() == [256]
    for bad in ([[(1, 0), (1, 1)]], [[(2, 0), (1, 0)]], [[(b, 0) for b in range(257)]], [[(-1, 0)]]):
        with pytest.raises(ValueError):
            MO.from_lists(bad)
    MO.from_lists([[(5, 0)], [(1, 0)]])                  # the step from one list into the next may descend
    for off, ob in (([0, 2, 1], [[0, 0], [1, 0]]), ([1, 2], [[0, 0], [1, 0]]), ([0, 1], [[0, 0], [1, 0]]), ([0, 1], [[0.5, 0]])):
        with pytest.raises(ValueError):
            MO.from_arrays(off, ob)


def test_library_rejects_bad_arguments_without_a_device(fz):
    """Both entry points check their arguments before they look at the context, so every check that needs no device pointer
    can be reached here with a null context: each is told from the others, and from the null-context error a valid call ends
    in, by the library's error text."""
    from slamhip._lib import SLAM_ERR_INVALID, FuseParams, ProjFrames, ProjParams, ProjPoints, addr, load
    lib = load()
    assert fz.limits()["observations"] == 256 and fz.limits()["pair_bytes"] == 184
    assert lib.slam_fuse_limits(None) == SLAM_ERR_INVALID

    def said(rc, text):
        msg = lib.slam_last_error().decode()
        assert rc == SLAM_ERR_INVALID and text in msg, (rc, msg)

    # ---- the refresh: one frame of 4 rows, 8 levels
    foff, s = np.array([0, 4], np.int64), np.ones(8)

    def refresh(off, M, select=None, K=0, frame_off=foff, B=1, scale=s, levels=8):
        return lib.slam_fuse_refresh(None, None, addr(off) if off is not None else None, None, M, addr(select) if select is not None else None, K,
                                     None, None, None, addr(frame_off), B, None, None, addr(scale) if scale is not None else None, levels,
                                     None, None, None, None)

    said(refresh(np.array([0, 2, 259], np.int64), 2), "point 1 has 257 observations")
    said(refresh(np.array([0, 3, 2], np.int64), 2), "offsets descend at point 1")
    said(refresh(np.array([1, 2], np.int64), 1), "do not start at 0")
    said(refresh(None, 1), "null observation offsets")
    said(refresh(np.array([0, 1], np.int64), 1 << 25), "map points out of range")
    said(refresh(np.array([0, 1, 2], np.int64), 2, np.array([0, 2], np.int32), 2), "select[1] = 2 names no map point")
    said(refresh(np.array([0, 1], np.int64), 1, levels=17), "n_levels=17")
    said(refresh(np.array([0, 1], np.int64), 1, scale=None), "null scale table")
    said(refresh(np.array([0, 1], np.int64), 1, frame_off=np.array([0, 5, 4], np.int64), B=2), "frame 1 has -1 rows")
    said(refresh(np.array([0, 256], np.int64), 1), "null ctx")              # 256 is allowed: only the context is missing

    # ---- the search: one empty point set, one empty frame, a table of two points
    zero = np.array([0, 0], np.int64)
    sc, sc2 = C.SCALE, C.SCALE2
    pts = ProjPoints(None, None, None, None, None, None, addr(zero), 1)
    frm = ProjFrames(None, None, None, None, None, None, None, addr(zero), 1, 640, 480, 16, 0)
    prm = ProjParams(1.0, 1.0, 0.0, 0.0, 0.0, 640.0, 0.0, 480.0, 0.25, 0.0, addr(sc), addr(sc2), 8, 0, 1, -1, 0, 0)
    table = np.array([0, 1, 3], np.int64)
    d_off = 64                                           # never dereferenced on the host: any aligned non-null value

    def search(fp=FuseParams(0.64, 1.44, 5.99, 50, 0), off=table, M=2, P=0, frames=frm, params=prm):
        return lib.slam_fuse_search(None, ctypes.byref(pts), None, ctypes.byref(frames), None, addr(off), d_off, d_off, M, None, None, None, None, P,
                                    ctypes.byref(params), ctypes.byref(fp), *([None] * 8))

    for lo2, hi2 in ((np.nan, 1.44), (0.64, np.nan), (0.0, 1.44), (0.64, -1.0)):
        said(search(FuseParams(lo2, hi2, 5.99, 50, 0)), "margins")
    said(search(FuseParams(0.64, 1.44, np.nan, 50, 0)), "chi2 is not a number")
    said(search(FuseParams(0.64, 1.44, 5.99, 257, 0)), "th_low=257")
    said(search(FuseParams(0.64, 1.44, 5.99, -1, 0)), "th_low=-1")
    said(search(off=np.array([0, 2, 1], np.int64)), "offsets descend at point 1")
    said(search(off=np.array([0, 257, 258], np.int64)), "point 0 has 257 observations")
    said(search(P=4097), "P=4097")
    said(search(frames=ProjFrames(None, None, None, None, None, None, None, addr(zero), 1, 640, 480, 0, 0)), "cell=0")
    said(search(params=ProjParams(1.0, 1.0, 0.0, 0.0, 0.0, 640.0, 0.0, 480.0, 0.25, 0.0, addr(sc), addr(sc2), 8, 0, 1, 1, 0, 0)), "descend")
    said(search(), "null ctx")                           # every argument is in order: only the context is missing
    assert lib.slam_fuse_search(*([None] * 8), 0, *([None] * 4), 0, *([None] * 10)) == SLAM_ERR_INVALID

    assert ctypes.sizeof(FuseParams) == 32
    header = open(os.path.join(ROOT, "include", "slamhip.h")).read()
    for n in ("slam_fuse_limits", "slam_fuse_search", "slam_fuse_refresh"):
        assert re.search(r"SLAM_API int %s\(" % n, header)
    assert "#define SLAM_FUSE_OBS_MAX 256" in header


def test_python_rejects_bad_arguments_before_any_launch(fz):
    with pytest.raises(ValueError):
        fz._fuse_params(50, (np.nan, 1.44), 5.99)
    with pytest.raises(ValueError):
        fz._fuse_params(50, (0.64, 0.0), 5.99)
    with pytest.raises(ValueError):
        fz._fuse_params(50, (-1.0, 1.0), 5.99)
    with pytest.raises(ValueError):
        fz._fuse_params(257, (0.64, 1.44), 5.99)
    with pytest.raises(ValueError):
        fz._fuse_params(50, (0.64, 1.44), np.nan)
    with pytest.raises(ValueError):
        fz._ids_arg([0, 5], 2, "ids", 5)
    with pytest.raises(ValueError):
        fz.fuse_points(None, [], None, [], None, [], [])
    with pytest.raises(ValueError):
        fz.apply_fusion([[(0, 0)]], [])
