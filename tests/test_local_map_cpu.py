"""Local-map selection and keyframe culling without a device: the numpy statements of slamhip.local_map against the brute-force
statement of tests/local_map_ref.py on every case of tests/local_map_cases.py, the host-only functions on inputs whose answers
are written out here, the host-only entries of csrc/local_map.hip, and every refusal that needs no device."""
import ctypes
import re

import numpy as np
import pytest

import local_map_cases as C
import local_map_ref as R


@pytest.fixture(scope="module")
def lib(built):
    import slamhip

    return slamhip.load()


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def _same_votes(a, b):
    return all(_same(a[k], b[k]) for k in ("votes", "best", "nvoted")) and a["skipped"] == b["skipped"]


# ---- the numpy statements against the brute force ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lengths", "designed", "random"])
def test_frame_points_host_equals_reference(built, name):
    from slamhip import frame_points_host

    s = C.cull_scenes()[name]
    got, want = frame_points_host(s.observations(), s.frame_offsets), R.frame_points_ref(s.lists, s.frame_offsets)
    assert _same(got[0], want[0]) and got[1:] == want[1:] == (0, 0) and (got[0] >= 0).sum() == sum(len(x) for x in s.lists)


def test_frame_points_host_counts_what_it_refuses(built):
    from slamhip import MapObservations, frame_points_host

    fo = np.array([0, 2, 5])
    lists = [[(0, 1), (1, 0)], [(0, 1)], [(1, 3)], [(2, 0)], [(1, 0)], [(1, 0)]]       # row (0, 1) twice, (1, 0) three times, two out of range
    got, want = frame_points_host(MapObservations.from_lists(lists), fo), R.frame_points_ref(lists, fo)
    assert _same(got[0], want[0]) and got[1:] == want[1:] == (2, 3) and got[0].tolist() == [-1, 1, 5, -1, -1]


@pytest.mark.parametrize("F", [1, 2, 37])
def test_votes_host_equals_reference(built, F):
    from slamhip import votes_host

    s = C.vote_scene(F)
    for B in (1, 70):
        q = C.vote_queries(s, B)
        for rem, bad in ((s.removed, s.bad), ((), ())):
            got = votes_host(s.observations(), F, q, frame_removed=s.mask("removed") if rem else None, point_bad=s.mask("bad") if bad else None)
            assert _same_votes(got, R.votes_ref(s.lists, F, q, rem, bad))
    got = votes_host(s.observations(), F, C.vote_queries(s, 70), frame_removed=s.mask("removed"), point_bad=s.mask("bad"))
    assert got["skipped"] == 3 and got["best"][0].tolist() == got["best"][1].tolist() == [-1, 0] and got["nvoted"][:2].tolist() == [0, 0]
    assert got["votes"][:, s.removed].sum() == 0 and got["votes"][:, F - 1].sum() > 0


def test_vote_tie_goes_to_the_lowest_index(built):
    from slamhip import votes_host

    s = C.tie_scene()
    got = votes_host(s.observations(), s.F, [[0, 1, 2]])
    assert _same_votes(got, R.votes_ref(s.lists, s.F, [[0, 1, 2]]))
    assert got["best"].tolist() == [[2, 3]] and got["votes"][0].tolist() == [0, 0, 3, 0, 0, 3, 0, 1, 0] and got["nvoted"].tolist() == [3]
    none = votes_host(s.observations(), s.F, [])                      # no query at all
    assert none["votes"].shape == (0, s.F) and none["best"].shape == (0, 2) and none["skipped"] == 0


@pytest.mark.parametrize("M", C.points_sizes()[:3] + C.points_sizes()[-1:])
def test_local_points_host_equals_reference(built, M):
    from slamhip import frame_points_host, local_points_host

    s = C.points_scene(M)
    fp = frame_points_host(s.observations(), s.frame_offsets)[0]
    kfs, qs = C.points_queries(s)
    got = local_points_host(fp, s.frame_offsets, M, kfs, qs, frame_removed=s.mask("removed"), point_bad=s.mask("bad"))
    want = R.local_points_ref(fp, s.frame_offsets, M, kfs, qs, s.removed, s.bad)
    assert len(got) == 3 and all(_same(a, b) for a, b in zip(got, want))
    assert len(got[0]) > M // 2 and len(got[1]) == len(got[2]) == 0 and not set(got[0]) & (set(s.bad) | {0, 2})
    assert (np.diff(got[0]) > 0).all()                               # ascending, each once, though keyframes overlap


@pytest.mark.parametrize("name", ["lengths", "designed", "random"])
def test_redundancy_host_equals_reference(built, name):
    from slamhip import frame_points_host, keyframe_redundancy_host

    s = C.cull_scenes()[name]
    obs = s.observations()
    fp = frame_points_host(obs, s.frame_offsets)[0]
    for cname, cand in C.candidate_sets(s).items():
        for th in (C.TH, 0, 2):
            got = keyframe_redundancy_host(obs, fp, s.level, s.frame_offsets, cand, th, s.mask("removed"), s.mask("bad"))
            want = R.redundancy_ref(s.lists, fp, s.level, s.frame_offsets, cand, th, s.removed, s.bad)
            assert _same(got[0], want[0]) and _same(got[1], want[1]), (cname, th)


def test_designed_cases_have_the_property_they_exist_for(built):
    from slamhip import frame_points_host, keyframe_redundancy_host, redundant_verdict

    s = C.cull_designed()
    obs, n = s.observations(), s.notes
    fp = frame_points_host(obs, s.frame_offsets)[0]
    counts = keyframe_redundancy_host(obs, fp, s.level, s.frame_offsets, None, C.TH, s.mask("removed"))[0]
    assert counts[n["exact"]].tolist() == [2, 1] and counts[n["short"]].tolist() == [1, 0] and counts[n["levels"]].tolist() == [2, 1]
    assert counts[n["own"]].tolist() == [1, 0] and counts[n["nine"]].tolist() == [10, 9] and counts[n["ten"]].tolist() == [10, 10]
    assert counts[n["removed"]].tolist() == [1, 0] and counts[n["removed_candidate"]].tolist() == [0, 0]
    assert [counts[k].tolist() for k in n["twins"]] == [[30, 30], [30, 30]]
    alive = keyframe_redundancy_host(obs, fp, s.level, s.frame_offsets, None, C.TH)[0]               # nothing removed: N = 4 again
    assert alive[n["removed"]].tolist() == [1, 1] and alive[n["removed_candidate"]].tolist() == [2, 2]
    v = redundant_verdict(counts)
    assert not v[n["nine"]] and v[n["ten"]] and redundant_verdict(counts, (0, 1))[n["nine"]] and not redundant_verdict(counts, (0, 1))[n["own"]]
    lengths = C.cull_lengths()
    lim = C.limits()
    assert {lim["group16"] - 1, lim["group16"], lim["group16"] + 1, lim["group64"] - 1, lim["group64"], lim["group64"] + 1, lim["group256"] - 1,
            lim["group256"]} <= set(lengths.notes["lengths"])
    fo = lengths.frame_offsets
    lfp = frame_points_host(lengths.observations(), fo)[0]
    assert fo[301] == fo[300] and (lfp[fo[301]:fo[302]] == -1).all() and set(lfp[fo[302]:fo[303]]) - {-1} == set(lengths.bad)


# ---- the host-only functions on written-out inputs --------------------------------------------------------------------------
def _graph():
    from slamhip import CovisibilityGraph

    # 0 - 1 (9), 1 - 2 (8), 1 - 3 (7), 3 - 4 (6), 2 - 5 (5), 0 - 5 (1): parents 1 <- 0, 2 <- 1, 3 <- 1, 4 <- 3, 5 <- 2; 6 alone
    return CovisibilityGraph(7, [(0, 1), (1, 2), (1, 3), (3, 4), (2, 5), (0, 5)], [9, 8, 7, 6, 5, 1])


def test_local_keyframes_on_a_written_out_graph(built):
    from slamhip import local_keyframes

    g = _graph()
    assert g.spanning_tree().tolist() == [-1, 0, 1, 1, 3, 2, -1]
    # K1 = {1, 4}; from 1: best neighbour 0, first child 2, parent 0 (in); from 4: best neighbour 3, no child, parent 3 (in)
    kfs, ref = local_keyframes(np.array([0, 5, 0, 0, 5, 0, 0]), g)
    assert kfs.tolist() == [1, 4, 0, 2, 3] and ref == 1 and kfs.dtype == np.int32
    # K1 = {3}: best neighbour 1, first child 4, parent 1 (in)
    assert local_keyframes({"votes": np.array([[0, 0, 0, 2, 0, 0, 0]])}, g)[0].tolist() == [3, 1, 4]
    # removed frames are passed over: 1 gone, so the next best neighbour of 3 is 4; then no child left, parent gone
    assert local_keyframes(np.array([0, 0, 0, 2, 0, 0, 0]), g, frame_removed=[0, 1, 0, 0, 0, 0, 0])[0].tolist() == [3, 4]
    # the limit stops the expansion once the list holds more than `limit` entries; best = 0 leaves tree links only
    assert local_keyframes(np.array([0, 5, 0, 0, 5, 0, 0]), g, limit=1)[0].tolist() == [1, 4]
    assert local_keyframes(np.array([0, 5, 0, 0, 5, 0, 0]), g, limit=2)[0].tolist() == [1, 4, 0, 2]
    assert local_keyframes(np.array([0, 5, 0, 0, 5, 0, 0]), g, best=0)[0].tolist() == [1, 4, 2, 0, 3]
    none = local_keyframes(np.zeros(7, np.int64), g)
    assert none[0].tolist() == [] and none[1] == -1
    alone = local_keyframes(np.array([0, 0, 0, 0, 0, 0, 3]), g)
    assert alone[0].tolist() == [6] and alone[1] == 6
    for bad in (lambda: local_keyframes(np.zeros(6, np.int64), g), lambda: local_keyframes(np.zeros(7), g),
                lambda: local_keyframes(np.zeros(7, np.int64), None), lambda: local_keyframes(np.zeros(7, np.int64), g, limit=-1)):
        with pytest.raises(ValueError):
            bad()


def test_cull_map_points_on_written_out_inputs(built):
    from slamhip import cull_map_points

    #          ratio < 1/4   exactly 1/4   young, few obs   age 2, few obs   age 2, enough   age 3, few   age 3, enough   age 1
    found = [1, 1, 9, 9, 9, 9, 9, 9]
    visible = [5, 4, 9, 9, 9, 9, 9, 9]
    first = [10, 10, 9, 8, 8, 7, 7, 9]
    n_obs = [9, 9, 1, 2, 3, 2, 3, 0]
    got = cull_map_points(found, visible, first, n_obs, current_keyframe=10)
    assert got.dtype == np.uint8 and got.tolist() == [1, 0, 0, 2, 0, 2, 3, 0]
    assert cull_map_points(found, visible, first, n_obs, 10, th_obs=3).tolist() == [1, 0, 0, 2, 2, 2, 2, 0]
    assert cull_map_points([], [], [], [], 3).tolist() == []
    with pytest.raises(ValueError):
        cull_map_points([1], [1, 2], [0], [0], 3)
    with pytest.raises(ValueError):
        cull_map_points([1.0], [1], [0], [0], 3)


def test_remove_frames_on_written_out_inputs(built):
    from slamhip import MapObservations, remove_frames

    obs = MapObservations.from_lists([[(0, 3), (2, 1), (5, 0)], [], [(2, 7)], [(1, 1), (5, 2)]])
    out = remove_frames(obs, [2, 5])
    assert out.lists() == [[(0, 3)], [], [], [(1, 1)]] and out.offsets.tolist() == [0, 1, 1, 1, 2]
    assert remove_frames(obs, np.array([False, False, True, False, False, True])).lists() == out.lists()
    assert remove_frames(obs, []).lists() == obs.lists() and remove_frames(obs, [0, 1, 2, 5]).nnz == 0
    assert obs.lists()[0] == [(0, 3), (2, 1), (5, 0)]                  # the argument is left as it was
    for bad in (lambda: remove_frames(obs.lists(), [1]), lambda: remove_frames(obs, [-1]), lambda: remove_frames(obs, [0.5])):
        with pytest.raises(ValueError):
            bad()


# ---- the host-only entries ---------------------------------------------------------------------------------------------------
NAMES = ("slam_lmap_limits", "slam_lmap_workspace", "slam_lmap_frame_points", "slam_lmap_vote", "slam_lmap_points_mark", "slam_lmap_points_fill",
         "slam_lmap_cull_count")


def test_abi_table_header_and_library_agree(lib):
    import os

    from slamhip import _lib

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "slamhip.h")).read()
    declared = re.findall(r"SLAM_API int (slam_lmap_\w+)\(([^;]*)\);", header)
    assert sorted(n for n, _ in declared) == sorted(NAMES) == sorted(n for n in _lib.SIGNATURES if n.startswith("slam_lmap_"))
    for name, args in declared:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1] and len(_lib.SIGNATURES[name][1]) == args.count(",") + 1, name


def test_limits_and_workspace_need_no_device(lib):
    from slamhip import local_map as L

    lim = L.limits()
    assert lim["threads"] == 256 and (lim["group16"], lim["group64"], lim["group256"]) == (16, 64, 256)
    assert lim["vote_lds_small"] * 4 == 16384 and 4 * lim["vote_lds_frames"] + 1024 <= 160 * 1024 < 4 * (lim["vote_lds_frames"] + 1024)
    assert lim["scan_tile_words"] % lim["threads"] == 0 and lim["scalar_bytes"] == 256
    a, b = L.workspace_bytes(1, 200, 50000, 30), L.workspace_bytes(256, 2000, 200000, 2000)
    assert all(a[k] >= 256 and a[k] % 256 == 0 for k in a) and a["frame_points"] == b["frame_points"] == 256
    assert b["vote"] >= 256 + 257 * 8 and b["points"] >= 256 + 3 * 257 * 8 + 256 * 7 * 4 and b["cull"] >= 256 + 2000 * 4 + 2001 * 8
    assert b["points"] > a["points"] and b["cull"] > a["cull"] and b["vote"] > a["vote"]
    n = (ctypes.c_uint64 * 4)()
    for B, F, M, Cn in ((-1, 1, 1, 0), (65536, 1, 1, 0), (0, 0, 1, 0), (0, (1 << 24) + 1, 1, 0), (0, 1, 0, 0), (0, 1, (1 << 24) + 1, 0), (0, 1, 1, -1)):
        assert lib.slam_lmap_workspace(B, F, M, Cn, n) == -1 and b"slam_lmap_workspace" in lib.slam_last_error()
    assert lib.slam_lmap_workspace(65535, 1 << 24, 1 << 24, 1 << 24, n) == 0
    assert lib.slam_lmap_workspace(1, 1, 1, 0, None) == -1 and lib.slam_lmap_limits(None) == -1


def test_entry_points_refuse_before_they_look_at_a_device(lib):
    o = ctypes.c_void_p(256)                   # never dereferenced: every call below is refused on its arguments
    off = (ctypes.c_int64 * 3)(0, 1, 2)
    desc = (ctypes.c_int64 * 3)(0, 2, 1)
    s = (ctypes.c_int64 * 2)()
    bad = [lib.slam_lmap_frame_points(None, 1, 0, o, o, 1, o, 0, o, o, s),
           lib.slam_lmap_vote(None, 1, o, off, 1, 0, o, o, None, 1, None, 0, o, o, o, o, None),
           lib.slam_lmap_points_mark(None, 1, o, off, o, off, 1, None, 1, o, 0, o, None, o, o, s),
           lib.slam_lmap_points_fill(None, 1, 1, o, o, off, o),
           lib.slam_lmap_cull_count(None, 1, None, 1, 0, o, o, None, 1, off, o, o, o, None, 3, 16, o, o, None)]
    assert bad == [-1] * len(bad)


@pytest.mark.parametrize("what", ["masks", "lists", "th_obs", "candidates", "ratio", "offsets"])
def test_python_refusals_need_no_device(built, what):
    from slamhip import keyframe_redundancy_host, local_map as L, local_points_host, votes_host

    s = C.tie_scene()
    obs = s.observations()
    fp = L.frame_points_host(obs, s.frame_offsets)[0]
    calls = {
        "masks": [lambda: votes_host(obs, s.F, [[0]], frame_removed=np.zeros(s.F + 1, bool)), lambda: votes_host(obs, s.F, [[0]], point_bad=np.zeros(s.M)),
                  lambda: local_points_host(fp, s.frame_offsets, s.M, [[0]], [[0]], point_bad=[0])],
        "lists": [lambda: votes_host(obs, s.F, [[0.5]]), lambda: votes_host(obs, s.F, [0, 1], offsets=[0, 1]), lambda: votes_host(obs, s.F, [1 << 40]),
                  lambda: local_points_host(fp, s.frame_offsets, s.M, [[0], [1]], [[0]])],
        "th_obs": [lambda: keyframe_redundancy_host(obs, fp, s.level, s.frame_offsets, None, 257), lambda: keyframe_redundancy_host(obs, fp, s.level, s.frame_offsets, None, 1.5),
                   lambda: keyframe_redundancy_host(obs, fp, s.level, s.frame_offsets, None, -1)],
        "candidates": [lambda: keyframe_redundancy_host(obs, fp, s.level, s.frame_offsets, [s.F]), lambda: keyframe_redundancy_host(obs, fp, s.level, s.frame_offsets, [-1]),
                       lambda: keyframe_redundancy_host(obs, fp, s.level, s.frame_offsets, [[0]])],
        "ratio": [lambda: L.redundant_verdict([[1, 1]], (1, 0)), lambda: L.redundant_verdict([[1, 1]], (-1, 2)), lambda: L.redundant_verdict([[1, 1]], (0.9, 1))],
        "offsets": [lambda: L.frame_points_host(obs, [0]), lambda: L.frame_points_host(obs, [1, 2]), lambda: L.frame_points_host(obs, [0, 3, 2]),
                    lambda: L.MapTables.from_observations(obs.lists(), s.frame_offsets, s.level)],
    }[what]
    for call in calls:
        with pytest.raises(ValueError):
            call()
