"""Local-map selection and keyframe culling on the device (csrc/local_map.hip) against the numpy statements of
slamhip.local_map and the brute-force statement of tests/local_map_ref.py, bit for bit on every output array.  Every call runs
twice: on workspaces filled with 0xFF and outputs filled with 0xA5, then on what the first run left in the same blocks."""
import ctypes

import numpy as np
import pytest

import local_map_cases as C
import local_map_ref as R
import proj_match_cases as PC

pytestmark = pytest.mark.gpu


class Blocks:
    """Stands in for ``local_map._new``: every block a call takes is remembered and filled - a workspace with 0xFF, an output
    with 0xA5 - and handed out as a view, so that it outlives the call; ``twice`` hands the same blocks out once more, in the
    same order, as the first run left them."""

    def __init__(self, monkeypatch):
        from slamhip import local_map

        self.blocks, self.replay = [], []
        monkeypatch.setattr(local_map, "_new", self.new)

    def new(self, ctx, held, nbytes, role):
        n = max(int(nbytes), 16)
        if self.replay:
            b, was, size = self.replay.pop(0)
            assert (was, size) == (role, n)
        else:
            b = ctx.malloc(n)
            b.upload(np.full(n, 0xFF if role == "ws" else 0xA5, np.uint8))
        self.blocks.append((b, role, n))
        return b.view(0, n)


def twice(blocks, fn):
    """``fn()`` on poisoned blocks and again on the leftovers -> both results; the blocks of the two runs are freed."""
    base = len(blocks.blocks)
    try:
        first = fn()
        blocks.replay = blocks.blocks[base:]
        del blocks.blocks[base:]
        second = fn()
        assert not blocks.replay                                     # the second run took the blocks of the first, all of them
        return first, second
    finally:
        for b, _, _ in blocks.blocks[base:] + blocks.replay:
            b.free()
        del blocks.blocks[base:]
        blocks.replay = []


class Allocations:
    """Every buffer the context hands out while this is installed; ``live`` are the ones not freed yet."""

    def __init__(self, ctx, monkeypatch):
        self.buffers = []
        malloc = ctx.malloc

        def tracked(nbytes):
            self.buffers.append(malloc(nbytes))
            return self.buffers[-1]

        monkeypatch.setattr(ctx, "malloc", tracked, raising=False)

    @property
    def live(self):
        return [b for b in self.buffers if b.ptr]


class Resident:
    """The tables of a scene on the device for the length of a ``with``."""

    def __init__(self, ctx, scene):
        self.ctx, self.scene = ctx, scene

    def __enter__(self):
        self.t, self.obs = self.scene.tables(self.ctx)
        return self.t

    def __exit__(self, *exc):
        self.t.free()
        self.obs.free()


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _same_votes(a, b):
    return all(_same(a[k], b[k]) for k in ("votes", "best", "nvoted")) and a["skipped"] == b["skipped"]


# ---- the inverse table ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lengths", "designed", "random"])
def test_frame_points_equal_host_and_reference(gpu_ctx, monkeypatch, name):
    from slamhip import frame_points_host

    s = C.cull_scenes()[name]
    blocks = Blocks(monkeypatch)
    want = frame_points_host(s.observations(), s.frame_offsets)[0]
    assert _same(want, R.frame_points_ref(s.lists, s.frame_offsets)[0])

    def run():
        with Resident(gpu_ctx, s) as t:
            assert t.frame_removed.tolist() == s.mask("removed").tolist() and t.max_list == max(len(x) for x in s.lists)
            assert t.d_frame_removed.download(np.uint8, (s.F,)).tolist() == s.mask("removed").tolist()
            return t.frame_points(), t.level()

    for fp, lv in twice(blocks, run):
        assert _same(fp, want) and _same(lv, s.level)


def test_frame_points_round_trip_on_the_fusion_scene(gpu_ctx, monkeypatch):
    import fuse_cases as FC
    from slamhip import FrameGrids, MapObservations, MapTables

    W = FC.world(5, 120, n_frames=4, n_dup=6)
    frames = W["frames"]
    off = np.concatenate([[0], np.cumsum([len(f["level"]) for f in frames])]).astype(np.int64)
    cat = lambda k, dt: np.concatenate([np.asarray(f[k], dt) for f in frames])  # noqa: E731
    fg = FrameGrids.from_arrays(cat("desc", np.uint8), cat("xy", np.float32), cat("level", np.int64), FC.SIZE, off, ctx=gpu_ctx)
    obs = MapObservations.from_lists(W["lists"], gpu_ctx)
    blocks = Blocks(monkeypatch)
    try:
        def run():
            t = MapTables.from_observations(obs, fg)                # the levels are the grids' own
            try:
                assert t.d_level is fg.device["level"] and t.F == 4 and t.M == len(W["lists"])
                return t.frame_points(), t.level()
            finally:
                t.free()

        for fp, lv in twice(blocks, run):
            assert _same(fp, cat("point", np.int32)) and _same(lv, cat("level", np.int32))
        assert fg.device["level"].ptr                               # freeing the tables left the grids whole
    finally:
        obs.free()
        fg.free()


def test_frame_points_refusals_are_counted_and_write_nothing_outside(gpu_ctx, monkeypatch):
    from slamhip import MapObservations, MapTables, frame_points_host, local_map

    fo = np.array([0, 2, 5], np.int64)
    level = np.zeros(5, np.int32)
    refused = [("a row claimed twice", [[(0, 1), (1, 0)], [(0, 1)], [(1, 2)]], "1 claims of a frame row"),
               ("a row past its frame", [[(0, 2)], [(1, 0)]], "1 observations name a frame or a row outside"),
               ("a frame past the last", [[(0, 0), (2, 0)], [(1, 1)], [(7, 0)]], "2 observations name a frame or a row outside")]
    alloc = Allocations(gpu_ctx, monkeypatch)
    good = [[(0, 1), (1, 0)], [(0, 0)], []]
    for what, lists, message in refused:
        obs = MapObservations.from_lists(lists, gpu_ctx)
        try:
            with pytest.raises(ValueError, match=message):
                MapTables.from_observations(obs, fo, level)
        finally:
            obs.free()
        assert not alloc.live, what
        ok = MapObservations.from_lists(good, gpu_ctx)            # the context still serves
        t = MapTables.from_observations(ok, fo, level)
        assert t.frame_points().tolist() == [1, 0, 0, -1, -1]
        t.free()
        ok.free()
        assert not alloc.live, what
    # the library's own count on a table with both faults, in a block with a guard behind it: nothing lands outside
    lists = [[(0, 1), (1, 0)], [(0, 1), (1, 3)], [(5, 0)], [(1, 0)], [(1, 1 << 20)]]
    obs = MapObservations.from_lists(lists, gpu_ctx)
    want = frame_points_host(obs, fo)
    assert want[1:] == R.frame_points_ref(lists, fo)[1:] == (3, 2)
    held = [gpu_ctx.upload(fo), gpu_ctx.upload(np.full(5 * 4 + 256, 0xA5, np.uint8)), gpu_ctx.upload(np.full(256, 0xFF, np.uint8))]
    try:
        dev = obs._resident(gpu_ctx)
        s = (ctypes.c_int64 * 2)()
        local_map.check(gpu_ctx.lib.slam_lmap_frame_points(gpu_ctx.handle, len(lists), obs.nnz, dev["offsets"].ptr, dev["obs"].ptr, 2, held[0].ptr, 5,
                                                           held[1].ptr, held[2].ptr, s))
        assert (s[0], s[1]) == want[1:]
        assert _same(held[1].download(np.int32, (5,)), want[0]) and (held[1].download(np.uint8, (5 * 4 + 256,))[20:] == 0xA5).all()
        n = ctypes.c_int64(0)
        local_map.check(gpu_ctx.lib.slam_index_errors(gpu_ctx.handle, ctypes.byref(n)))
        assert n.value >= 3
    finally:
        for b in held:
            b.free()
        obs.free()
    empty = MapObservations.from_lists([[], []], gpu_ctx)          # nnz = 0: a table of -1
    t = MapTables.from_observations(empty, fo, level)
    assert t.frame_points().tolist() == [-1] * 5 and t.max_list == 0
    t.free()
    empty.free()
    assert not alloc.live


# ---- the vote ------------------------------------------------------------------------------------------------------------------
def _forms(F):
    lim = C.limits()
    return ["auto"] + (["lds16"] if F <= lim["vote_lds_small"] else []) + (["lds"] if F <= lim["vote_lds_frames"] else []) + ["global"]


@pytest.mark.parametrize("F", C.vote_sizes())
def test_votes_equal_host_and_reference_in_every_form(gpu_ctx, monkeypatch, F):
    from slamhip import local_keyframe_votes, votes_host

    s = C.vote_scene(F)
    blocks = Blocks(monkeypatch)
    with Resident(gpu_ctx, s) as t:
        for B in (1, 6) + ((70,) if F == 37 else ()):
            q = C.vote_queries(s, B)
            want = votes_host(t.obs, F, q, frame_removed=s.mask("removed"), point_bad=s.mask("bad"))
            assert _same_votes(want, R.votes_ref(s.lists, F, q, s.removed, s.bad))
            assert B == 1 or (want["skipped"] == 3 and want["votes"][:, F - 1].max() > 0)
            for form in _forms(F):
                runs = twice(blocks, lambda: local_keyframe_votes(t, q, form=form))
                assert all(_same_votes(got, want) for got in runs), (B, form)
        flat = np.concatenate(q)
        off = np.concatenate([[0], np.cumsum([len(x) for x in q])])
        assert _same_votes(local_keyframe_votes(t, flat, off), want)                    # the flat form of the same lists


def test_vote_tie_masks_and_empty_batches(gpu_ctx, monkeypatch):
    from slamhip import local_keyframe_votes, votes_host

    s = C.tie_scene()
    blocks = Blocks(monkeypatch)
    with Resident(gpu_ctx, s) as t:
        for form in _forms(s.F):
            for got in twice(blocks, lambda: local_keyframe_votes(t, [0, 1, 2], form=form)):
                assert got["best"].tolist() == [[2, 3]] and got["votes"].tolist() == [[0, 0, 3, 0, 0, 3, 0, 1, 0]] and got["nvoted"].tolist() == [3]
        t.remove_frame(2)                                             # a removed frame gets no vote: the tie is gone
        got = local_keyframe_votes(t, [[0, 1, 2], [3], []])
        assert got["best"].tolist() == [[5, 3], [8, 1], [-1, 0]] and got["votes"][:, 2].tolist() == [0, 0, 0]
        assert _same_votes(got, votes_host(t.obs, s.F, [[0, 1, 2], [3], []], frame_removed=t.frame_removed))
        bad = np.zeros(s.M, np.uint8)
        bad[2] = 1
        t.set_point_bad(bad)
        assert local_keyframe_votes(t, [2, 2, 3])["votes"].tolist() == [[0, 0, 0, 0, 0, 0, 0, 0, 1]]
        none = local_keyframe_votes(t, [])
        assert none["votes"].shape == (0, s.F) and none["best"].shape == (0, 2)


# ---- local points --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", C.points_sizes())
def test_local_points_equal_host_and_reference(gpu_ctx, monkeypatch, M):
    from slamhip import local_points, local_points_host

    s = C.points_scene(M)
    kfs, qs = C.points_queries(s)
    blocks = Blocks(monkeypatch)
    with Resident(gpu_ctx, s) as t:
        fp = t.frame_points()
        want = local_points_host(fp, s.frame_offsets, M, kfs, qs, frame_removed=s.mask("removed"), point_bad=s.mask("bad"))
        ref = R.local_points_ref(fp, s.frame_offsets, M, kfs, qs, s.removed, s.bad)
        assert all(_same(a, b) for a, b in zip(want, ref))
        assert len(want[0]) > M // 2 and len(want[1]) == 0 and len(want[2]) == 0          # the empty middle query, and all tracked
        for got in twice(blocks, lambda: local_points(t, kfs, qs)):
            assert len(got) == 3 and all(_same(a, b) for a, b in zip(got, want))
        # the last query with one point less tracked: its slice starts behind the empty one
        qs2 = [qs[0], qs[1], qs[2][qs[2] != (5 if M > 5 else 0)]]
        want2 = local_points_host(fp, s.frame_offsets, M, kfs, qs2, frame_removed=s.mask("removed"), point_bad=s.mask("bad"))
        got2 = local_points(t, kfs, qs2)
        assert all(_same(a, b) for a, b in zip(got2, want2)) and [len(x) for x in got2[1:]] == [0, 1]
        one = local_points(t, [0, 1], [3, 4])                         # one query, plain lists
        assert len(one) == 1 and _same(one[0], local_points_host(fp, s.frame_offsets, M, [0, 1], [3, 4], frame_removed=s.mask("removed"),
                                                                 point_bad=s.mask("bad"))[0])
        assert local_points(t, [], []) == []


# ---- keyframe culling ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lengths", "designed", "random"])
def test_redundancy_equals_host_and_reference(gpu_ctx, monkeypatch, name):
    from slamhip import keyframe_redundancy, keyframe_redundancy_host

    s = C.cull_scenes()[name]
    blocks = Blocks(monkeypatch)
    with Resident(gpu_ctx, s) as t:
        fp = t.frame_points()
        for cname, cand in C.candidate_sets(s).items():
            for th in (C.TH, 0, 2):
                want = keyframe_redundancy_host(t.obs, fp, s.level, s.frame_offsets, cand, th, s.mask("removed"), s.mask("bad"))
                ref = R.redundancy_ref(s.lists, fp, s.level, s.frame_offsets, cand, th, s.removed, s.bad)
                assert _same(want[0], ref[0]) and _same(want[1], ref[1])
                for counts, flags in twice(blocks, lambda: keyframe_redundancy(t, cand, th, return_flags=True)):
                    assert _same(counts, want[0]) and _same(flags, want[1]), (cname, th)          # the flags row by row
                assert _same(keyframe_redundancy(t, cand, th), want[0])
        # a shorter promise about the lists costs time, never a verdict: every class by the striding lanes of the first
        want = keyframe_redundancy_host(t.obs, fp, s.level, s.frame_offsets, None, C.TH, s.mask("removed"), s.mask("bad"))
        for promise in (0, 16, 17, 64, 65):
            t.max_list = promise
            counts, flags = keyframe_redundancy(t, None, C.TH, return_flags=True)
            assert _same(counts, want[0]) and _same(flags, want[1]), promise


def test_designed_boundaries_on_the_device(gpu_ctx):
    from slamhip import keyframe_redundancy

    s = C.cull_designed()
    n = s.notes
    with Resident(gpu_ctx, s) as t:
        c = keyframe_redundancy(t)
        assert c[n["exact"]].tolist() == [2, 1] and c[n["short"]].tolist() == [1, 0] and c[n["levels"]].tolist() == [2, 1]
        assert c[n["own"]].tolist() == [1, 0] and c[n["nine"]].tolist() == [10, 9] and c[n["ten"]].tolist() == [10, 10]
        assert c[n["removed"]].tolist() == [1, 0] and c[n["removed_candidate"]].tolist() == [0, 0]
        t.set_frame_removed(np.zeros(s.F, np.uint8))                   # frame 20 back: N crosses th_obs again
        c = keyframe_redundancy(t, [n["removed"], n["removed_candidate"]])
        assert c.tolist() == [[1, 1], [2, 2]]


def test_cull_keyframes_sequential_snapshot_and_protect(gpu_ctx):
    from slamhip import cull_keyframes

    s = C.cull_designed()
    n = s.notes
    a, b = n["twins"]
    with Resident(gpu_ctx, s) as t:
        def fresh():
            t.set_frame_removed(s.mask("removed"))
            t.cull_launches = 0

        def on_device():
            return np.flatnonzero(t.d_frame_removed.download(np.uint8, (s.F,))).tolist()

        fresh()
        assert cull_keyframes(t, [a, b]).tolist() == [a] and t.cull_launches == 2 and on_device() == [a, 20]       # removals + 1 launches
        assert np.flatnonzero(t.frame_removed).tolist() == [a, 20]
        fresh()
        assert cull_keyframes(t, [b, a]).tolist() == [b] and on_device() == [b, 20]                                 # the first in order goes
        fresh()
        assert cull_keyframes(t, [a, b], sequential=False).tolist() == [a, b] and t.cull_launches == 1 and on_device() == [a, b, 20]
        fresh()
        assert cull_keyframes(t, [a, b], protect=(0, a)).tolist() == [b] and on_device() == [b, 20]
        fresh()
        assert cull_keyframes(t, [n["nine"], n["ten"], n["exact"]]).tolist() == [n["ten"]] and t.cull_launches == 2   # 90 > 90 is false
        fresh()
        assert cull_keyframes(t, [n["nine"], n["own"]], ratio=(0, 1)).tolist() == [n["nine"]]
        fresh()
        assert cull_keyframes(t, [0, 20], ratio=(0, 1), protect=(0,)).tolist() == [] and on_device() == [20]         # protected, and removed already
        fresh()
        assert cull_keyframes(t, []).tolist() == [] and t.cull_launches == 0
        assert cull_keyframes(t, [n["exact"]], protect=None).tolist() == []                                          # nothing protected, nothing redundant
        fresh()
        got = cull_keyframes(t, None, sequential=False, protect=())
        assert a in got and b in got and n["ten"] in got and n["nine"] not in got and 20 not in got


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_nothing_behind(gpu_ctx, monkeypatch):
    from slamhip import SlamHipError, cull_keyframes, keyframe_redundancy, local_keyframe_votes, local_points

    s = C.vote_scene(C.limits()["vote_lds_small"] + 1)
    with Resident(gpu_ctx, s) as t:
        alloc = Allocations(gpu_ctx, monkeypatch)
        want = local_keyframe_votes(t, [0, 1, 2])

        def tampered(name, value):
            """``keyframe_redundancy`` with one field of the tables changed behind Python's own checks, and put back."""
            kept = getattr(t, name)
            setattr(t, name, value)
            try:
                return keyframe_redundancy(t, [0, 1], return_flags=True)
            finally:
                setattr(t, name, kept)

        refused = [("a form the frames do not fit", SlamHipError, lambda: local_keyframe_votes(t, [0], form="lds16")),
                   ("a list length no table has, met by the library behind the allocations", SlamHipError, lambda: tampered("max_list", 300)),
                   ("frame offsets that descend, met by the library behind the allocations", SlamHipError,
                    lambda: tampered("frame_offsets", np.ascontiguousarray(t.frame_offsets[::-1]))),
                   ("an unknown form", ValueError, lambda: local_keyframe_votes(t, [0], form="fast")),
                   ("lists that are no integers", ValueError, lambda: local_keyframe_votes(t, [[0.5]])),
                   ("offsets that do not end at the list", ValueError, lambda: local_keyframe_votes(t, [0, 1], [0, 1])),
                   ("not the tables", ValueError, lambda: local_keyframe_votes(s, [0])),
                   ("a keyframe list too few", ValueError, lambda: local_points(t, [[0]], [[0], [1]])),
                   ("a candidate past the frames", ValueError, lambda: keyframe_redundancy(t, [s.F])),
                   ("th_obs past a list", ValueError, lambda: keyframe_redundancy(t, None, 257)),
                   ("a ratio without a denominator", ValueError, lambda: cull_keyframes(t, [0], ratio=(1, 0))),
                   ("a protected frame that is none", ValueError, lambda: cull_keyframes(t, [0], protect=(s.F,)))]
        for what, error, call in refused:
            with pytest.raises(error):
                call()
            assert not alloc.live, what
            assert _same_votes(local_keyframe_votes(t, [0, 1, 2]), want), what          # the context still serves
            assert not alloc.live, what
        assert len(alloc.buffers) > 4 * len(refused)
    with pytest.raises(ValueError, match="freed"):
        local_keyframe_votes(t, [0])
    with pytest.raises(ValueError, match="freed"):
        keyframe_redundancy(t)


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_local_map_feeds_the_projection_search(gpu_ctx):
    """frame -> vote -> local keyframes -> local points -> search_by_projection: fed from the device tables and fed from the numpy
    statements, the search finds the same matches."""
    from backend import Backend
    from slamhip import CovisibilityTables, FrameGrids, PointSets, local_keyframes, local_points_host, search_by_projection, votes_host

    pts, fr, pose, row_of_point = PC.make_scene(77, 600, 300)
    rng = np.random.default_rng(9)
    K, M = 12, 600
    tracks = [sorted(set(int(k) for k in ((m // 60 + d) % K for d in range(int(rng.integers(1, 4)))))) for m in range(M)]
    s = C.from_tracks(K, tracks, 18, spare=2)
    tracked = np.r_[rng.choice(120, 60, replace=False), -1, -1]        # the frame tracks points of the first keyframes
    centre = -pose[:, :3].T @ pose[:, 3]
    fg = FrameGrids.from_arrays(fr["desc"], fr["xy"], fr["level"], PC.SIZE, ctx=gpu_ctx)
    with Resident(gpu_ctx, s) as t:
        cov = CovisibilityTables.from_observations(t.obs, K)
        try:
            graph = cov.graph()
        finally:
            cov.free()
        kfs, ref, ids = Backend().local_map(t, graph, tracked)
        votes = votes_host(t.obs, K, [tracked])
        h_kfs, h_ref = local_keyframes(votes, graph)
        h_ids = local_points_host(t.frame_points(), s.frame_offsets, M, [h_kfs], [tracked])[0]
        assert _same(kfs, h_kfs) and ref == h_ref == int(votes["best"][0, 0]) and _same(ids, h_ids)
        assert 100 < len(ids) < M and not set(ids) & set(tracked) and len(kfs) > int(votes["nvoted"][0])

        def search(idx):
            ps = PointSets(pts["xyz"][idx], pts["desc"][idx], dmin2=pts["range"][idx, 0], dmax2=pts["range"][idx, 1], normal=pts["normal"][idx],
                           ctx=gpu_ctx)
            try:
                return search_by_projection(ps, fg, [(0, 0)], [pose], [centre], PC.CAMERA, th=15.0, ctx=gpu_ctx)
            finally:
                ps.free()

        try:
            got, want = search(ids), search(h_ids)
        finally:
            fg.free()
        assert _same(got[0][0], want[0][0]) and np.array_equal(got[1], want[1])
        hit = got[0][0] >= 0
        assert hit.sum() > len(ids) // 2 and (row_of_point[ids[hit]] == got[0][0][hit]).mean() > 0.98
