"""One table of entry points that use a context block or a caller-owned workspace ("State contract of the context
blocks"), shared by tests/test_ctx_poison_gpu.py and tests/test_ctx_poison_cpu.py.

A case names the source file and the ``extern "C"`` function it enters, the call sites of ``slam_workspace``, ``slam_io_arena``
and ``radius_tables`` it runs through (``sites``: (callee, enclosing function) - the CPU test requires the sites of the table
and those of the sources to be the same multiset, so a new call site without a case fails there), the reference it is
compared with, and a builder that returns ``(call, check)``:

  ``call(ctx)``   runs the family's Python wrapper - the one its own GPU suite uses - and returns every output as host arrays
                  over their full documented extent, as a dict name -> array;
  ``check(outs)`` asserts that those outputs are what the family's reference or twin gives, with the tolerance the family's
                  suite uses (bit for bit wherever that suite is).

The inputs come from the families' case modules and from the helpers of their GPU suites (imported, not copied); every case
is the smallest shape at which its path still lives in the block, and ``call`` asserts that the path was taken.

``undefined``: the output elements a header leaves undefined, as (output name, mask function, quoted header line).  Exactly
those are masked before two runs are compared, and nothing else.  No case returns such an element today: every wrapper
downloads the documented extent only (the entries of a radius search up to its total, the rows of a candidate's range).

``before``: a larger call of the case's own family that the poisoned and the moved-workspace runs make first."""
import ctypes
import functools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam-experiments_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "slamhip.h")
POISON_BYTES = (0x00, 0xFF, 0x7F)


class Case:
    def __init__(self, name, file, entry, sites, reference, build, undefined=(), bf=False, before=None):
        self.name, self.file, self.entry, self.sites, self.reference = name, file, entry, tuple(sites), reference
        self._build, self.undefined, self.bf = build, tuple(undefined), bf
        self.before = before            # a larger call of the case's own family that lays the block out differently (or None)

    @functools.cached_property
    def built(self):
        """(call, check), built once: the inputs and the reference are computed once and left unchanged."""
        return self._build()

    def call(self, ctx):
        outs = self.built[0](ctx)
        return {k: np.ascontiguousarray(v) for k, v in outs.items()}

    def check(self, outs):
        self.built[1](outs)

    def masked(self, outs):
        """The outputs with the elements the header leaves undefined set to zero."""
        outs = {k: v.copy() for k, v in outs.items()}
        for name, where, _line in self.undefined:
            outs[name][where(outs)] = 0
        return outs


def same(a, b):
    """Every output equal bit for bit: dtype, shape and bytes."""
    assert sorted(a) == sorted(b), (sorted(a), sorted(b))
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape, (k, x.dtype, y.dtype, x.shape, y.shape)
        if x.tobytes() != y.tobytes():
            bad = np.flatnonzero(x.reshape(-1).view(np.uint8) != y.reshape(-1).view(np.uint8))
            raise AssertionError(f"output {k!r}: {bad.size} bytes differ, first at byte {bad[0]} of {x.nbytes}")


def index_errors(ctx):
    n = ctypes.c_int64(-1)
    assert ctx.lib.slam_index_errors(ctx.handle, ctypes.byref(n)) == 0
    return n.value


def _rows(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def _cat(parts, tail=(), dtype=np.float64):
    parts = [np.asarray(p, dtype).reshape((-1,) + tuple(tail)) for p in parts]
    return np.concatenate(parts) if parts else np.zeros((0,) + tuple(tail), dtype)


# =============================================================== the searches ================================================
def _top2_chunks(engine):
    """Top-2 Hamming search with the chunk knob forcing several chunks, so the partial bests are merged (engine 1, 2 or 3)."""
    def build():
        from oracle import oracle
        rng = np.random.default_rng(9100 + engine)
        n, m = 300, 2100                                         # more than one query block, a train set that is no multiple of the chunk
        q, t = _rows(rng, n), _rows(rng, m)
        t[5] = t[1900]
        q[10] = t[1900]                                          # a tie across two chunks: the lowest index wins
        want = oracle.bf_knn_c(q, t, 2)

        def call(ctx):
            import slamhip
            ctx.set_engine(engine)
            ctx.set_tuning(chunk=512)
            try:
                assert ctx.plan_info(n, m)["chunks"] >= 2
                if engine in (2, 3):
                    assert slamhip.mx_tile_describe(n, m, engine) == (16 if engine == 2 else 32)
                dq, dt = slamhip.DeviceDescriptors(ctx, q), slamhip.DeviceDescriptors(ctx, t)
                tab = slamhip.Top2Table(ctx, n)
                try:
                    slamhip.knn2_device(ctx, dq.buf, n, dt.buf, m, tab.idx, tab.dist)
                    idx, dist = tab.download()
                finally:
                    for o in (tab, dq, dt):
                        o.free()
            finally:
                ctx.set_tuning()
                ctx.set_engine(0)
            return dict(idx=idx, dist=dist)

        def check(o):
            assert np.array_equal(o["idx"], want[0]) and np.array_equal(o["dist"], want[1])
            assert o["idx"][10, 0] == 5 and o["dist"][10, 0] == 0
        return call, check
    return build


def _top2_passes():
    """A train set of more than 2^23 rows: the per-pass tables live in the workspace and slam_bf_merge_top2 reads them."""
    from oracle import oracle
    rng = np.random.default_rng(9104)
    n, m = 3, (1 << 23) + 77
    block = _rows(rng, 1 << 16)
    t = np.ascontiguousarray(np.tile(block, (m // len(block) + 1, 1))[:m])
    t[:, 0] ^= (np.arange(m) >> 16).astype(np.uint8)             # the copies of the block differ in their first byte
    q = np.stack([t[17], t[(1 << 23) + 5], _rows(rng, 1)[0]])
    want = oracle.bf_knn_c(q, t, 2, threads=16)

    def call(ctx):
        import slamhip
        dq, dt = slamhip.DeviceDescriptors(ctx, q), slamhip.DeviceDescriptors(ctx, t)
        tab = slamhip.Top2Table(ctx, n)
        try:
            slamhip.knn2_device(ctx, dq.buf, n, dt.buf, m, tab.idx, tab.dist)
            idx, dist = tab.download()
        finally:
            for o in (tab, dq, dt):
                o.free()
        assert ctx.block_bytes()["workspace"] >= 2 * 2 * n * 2 * 4
        return dict(idx=idx, dist=dist)

    def check(o):
        assert np.array_equal(o["idx"], want[0]) and np.array_equal(o["dist"], want[1])
        assert o["idx"][0, 0] == 17 and o["idx"][1, 0] == (1 << 23) + 5 and (o["dist"][:2, 0] == 0).all()
    return call, check


def _topk(host):
    """Top-k with k = 5 over several chunks: the partial tables of the chunks live in the workspace (plan "ws" > 0)."""
    def build():
        from oracle import oracle
        rng = np.random.default_rng(9110 + host)
        n, m, k = 70, 3000, 5
        q, t = _rows(rng, n), _rows(rng, m)
        t[2500] = t[3]
        want = oracle.bf_knn_c(q, t, k)

        def call(ctx):
            import slamhip
            plan = slamhip.plan_describe_topk(n, m, k, num_cu=ctx.plan_info(n, m)["cus"])
            assert plan["chunks"] >= 2 and plan["workspace_bytes"] > 0, plan
            if host:
                idx, dist = slamhip.topk_match_arrays(q, t, k, ctx=ctx)
            else:
                from test_topk_gpu import device_topk
                idx, dist = device_topk(ctx, q, t, k)
            return dict(idx=idx, dist=dist)

        def check(o):
            assert np.array_equal(o["idx"], want[0]) and np.array_equal(o["dist"], want[1])
        return call, check
    return build


def _window(host):
    """The window search: every table of its binning lives in the workspace (the plan reports its bytes)."""
    def build():
        from hamming_families import ref_window
        rng = np.random.default_rng(9120 + host)
        n, m, k = 130, 300, 2
        q, t = _rows(rng, n), _rows(rng, m)
        qxy, txy = rng.uniform(0, 64, (n, 2)).astype(np.float32), rng.uniform(0, 64, (m, 2)).astype(np.float32)
        qxy[7] = (1000.0, 1000.0)                                # a query with an empty window: (-1, INT32_MAX) twice
        want = ref_window(q, t, qxy, txy, 6.0, k)

        def call(ctx):
            import slamhip
            assert slamhip.plan_describe_window(n, m)["workspace_bytes"] > 0
            if host:
                idx, dist = slamhip.window_match_arrays(q, t, qxy, txy, 6.0, k, ctx=ctx)
            else:
                from test_window_gpu import run_device
                idx, dist = run_device(ctx, q, t, qxy, txy, 6.0, k)
            return dict(idx=idx, dist=dist)

        def check(o):
            assert np.array_equal(o["idx"], want[0]) and np.array_equal(o["dist"], want[1])
            assert o["idx"][7].tolist() == [-1, -1] and (o["dist"][7] == 2**31 - 1).all()
        return call, check
    return build


def _radius(kind):
    """The radius search. "short": every list at most SLAM_RADIUS_SHORT entries, on device rows; "long": one list above it
    (lq_id, lq_tile_end and the tile histograms are used), through the host entry and the io arena; "total": capacity 0, only
    the offsets and the total come back."""
    def build():
        import slamhip
        from hamming_families import ref_radius
        short = slamhip.plan_describe_radius(1, 1)["short_max"]
        rng = np.random.default_rng(9130)
        n, m, r = 70, 2 * short + 300, 6.0
        q, t = _rows(rng, n), _rows(rng, m)
        if kind == "long":
            for j in range(short + 40):                          # query 3 gets a list longer than one tile: rows at distance j % 5
                t[7 + j] = q[3]
                t[7 + j, j % 32] ^= np.uint8((1 << (j % 5)) - 1)
        t[m - 1] = q[60]
        t[0] = q[60]
        off, idx, dist = ref_radius(q, t, (r,))[r]
        assert (np.diff(off).max() > short) == (kind == "long") and off[-1] > 1

        def call(ctx):
            if kind == "long":
                o, i, d = slamhip.radius_match_arrays(q, t, r, ctx=ctx)
                return dict(offsets=o, idx=i, dist=d)
            from test_radius_gpu import Csr
            cap = 0 if kind == "total" else int(off[-1])
            dq, dt, out = slamhip.DeviceDescriptors(ctx, q), slamhip.DeviceDescriptors(ctx, t), Csr(ctx, n, cap)
            try:
                total = slamhip.radius_device(ctx, dq.buf, n, dt.buf, m, r, out.off, cap, out.idx if cap else None, out.dist if cap else None)
                o, i, d = out.download(total if cap else 0)
            finally:
                for x in (out, dq, dt):
                    x.free()
            return dict(offsets=o, idx=i, dist=d, total=np.array([total], np.int64))

        def check(o):
            assert np.array_equal(o["offsets"], off)
            if kind == "total":
                assert o["total"][0] == off[-1] and len(o["idx"]) == 0
            else:
                assert np.array_equal(o["idx"], idx) and np.array_equal(o["dist"], dist)
        return call, check
    return build


# =============================================================== the RANSAC families =========================================
def _ransac(family):
    """B = 3 candidates with an empty one in the middle and one below the minimal sample at the end, H = 70 hypotheses (no
    multiple of a wave or a block), against the family's twin per candidate, bit for bit."""
    def build():
        H, seed = 70, 5
        if family == "two_view":
            import two_view_ref as ref
            from oracle import oracle
            sc = ref.make_scene(np.random.default_rng(9201), 60, 0.5, 0.3)
            a, b = sc["px1"], sc["px2"]
            cands = [(a, b), (a[:0], b[:0]), (a[:4], b[:4])]
            twin = [oracle.tv_twin_ransac(x, y, ref.EUROC, H, 1.0, seed) for x, y in cands]

            def run(ctx):
                import slamhip
                E, masks, st = slamhip.find_essential_batch(cands, ref.EUROC, H, 1.0, seed, ctx=ctx)
                return E.reshape(3, 9), masks, st
        elif family == "homography":
            import hg_twin as tw
            import homography_ref as hr
            sc = hr.scenes_planar_noisy(seed=4, n=60)[1]
            a, b = sc["px1"], sc["px2"]
            cands = [(a, b), (a[:0], b[:0]), (a[:3], b[:3])]
            twin = [tw.ransac(x, y, H, 3.0, seed) for x, y in cands]

            def run(ctx):
                import slamhip
                Hm, masks, st = slamhip.find_homography_batch(cands, H, 3.0, seed, ctx=ctx)
                return Hm.reshape(3, 9), masks, st
        elif family == "pnp":
            import pnp_ref as ref
            import pnp_twin as tw
            sc = ref.make_scene(np.random.default_rng(9203), 60, 0.5, 0.3)
            a, b = sc["X"], sc["px"]
            cands = [(a, b), (a[:0], b[:0]), (a[:2], b[:2])]
            twin = [tw.ransac(x, y, ref.EUROC, H, 8.0, seed) for x, y in cands]

            def run(ctx):
                import slamhip
                poses, masks, _counts, st, _ = slamhip.solve_pnp_ransac_batch(cands, ref.EUROC, H, 8.0, seed, refine=False, ctx=ctx)
                return poses.reshape(3, 12), masks, st
        else:
            import sim3_ref as ref
            import sim3_twin as tw
            sc = ref.make_scene(np.random.default_rng(9204), 60, 1.3, 0.001, 0.3)
            a, b = sc["X1"], sc["X2"]
            cands = [(a, b), (a[:0], b[:0]), (a[:2], b[:2])]
            twin = [tw.ransac(x, y, ref.EUROC, H, ref.CHI2, seed) for x, y in cands]

            def run(ctx):
                import slamhip
                s, R, t, masks, st, rs = slamhip.estimate_sim3_batch(cands, ref.EUROC, H, ref.CHI2, False, seed, refit=False, ctx=ctx)
                assert rs is None
                return np.stack([ref.pack(s[i], R[i], t[i]) for i in range(3)]), masks, st

        def call(ctx):
            model, masks, st = run(ctx)
            return dict(model=np.asarray(model, np.float64), mask=_cat(masks, (), np.uint8), stats=np.asarray(st, np.int32))

        def check(o):
            assert o["stats"][0, 0] >= 5 and o["stats"][0, 3] > 0          # the first candidate has a model that counts inliers
            assert o["stats"][1].tolist() == [0, -1, -1, 0] and o["stats"][2].tolist() == [0, -1, -1, 0]      # "no model"
            for i, (m, mask, st) in enumerate(twin):
                assert o["model"][i].tobytes() == np.ascontiguousarray(m, np.float64).reshape(-1).tobytes(), i
                assert o["stats"][i].tolist() == np.asarray(st).tolist(), i
            assert np.array_equal(o["mask"], _cat([t[1] for t in twin], (), np.uint8))
        return call, check
    return build


# =============================================================== the matchers ================================================
def _proj_inputs():
    """Two point sets and three frames: the pairs (0, 0) and (1, 0) share frame 0; point 9 of set 0 sits where point 8 does
    and is nearer to the row that point 8 matches (a contested row: the claim words decide); frame 1 is empty; set 2 is
    empty."""
    import proj_match_cases as C
    import test_proj_match_gpu as T
    rng = np.random.default_rng(9301)
    p0, f0, pose, row_of = C.make_scene(9302, 70, n_clutter=30)
    p0["desc"][9] = C.flip_bits(rng, f0["desc"][row_of[8]:row_of[8] + 1], 1)[0]
    for k in ("xyz", "range", "normal", "level", "bins"):
        p0[k][9] = p0[k][8]
    p1 = {k: v[5:45].copy() for k, v in p0.items()}
    empty_p = {k: v[:0].copy() for k, v in p0.items()}
    empty_f = {k: v[:0].copy() for k, v in f0.items()}
    f2 = T.features(rng, 65, bins=True)
    pts, frames = [p0, p1, empty_p], [f0, empty_f, f2]
    pairs = [(0, 0), (1, 0), (0, 1), (2, 2), (1, 2)]
    poses = [pose] * len(pairs)
    centres = [-pose[:, :3].T @ pose[:, 3]] * len(pairs)
    return C, T, pts, frames, pairs, poses, centres, int(row_of[8])


def _proj_search(tables):
    def build():
        import proj_match_ref as R
        C, T, pts, frames, pairs, poses, centres, contested = _proj_inputs()
        kw = dict(ratio=1.0, th_high=256)
        want = [R.search(pts[a], frames[b], poses[p], centres[p], 6.0, C.CAMERA, C.BOUNDS, *T.S12, **kw) for p, (a, b) in enumerate(pairs)]
        assert want[0][2]["idx"][8, 0] == contested and want[0][2]["idx"][9, 0] == contested and want[0][0][8] == -1 and want[0][0][9] == contested

        def call(ctx):
            from slamhip import proj_match as pm
            ps, fg = T.upload(pm, ctx, pts, frames)
            try:
                got = pm.search_by_projection(ps, fg, pairs, poses, centres, C.CAMERA, C.BOUNDS, T.S12, 6.0, return_tables=tables, ctx=ctx, **kw)
            finally:
                ps.free()
                fg.free()
            out = dict(matches=_cat(got[0], (), np.int32), counts=got[1])
            if tables:
                for k, dt, tail in (("status", np.int32, ()), ("u", np.float64, ()), ("v", np.float64, ()), ("lp", np.int32, ()),
                                    ("idx", np.int32, (2,)), ("dist", np.int32, (2,))):
                    out[k] = _cat([t[k] for t in got[2]], tail, dt)
            return out

        def check(o):
            assert np.array_equal(o["matches"], _cat([w[0] for w in want], (), np.int32)) and o["counts"].tolist() == [w[1] for w in want]
            assert o["counts"][0] > 20 and o["counts"][2] == 0 and o["counts"][3] == 0
            assert o["matches"][8] == -1 and o["matches"][9] == contested               # the nearer point keeps the row
            if tables:
                for k in ("status", "u", "v", "lp", "idx", "dist"):
                    assert C.same_bits(o[k], _cat([w[2][k] for w in want], o[k].shape[1:], o[k].dtype)), k
        return call, check
    return build


def _proj_project():
    import proj_match_ref as R
    C, T, pts, frames, pairs, poses, centres, _ = _proj_inputs()
    sets = [0, 2, 1]
    want = [R.gates(pts[a]["xyz"], poses[0], centres[0], 6.0, C.CAMERA, C.BOUNDS, *T.S12, rng=pts[a]["range"], normal=pts[a]["normal"]) for a in sets]

    def call(ctx):
        from slamhip import proj_match as pm
        ps, fg = T.upload(pm, ctx, pts, [])
        try:
            got = pm.project_points(ps, sets, poses[:3], centres[:3], C.CAMERA, C.BOUNDS, T.S12, 6.0, ctx=ctx)
        finally:
            ps.free()
            fg.free()
        return {k: _cat([g[k] for g in got], (), dt) for k, dt in (("status", np.int32), ("u", np.float64), ("v", np.float64), ("lp", np.int32))}

    def check(o):
        for i, k in enumerate(("status", "u", "v")):
            assert C.same_bits(o[k], _cat([w[i] for w in want], (), o[k].dtype)), k
        assert C.same_bits(o["lp"], _cat([w[3] for w in want], (), np.int32))
        assert (o["status"] == 0).sum() > 50 and np.isnan(o["u"][o["status"] == 1]).all()
    return call, check


def _proj_grid():
    """slam_proj_match_grid on two frames, the first empty: the sorted copies against a stable sort by cell stated here."""
    import proj_match_cases as C
    import test_proj_match_gpu as T
    rng = np.random.default_rng(9303)
    f = T.features(rng, 150, taken=True)
    f["xy"][:4] = [(0.0, 0.0), (639.999, 479.999), (640.0, 10.0), (-1.0, 5.0)]        # the corners, and two rows outside the image
    empty = {k: v[:0].copy() for k, v in f.items()}
    cell, (W, H) = 16, C.SIZE
    gw, gh = -(-W // cell), -(-H // cell)
    x, y = f["xy"][:, 0].astype(np.float64), f["xy"][:, 1].astype(np.float64)
    cells = (np.clip(np.floor(y / cell), 0, gh - 1) * gw + np.clip(np.floor(x / cell), 0, gw - 1)).astype(np.int32)      # clamped into the grid

    def call(ctx):
        from slamhip import proj_match as pm
        ps, fg = T.upload(pm, ctx, [], [empty, f])
        try:
            out = dict(cells=fg.cells, order=fg.order, cells_sorted=fg.cells_sorted, desc_sorted=fg.descriptors_sorted, xy_sorted=fg.xy_sorted)
        finally:
            ps.free()
            fg.free()
        return out

    def check(o):
        assert np.array_equal(o["cells"], cells)
        order = np.argsort(cells, kind="stable").astype(np.int32)          # by cell, the rows of one cell in row order
        assert np.array_equal(o["order"], order) and np.array_equal(o["cells_sorted"], cells[order])
        assert np.array_equal(o["desc_sorted"], f["desc"][order]) and np.array_equal(o["xy_sorted"], f["xy"][order])
    return call, check


def _bow_inputs():
    """Side 1: two images and an empty one; side 2: one image both share, and an empty one.  Rows 0 and 1 of the first
    side-1 image are copies of side-2 row 4 but for three bits and one bit: a contested row."""
    import test_bow_match_gpu as T
    rng = np.random.default_rng(9401)
    d2, n2 = _rows(rng, 90), rng.integers(0, 4, 90)
    mk = lambda n: (T.noisy(rng, d2[rng.integers(0, 90, n)], 4), rng.integers(0, 4, n))  # noqa: E731
    a, b = mk(70), mk(65)
    for row, flips in ((0, 3), (1, 1)):
        a[0][row] = d2[4]
        a[0][row, :flips] ^= 1
        a[1][row] = n2[4]
    images1 = [a, b, (np.zeros((0, 32), np.uint8), np.zeros(0, np.int64))]
    images2 = [(d2, n2), (np.zeros((0, 32), np.uint8), np.zeros(0, np.int64))]
    pairs = [(0, 0), (2, 0), (0, 1), (1, 0)]                    # (the empty pairs are not the last: the last rows of every table are live)
    return T, images1, images2, pairs


def _bow_search(tables):
    def build():
        import bow_match_ref as R
        T, images1, images2, pairs = _bow_inputs()
        kw = dict(th_low=256, ratio=1.0)
        want = [R.search(images1[a][0], images1[a][1], images2[b][0], images2[b][1], None, None, **kw) for a, b in pairs]
        assert want[0][2][0][0, 0] == 4 and want[0][2][0][1, 0] == 4 and want[0][0][:2].tolist() == [-1, 4]      # the nearer row keeps it

        def call(ctx):
            from slamhip import bow_match as bm
            fv1, fv2 = T.make_set(bm, ctx, images1), T.make_set(bm, ctx, images2)
            try:
                got = bm.search_by_bow(fv1, fv2, pairs, None, None, return_tables=tables, ctx=ctx, **kw)
            finally:
                fv1.free()
                fv2.free()
            out = dict(matches=_cat(got[0], (), np.int32), counts=got[1])
            if tables:
                out["idx"], out["dist"] = _cat([t[0] for t in got[2]], (2,), np.int32), _cat([t[1] for t in got[2]], (2,), np.int32)
            return out

        def check(o):
            assert np.array_equal(o["matches"], _cat([w[0] for w in want], (), np.int32)) and o["counts"].tolist() == [w[1] for w in want]
            assert o["counts"][0] > 20 and o["counts"][1] == 0 and o["counts"][2] == 0 and o["counts"][3] > 20
            if tables:
                assert np.array_equal(o["idx"], _cat([w[2][0] for w in want], (2,), np.int32))
                assert np.array_equal(o["dist"], _cat([w[2][1] for w in want], (2,), np.int32))
        return call, check
    return build


def _bow_group():
    """slam_bow_match_group: the sorted copies of three images, the middle one empty."""
    T, images1, images2, pairs = _bow_inputs()
    images = [images1[0], images1[2], images1[1]]
    desc, nodes = np.concatenate([i[0] for i in images]), np.concatenate([i[1] for i in images]).astype(np.int64)

    def call(ctx):
        from slamhip import bow_match as bm
        fv = T.make_set(bm, ctx, images)
        try:
            return dict(order=fv.order, nodes_sorted=fv.nodes_sorted, desc_sorted=fv.descriptors_sorted)
        finally:
            fv.free()

    def check(o):
        n0 = len(images[0][1])
        local = [np.argsort(nodes[:n0], kind="stable"), np.argsort(nodes[n0:], kind="stable")]        # the order holds rows of the image
        rows = np.concatenate([local[0], n0 + local[1]])
        assert np.array_equal(o["order"], np.concatenate(local)) and np.array_equal(o["nodes_sorted"], nodes[rows])
        assert np.array_equal(o["desc_sorted"], desc[rows])
    return call, check


def _tri_inputs():
    import tri_match_cases as C
    a, s2 = C.random_pair(9501, 70, 90, n_nodes=3, pool=C.POOL)
    b, _ = C.random_pair(9502, 65, 1, n_nodes=3, pool=C.POOL)
    for row, flips in ((0, 3), (1, 1)):                          # rows 0 and 1 of the first image want side-2 row 4: a contested row
        a["desc"][row] = s2["desc"][4]
        a["desc"][row, :flips] ^= 1
        a["nodes"][row], a["xy"][row], a["level"][row] = max(int(s2["nodes"][4]), 0), s2["xy"][4] + np.float32([50 + row, 0]), 2
        a["taken"][row] = 0
    s2["nodes"][4], s2["taken"][4] = max(int(s2["nodes"][4]), 0), 0
    e1, e2 = C.random_pair(9503, 0, 0, n_nodes=3, pool=C.POOL)
    return C, [a, b, e1], [s2, e2], [(0, 0), (2, 0), (0, 1), (1, 0)]


def _tri_search(tables):
    def build():
        import tri_match_ref as R
        import test_tri_match_gpu as T
        C, images1, images2, pairs = _tri_inputs()
        want = [R.search(images1[a], images2[b], C.F_RECT, C.NO_EPIPOLE, C.SCALE, C.SIGMA2, th_low=256) for a, b in pairs]
        assert want[0][2][0][0, 0] == 4 and want[0][2][0][1, 0] == 4 and want[0][0][:2].tolist() == [-1, 4]

        def call(ctx):
            from slamhip import tri_match as tm
            f1, v1, _ = T.make_set(tm, ctx, images1)
            f2, v2, _ = T.make_set(tm, ctx, images2)
            P = len(pairs)
            try:
                got = tm.search_for_triangulation(f1, f2, pairs, v1, v2, np.broadcast_to(C.F_RECT, (P, 3, 3)), np.broadcast_to(C.NO_EPIPOLE, (P, 2)),
                                                  (C.SCALE, C.SIGMA2), None, None, return_tables=tables, ctx=ctx, th_low=256)
            finally:
                for x in (f1, v1, f2, v2):
                    x.free()
            out = dict(matches=_cat(got[0], (), np.int32), counts=np.asarray(got[1], np.int32))
            if tables:
                out["idx"], out["dist"] = _cat([t[0] for t in got[2]], (2,), np.int32), _cat([t[1] for t in got[2]], (2,), np.int32)
            return out

        def check(o):
            assert np.array_equal(o["matches"], _cat([w[0] for w in want], (), np.int32)) and o["counts"].tolist() == [w[1] for w in want]
            assert o["counts"][0] > 5 and o["counts"][1] == 0 and o["counts"][2] == 0 and o["counts"][3] > 5
            if tables:
                assert np.array_equal(o["idx"], _cat([w[2][0] for w in want], (2,), np.int32))
                assert np.array_equal(o["dist"], _cat([w[2][1] for w in want], (2,), np.int32))
        return call, check
    return build


def _tri_triangulate():
    """slam_tri_match_triangulate on the 300-match scene cut to 70 rows, two pairs sharing side 2 and an empty pair, against
    the host twin of csrc/tri_point.h."""
    import test_tri_match_gpu as T
    import tri_match_cases as C
    import tri_match_twin as TW
    s1, s2, _, truth = C.make_scene(9504, 70, 70)
    m12 = np.full(70, -1, np.int32)
    m12[truth["rows1"]] = truth["rows2"]
    m12[::9] = -1
    m12[5] = 70                                                  # out of range: status 1, no read
    s1b = {k: v[:65].copy() for k, v in s1.items()}
    empty = {k: v[:0].copy() for k, v in s1.items()}
    images1, images2, pairs = [s1, empty, s1b], [s2], [(0, 0), (1, 0), (2, 0)]
    matches = [m12, m12[:0], np.minimum(m12[:65], 69)]
    T1, T2 = C.POSES[0], C.POSES[1]

    def call(ctx):
        from slamhip import tri_match as tm
        f1, v1, _ = T.make_set(tm, ctx, images1)
        f2, v2, _ = T.make_set(tm, ctx, images2)
        try:
            pts, created = tm.triangulate_matches(f1, f2, pairs, v1, v2, matches, np.stack([T1] * 3), np.stack([T2] * 3), C.CAMERA,
                                                  (C.SCALE, C.SIGMA2), ctx=ctx)
        finally:
            for x in (f1, v1, f2, v2):
                x.free()
        out = {k: _cat([p[k] for p in pts], tail, dt) for k, tail, dt in (("X", (3,), np.float64), ("normal", (3,), np.float64),
                                                                          ("dmin2", (), np.float64), ("dmax2", (), np.float64), ("status", (), np.int32))}
        out["created"] = np.asarray(created, np.int32)
        return out

    def check(o):
        from slamhip.proj_match import camera_centres
        O1, O2 = camera_centres(T1[None])[0], camera_centres(T2[None])[0]
        at = 0
        for (a, b), m in zip(pairs, matches):
            n = len(m)
            has = (m >= 0) & (m < 70)
            st = o["status"][at:at + n]
            assert (st[~has] == 1).all()
            if has.any():
                w = TW.triangulate_centres(T1, T2, O1, O2, C.CAMERA, C.SCALE, C.SIGMA2, images1[a]["xy"][has], s2["xy"][m[has]], images1[a]["level"][has],
                                           s2["level"][m[has]])
                assert st[has].tolist() == w["status"].tolist()
                for k in ("X", "normal", "dmin2", "dmax2"):
                    assert T.same_bits(o[k][at:at + n][has], w[k]), k
            for k in ("X", "normal", "dmin2", "dmax2"):
                assert np.isnan(o[k][at:at + n][st != 0]).all()
            assert o["created"][pairs.index((a, b))] == (st == 0).sum()
            at += n
        assert o["created"][0] > 30 and o["created"][1] == 0
    return call, check


def _fuse_search(tables):
    """slam_fuse_search on the world of the fusion suite: ten pairs, several sharing a frame, an empty set and an empty frame,
    and one more set in which two map points sit on one landmark's feature (a contested row)."""
    def build():
        import fuse_cases as C
        import test_fuse_gpu as T
        W = C.world(21, 65, n_frames=3, n_dup=5, n_clutter=10)
        idx, sets, frames, poses, centres, pairs = T.world_case(W)
        free = [m for m in range(5, 65) if not any(f == 1 for f, _ in W["lists"][m])][:2]       # two landmarks frame 1 does not observe
        twin = C.subset(W["pts"], free)
        for k in ("xyz", "range", "normal"):
            twin[k][1] = twin[k][0]
        row = int(W["row_of"][1][free[0]])
        twin["desc"][0] = C.flip_bits(np.random.default_rng(3), frames[1]["desc"][row:row + 1], 3)[0]
        twin["desc"][1] = C.flip_bits(np.random.default_rng(4), frames[1]["desc"][row:row + 1], 1)[0]
        sets, pairs = sets + [twin], pairs + [(5, 1)]
        A, O = poses[[b for _, b in pairs]], centres[[b for _, b in pairs]]
        want = T.world_ref(W, sets, frames, poses, centres, pairs)
        assert want[-1]["row"].tolist() == [row, row] and want[-1]["status"].tolist() == [8, 0]      # both want the row; the nearer one holds the claim
        keys = ("row", "dist", "status", "other") + (("u", "v", "lp") if tables else ())

        def call(ctx):
            from slamhip import FrameGrids, PointSets
            from slamhip import fuse as fz
            if tables:
                res, cnt = T.run(fz, ctx, sets, frames, W["lists"], pairs, A, O)
            else:                                                # T.run asks for the tables; the same call without them
                off1 = np.concatenate([[0], np.cumsum([len(x["id"]) for x in sets])]).astype(np.int64)
                off2 = np.concatenate([[0], np.cumsum([len(f["level"]) for f in frames])]).astype(np.int64)
                rng = T.cat(sets, "range", (2,), np.float64)
                ps = PointSets(T.cat(sets, "xyz", (3,), np.float64), T.cat(sets, "desc", (32,), np.uint8), off1, dmin2=rng[:, 0], dmax2=rng[:, 1],
                               normal=T.cat(sets, "normal", (3,), np.float64), ctx=ctx)
                fr = ob = None
                try:
                    fr = FrameGrids.from_arrays(T.cat(frames, "desc", (32,), np.uint8), T.cat(frames, "xy", (2,), np.float32),
                                                T.cat(frames, "level", (), np.int64), C.SIZE, off2, ctx=ctx)
                    ob = fz.MapObservations.from_lists(W["lists"], ctx)
                    res, cnt = fz.fuse_points(ps, T.cat(sets, "id", (), np.int64), fr, T.cat(frames, "point", (), np.int64), ob, pairs, A, O,
                                              camera=C.CAMERA, scale=(C.SCALE, C.SCALE2), ctx=ctx)
                finally:
                    for x in (ps, fr, ob):
                        if x is not None:
                            x.free()
            out = {k: _cat([r[k] for r in res], (), np.float64 if k in "uv" else np.int32) for k in keys}
            out["count"] = np.asarray(cnt, np.int32)
            return out

        def check(o):
            for k in keys:
                w = _cat([x[k] for x in want], (), o[k].dtype)
                assert o[k].tobytes() == w.tobytes(), k
            assert np.array_equal(o["count"], np.stack([x["count"] for x in want]))
            assert o["count"][0].tolist() == [0, 0, 0] and o["count"][:, 0].sum() > 0
        return call, check
    return build


def _fuse_refresh():
    """slam_fuse_refresh with lists of 0, 1, 3, 16, 17, 64, 65 and 70 observations (all three kernels) over 70 frames of 2 rows."""
    import fuse_cases as C
    import fuse_ref as F
    rng = np.random.default_rng(9601)
    B = 70
    seeds = _rows(rng, 4)
    desc = [C.flip_bits(rng, seeds[rng.integers(0, 4, 2)], 5) for _ in range(B)]
    level = [rng.integers(0, 8, 2) for _ in range(B)]
    centres = rng.normal(0, 1, (B, 3))
    lens = [0, 1, 3, 16, 17, 64, 65, 70, 2]
    lists = [[(int(f), int(rng.integers(0, 2))) for f in np.sort(rng.choice(B, n, replace=False))] for n in lens]
    xyz = rng.normal(0, 1, (len(lens), 3)) + np.array([0, 0, 8.0])
    xyz[8] = np.nan
    ref = np.array([rng.integers(0, max(n, 1)) for n in lens])
    want = F.refresh(xyz, lists, desc, level, centres, C.SCALE, ref)

    def call(ctx):
        from slamhip import fuse as fz
        from test_fuse_gpu import frames_of
        fr = frames_of(ctx, desc, level)
        ob = fz.MapObservations.from_lists(lists, ctx)
        try:
            got = fz.refresh_map_points(xyz, ob, fr, centres, ref, (C.SCALE, C.SCALE2), ctx=ctx)
        finally:
            fr.free()
            ob.free()
        return {k: np.asarray(got[k]) for k in ("best", "descriptors", "normal", "dmin2", "dmax2")}

    def check(o):
        assert np.array_equal(o["best"], want["best"]) and np.array_equal(o["descriptors"], want["descriptors"])
        for k in ("normal", "dmin2", "dmax2"):
            assert np.ascontiguousarray(o[k], np.float64).tobytes() == np.ascontiguousarray(want[k], np.float64).tobytes(), k
        assert o["best"][0] == -1 and not o["descriptors"][0].any() and np.isnan(o["normal"][0]).all() and np.isnan(o["dmin2"][8])
    return call, check


# =============================================================== the graph solvers ===========================================
def _graph(kind, host):
    """``host``: the whole optimisation through slam_*_optimize_host_f64 on the family's smallest scene, against the
    reference's direct LM within the suite's yardsticks; else the PCG of slam_*_pcg_f64 on the same scene (glm_blocks),
    held to the tolerance it was asked for.  One fixed vertex, more than two PCG iterations (asserted)."""
    def build():
        if kind == "pg":
            import pose_graph_ref as R
            import test_pose_graph_cpu as TC
            import test_pose_graph_gpu as TG
            name, N = "loop_closure", 6
        else:
            import sim3_graph_ref as R
            import test_sim3_graph_cpu as TC
            import test_sim3_graph_gpu as TG
            name, N = "drift_loop", 7
        import pose_graph_ref as PR
        import test_pose_graph_cpu as PC
        fields = ("chi2_initial", "chi2_final", "iterations", "trials", "cg_iterations", "lam", "status")
        s = TC.scene(name)
        assert int(np.count_nonzero(s.fixed)) == 1
        if host:
            Pd, sd = TG.direct(name)

            def call(ctx):
                P, st = TG.run(s, ctx) if kind == "pg" else TG.run(s, ctx, iterations=TG.SOLVE_ITERATIONS[name])
                assert st["cg_iterations"] >= 2 * st["trials"] and st["status"] == 0
                return dict(states=np.asarray(P, np.float64), stats=np.array([st[k] for k in fields], np.float64))

            def check(o):
                P = o["states"].reshape(np.asarray(Pd).shape)
                got = {"chi2": abs(o["stats"][1] - sd["chi2_final"]) / sd["chi2_final"]}
                if kind == "pg":
                    got["rotation"], dist = R.pose_gap(P, Pd)
                else:
                    got["rotation"], dist, got["log_scale"] = R.sim_gap(P, Pd)
                got["translation"] = dist / PR.extent(s.gt)
                assert o["stats"][1] < o["stats"][0] and abs(o["stats"][0] - sd["chi2_initial"]) <= 1e-12 * sd["chi2_initial"]
                for key, v in got.items():
                    assert v <= PC.SOLVE_MARGIN * TC.YARD_SOLVE[name][key], (key, v)
                assert np.array_equal(P[s.fixed != 0], np.asarray(s.init).reshape(P.shape)[s.fixed != 0])
        else:
            _, b, Hd, W = R.linearize(s.init, s.edges, s.meas, s.info)[:4]
            H = R.assemble(s.V, s.edges, Hd, W)
            f = R.free_index(s.fixed)
            lam, tol = 1e-3 * np.abs(Hd).max(), 1e-8

            def call(ctx):
                import slamhip
                pcg = slamhip.pose_graph_pcg if kind == "pg" else slamhip.sim3_graph_pcg
                x, st = pcg(s.edges, s.fixed, Hd, W, b, lam, tol, 5000, ctx=ctx)
                assert st["converged"] and st["status"] == 0 and st["iterations"] >= 2
                return dict(x=np.asarray(x, np.float64), stats=np.array([st["iterations"], st["relres"], st["status"]], np.float64))

            def check(o):
                x = o["x"].reshape(s.V, N)
                bf = b.ravel()[f]
                res = float(np.linalg.norm(R.hmul(H, s.fixed, lam, x).ravel()[f] + bf) / np.linalg.norm(bf))
                assert res <= tol * PC.YARD_PCG_RECOMPUTE, res
                assert not x[s.fixed != 0].any()
        return call, check
    return build


def _larger_graph(kind):
    """The family's `hub` scene (1001 vertices): a larger graph whose layout puts every region of the workspace elsewhere."""
    def run(ctx):
        if kind == "pg":
            import test_pose_graph_cpu as TC
            import test_pose_graph_gpu as TG
            TG.run(TC.scene("hub"), ctx)
        else:
            import test_sim3_graph_cpu as TC
            import test_sim3_graph_gpu as TG
            TG.run(TC.scene("hub"), ctx, iterations=TG.SOLVE_ITERATIONS["hub"])
    return run


# =============================================================== ORB, the host calls, the normal equations ===================
def _orb_host():
    """slam_orb_extract_u8_host on one 120 x 160 image: the io arena and the workspace of the context path."""
    import orb_cases as C
    from slamhip import orb
    rng = np.random.default_rng(9701)
    img = (rng.integers(0, 256, (30, 40)).astype(np.uint8).repeat(4, 0).repeat(4, 1) // 2 + rng.integers(0, 128, (120, 160))).astype(np.uint8)
    P = orb.OrbParams(120, 160, n_features=100, n_levels=2)
    want = C.reference(img, P)
    assert 10 < len(want["x"]) <= P.n_max

    def call(ctx):
        from test_orb_edges_gpu import host_entry
        res = host_entry(ctx, P, img[None])                      # (asserts that the unused slots are zero)
        return dict(count=np.asarray(res.counts, np.int32), xy_level=res.xy_level[0], level=res.level[0], bin=res.bin[0], response=res.response[0],
                    descriptors=res.descriptors[0])

    def check(o):
        assert int(o["count"][0]) == len(want["x"])
        assert np.array_equal(o["xy_level"][:, 0], want["x"]) and np.array_equal(o["xy_level"][:, 1], want["y"])
        for k in ("level", "bin", "response", "descriptors"):
            assert np.array_equal(o[k], want[k]), k
    return call, check


def _knn2_host():
    from oracle import oracle
    rng = np.random.default_rng(9702)
    q, t = _rows(rng, 300), _rows(rng, 210)
    q[5] = t[17]
    want = oracle.bf_knn_c(q, t, 2)

    def call(ctx):
        import slamhip
        idx, dist = slamhip.knn_match_arrays(q, t, 2, ctx=ctx)
        return dict(idx=idx, dist=dist)

    def check(o):
        assert np.array_equal(o["idx"], want[0]) and np.array_equal(o["dist"], want[1])
    return call, check


def _match_host():
    """slam_bf_match_host: the drop-in match with the min-distance filter (its own kernel and its keep flags in the arena)."""
    from oracle import oracle
    rng = np.random.default_rng(9703)
    src, qry = _rows(rng, 300), _rows(rng, 210)
    qry[5] = src[17]
    qry[6] = src[17] ^ np.uint8(1)
    want = oracle.bf_match_c(src, qry, 104.0)

    def call(ctx):
        import slamhip
        qi, ti, d = slamhip.match_arrays(src, qry, 104.0, ctx=ctx)
        return dict(query=np.asarray(qi), train=np.asarray(ti), distance=np.asarray(d))

    def check(o):
        assert o["query"].tolist() == want[0].tolist() and o["train"].tolist() == want[1].tolist() and o["distance"].tolist() == want[2].tolist()
        assert 2 < len(o["query"]) < len(qry)
    return call, check


def _pose_host():
    """slam_pose_optimize_host_f64 on 130 edges (the zero-copy form: the kernel writes its results into the pinned block)."""
    from oracle import oracle
    from test_ba_limits_gpu import FX, FY, CX, CY, _pose_frame
    T0, X, meas = _pose_frame(130, 9704)
    Tr, inl, chi2, acc = oracle.pose_lm_np(T0, X, meas, FX, FY, CX, CY)

    def call(ctx):
        from slamhip.pose_opt import optimize_pose_only_device
        got = optimize_pose_only_device(T0, X, meas, (FX, FY, CX, CY), ctx=ctx)
        return dict(pose=got.pose, inliers=got.inliers.astype(np.uint8), chi2=got.chi2, stats=np.array([got.n_inliers, got.iterations], np.int32))

    def check(o):
        assert np.allclose(o["pose"], Tr, rtol=0, atol=1e-8)
        assert np.array_equal(o["inliers"].astype(bool), inl) and o["stats"][0] == int(inl.sum())
        assert np.allclose(o["chi2"], chi2, rtol=1e-6, atol=1e-6) and abs(int(o["stats"][1]) - acc) <= 8
    return call, check


def _ba_host():
    """slam_ba_optimize_host_f64: the one-launch window adjustment, its workspace in the context's block."""
    import test_ba_limits_gpu as T
    w = T._uneven(np.random.default_rng(9705))
    ref = T._oracle(w, 6, 1.0)

    def call(ctx):
        got = T._one_launch(ctx, w, 6, 1.0)
        return dict(poses=got.poses, points=got.points, stats=np.array([got.chi2_initial, got.chi2_final, got.iterations], np.float64))

    def check(o):
        from slamhip.ba import BAResult
        T._holds(BAResult(poses=o["poses"], points=o["points"], chi2_initial=o["stats"][0], chi2_final=o["stats"][1], iterations=int(o["stats"][2])),
                 ref, w)
    return call, check


def _normal_eq():
    """slam_pose_normal_eq_f64 over 5000 edges, the suite's own case (20 blocks of partial sums in the workspace)."""
    from oracle import oracle
    from test_reproj_gpu import CX, CY, FX, FY, _problem
    O = 5000
    rng = np.random.default_rng(O)
    poses, pts, _, _, _ = _problem(rng, 1, O, 1)
    e0 = oracle.reproj_rj_c(poses, pts, np.zeros(O, np.int32), np.arange(O, dtype=np.int32), np.zeros((O, 2)), FX, FY, CX, CY)[0]
    meas = -e0 + rng.normal(0, 2.0, (O, 2))
    act = (rng.uniform(size=O) > 0.1).astype(np.uint8)
    rH, rb, rchi2 = oracle.pose_normal_eq_c(poses[0], pts, meas, act, FX, FY, CX, CY, 1.0)

    def call(ctx):
        import slamhip
        prob = slamhip.PoseOnlyProblem(ctx, pts, meas, (FX, FY, CX, CY))
        try:
            prob.set_active(act)
            H, b, chi2 = prob.normal_equations(poses[0], 1.0)
        finally:
            prob.free()
        return dict(H=np.asarray(H), b=np.asarray(b), chi2=np.asarray(chi2))

    def check(o):
        H, bb, chi2 = o["H"].reshape(6, 6), o["b"].reshape(6), o["chi2"].reshape(np.shape(rchi2))
        assert np.allclose(H, rH, rtol=1e-10, atol=1e-10 * np.abs(rH).max()), np.abs(H - rH).max()
        assert np.allclose(bb, rb, rtol=1e-10, atol=1e-10 * np.abs(rb).max()), np.abs(bb - rb).max()
        assert np.allclose(chi2, rchi2, rtol=1e-12, atol=1e-12), np.abs(chi2 - rchi2).max()
        assert np.array_equal(H, H.T)
    return call, check


# =============================================================== caller-owned workspaces =====================================
def _sparse_ba():
    """bundle_adjust_sparse (slam_bas_workspace, and the covisibility workspaces behind it) on the `edges` window."""
    import test_ba_sparse_gpu as T
    from oracle import oracle
    w = T._case("edges")
    ref = oracle.ba_lm_c(T._rt(w["T0"]), w["X0"], w["op"], w["ol"], w["meas"], *T.R.INTR, 6, w["fixed"], 1.0)

    def call(ctx):
        got, st = T._sparse(ctx, w, 6, 1.0)
        assert st["unconverged"] == 0 and st["status"] == 0 and st["cg_iterations"] > 0
        return dict(poses=got.poses, points=got.points, stats=np.array([got.chi2_initial, got.chi2_final, got.iterations, st["trials"], st["edges"]],
                                                                       np.float64))

    def check(o):
        from slamhip.ba import BAResult
        T._holds(BAResult(poses=o["poses"], points=o["points"], chi2_initial=o["stats"][0], chi2_final=o["stats"][1], iterations=int(o["stats"][2])),
                 ref, w)
        assert o["stats"][3] == ref[5]
    return call, check


def _bow_vectors():
    """slam_bow_vectors (slam_bow_vectors_workspace) on the kept-lengths case: six images, up to 129 kept words each."""
    import bow_cases as C
    import bow_ref as R
    words, off, idf, n_words = C.vector_kept_case()
    want = R.vectors_of_words(words, off, idf, n_words)

    def call(ctx):
        from test_bow_edges_gpu import device_vectors
        o, w, v, q = device_vectors(ctx, words, off, idf, n_words)
        return dict(offsets=o, words=w, values=v, q=q)

    def check(o):
        from test_bow_edges_gpu import assert_vectors
        assert_vectors((o["offsets"], o["words"], o["values"], o["q"]), want)
    return call, check


def _bow_train():
    """train_vocabulary (slam_bow_train_seed_workspace and every scratch buffer of a round) on training case `b`."""
    import bow_cases as C
    import bow_ref as R
    d, off, k, depth = C.train_case("b")
    want = R.train(d, off, k, depth)
    names = ("node_desc", "child_begin", "child_count", "word_of_node", "idf")

    def call(ctx):
        from slamhip import bow
        v = bow.train_vocabulary(d, off, k, depth, ctx=ctx)
        try:
            return {n: np.asarray(getattr(v, n)).copy() for n in names}
        finally:
            v.free()

    def check(o):
        for n in names:
            assert o[n].shape == want[n].shape and np.array_equal(o[n], want[n]), n
    return call, check


def _covis():
    """covisibility_device (slam_covis_workspace: counts, pairs and edges) with one pair more than a scan tile."""
    import covis_cases as C
    from covis_ref import covisibility_ref, same_tables
    lim = C.limits()
    name = f"pairs-{max(lim['sort_tile'], lim['scan_tile']) + 1}"
    case = C.cases()[name]
    K, L, op, ol, fixed = case
    want = covisibility_ref(op, ol, K, fixed)
    keys = ("edges", "weights", "pair_ptr", "pair_a", "pair_b")

    def call(ctx):
        from test_covis_gpu import _device
        return dict(zip(keys, _device(ctx, case)))

    def check(o):
        assert same_tables(tuple(o[k] for k in keys), want) and len(o["pair_a"]) > lim["scan_tile"]
    return call, check


# =============================================================== the table ===================================================
CASES = [
    Case("top2-chunks-valu", "bf_hamming.hip", "slam_bf_knn2_u256", [], "oracle.oracle:bf_knn_c", _top2_chunks(1), bf=True),
    Case("top2-chunks-mx16", "bf_hamming.hip", "slam_bf_knn2_u256", [], "oracle.oracle:bf_knn_c", _top2_chunks(2), bf=True),
    Case("top2-chunks-mx32", "bf_hamming.hip", "slam_bf_knn2_u256", [], "oracle.oracle:bf_knn_c", _top2_chunks(3), bf=True),
    Case("top2-passes", "bf_hamming.hip", "slam_bf_knn2_u256", [("slam_workspace", "slam_bf_knn2_keep")], "oracle.oracle:bf_knn_c", _top2_passes,
         bf=True),
    Case("topk-partials", "bf_topk.hip", "slam_bf_knn_u256", [("slam_workspace", "topk_search")], "oracle.oracle:bf_knn_c", _topk(False), bf=True),
    Case("topk-host", "bf_topk.hip", "slam_bf_knn_u256_host", [("slam_io_arena", "slam_bf_knn_u256_host")], "oracle.oracle:bf_knn_c", _topk(True),
         bf=True),
    Case("window", "bf_window.hip", "slam_bf_window_knn_u256", [("slam_workspace", "window_search")], "hamming_families:ref_window", _window(False),
         bf=True),
    Case("window-host", "bf_window.hip", "slam_bf_window_knn_u256_host", [("slam_io_arena", "slam_bf_window_knn_u256_host")],
         "hamming_families:ref_window", _window(True), bf=True),
    Case("radius-short", "bf_radius.hip", "slam_bf_radius_u256", [("radius_tables", "radius_search")], "hamming_families:ref_radius",
         _radius("short"), bf=True),
    Case("radius-long-host", "bf_radius.hip", "slam_bf_radius_u256_host", [("slam_workspace", "radius_search"),
                                                                            ("slam_io_arena", "slam_bf_radius_u256_host")],
         "hamming_families:ref_radius", _radius("long"), bf=True),
    Case("radius-total-only", "bf_radius.hip", "slam_bf_radius_u256", [], "hamming_families:ref_radius", _radius("total"), bf=True),
    Case("two-view-ransac", "two_view.hip", "slam_tv_essential_ransac_f64", [("slam_workspace", "slam_tv_essential_ransac_f64")],
         "oracle.oracle:tv_twin_ransac", _ransac("two_view")),
    Case("homography-ransac", "homography.hip", "slam_hg_ransac_f64", [("slam_workspace", "slam_hg_ransac_f64")], "hg_twin:ransac",
         _ransac("homography")),
    Case("pnp-ransac", "pnp.hip", "slam_pnp_ransac_f64", [("slam_workspace", "slam_pnp_ransac_f64")], "pnp_twin:ransac", _ransac("pnp")),
    Case("sim3-ransac", "sim3.hip", "slam_sim3_ransac_f64", [("slam_workspace", "slam_sim3_ransac_f64")], "sim3_twin:ransac", _ransac("sim3")),
    Case("proj-search-tables", "proj_match.hip", "slam_proj_match_search", [("slam_workspace", "pm_run")], "proj_match_ref:search",
         _proj_search(True)),
    Case("proj-search-own-tables", "proj_match.hip", "slam_proj_match_search", [], "proj_match_ref:search", _proj_search(False)),
    Case("proj-project", "proj_match.hip", "slam_proj_match_project", [], "proj_match_ref:gates", _proj_project),
    Case("proj-grid", "proj_match.hip", "slam_proj_match_grid", [("slam_workspace", "slam_proj_match_grid")], "proj_match_ref:gates", _proj_grid),
    Case("bow-group", "bow_match.hip", "slam_bow_match_group", [("slam_workspace", "slam_bow_match_group")], "bow_match_ref:search", _bow_group),
    Case("bow-search-tables", "bow_match.hip", "slam_bow_match_search", [("slam_workspace", "bm_run")], "bow_match_ref:search", _bow_search(True)),
    Case("bow-search-own-tables", "bow_match.hip", "slam_bow_match_search", [], "bow_match_ref:search", _bow_search(False)),
    Case("tri-search-tables", "tri_match.hip", "slam_tri_match_search", [("slam_workspace", "slam_tri_match_search")], "tri_match_ref:search",
         _tri_search(True)),
    Case("tri-search-own-tables", "tri_match.hip", "slam_tri_match_search", [], "tri_match_ref:search", _tri_search(False)),
    Case("tri-triangulate", "tri_match.hip", "slam_tri_match_triangulate", [("slam_workspace", "slam_tri_match_triangulate")],
         "tri_match_twin:triangulate_centres", _tri_triangulate),
    Case("fuse-search-tables", "fuse.hip", "slam_fuse_search", [("slam_workspace", "slam_fuse_search")], "fuse_ref:search", _fuse_search(True)),
    Case("fuse-search-no-tables", "fuse.hip", "slam_fuse_search", [], "fuse_ref:search", _fuse_search(False)),
    Case("fuse-refresh", "fuse.hip", "slam_fuse_refresh", [("slam_workspace", "slam_fuse_refresh")], "fuse_ref:refresh", _fuse_refresh),
    Case("pose-graph-pcg", "graph_lm.h", "slam_pg_pcg_f64", [("slam_io_arena", "glm_blocks")], "pose_graph_ref:hmul", _graph("pg", False),
         before=_larger_graph("pg")),
    Case("pose-graph-optimize-host", "graph_lm.h", "slam_pg_optimize_host_f64", [("slam_io_arena", "glm_optimize_host_call")],
         "pose_graph_ref:optimize", _graph("pg", True), before=_larger_graph("pg")),
    Case("sim3-graph-pcg", "graph_lm.h", "slam_s3g_pcg_f64", [("slam_workspace", "glm_blocks")], "sim3_graph_ref:hmul", _graph("s3g", False),
         before=_larger_graph("s3g")),
    Case("sim3-graph-optimize-host", "graph_lm.h", "slam_s3g_optimize_host_f64", [("slam_workspace", "glm_optimize_host_call")],
         "sim3_graph_ref:optimize", _graph("s3g", True), before=_larger_graph("s3g")),
    Case("orb-host", "orb.hip", "slam_orb_extract_u8_host", [("slam_io_arena", "slam_orb_extract_u8_host"),
                                                             ("slam_workspace", "slam_orb_extract_u8_host")], "orb_cases:reference", _orb_host),
    Case("knn2-host", "host_calls.hip", "slam_bf_knn2_u256_host", [("slam_io_arena", "slam_bf_knn2_u256_host")], "oracle.oracle:bf_knn_c", _knn2_host,
         bf=True),
    Case("match-host", "host_calls.hip", "slam_bf_match_host", [("slam_io_arena", "slam_bf_match_host")], "oracle.oracle:bf_match_c", _match_host,
         bf=True),
    Case("pose-optimize-host", "host_calls.hip", "slam_pose_optimize_host_f64", [("slam_io_arena", "slam_pose_optimize_host_f64")],
         "oracle.oracle:pose_lm_np", _pose_host),
    Case("ba-one-launch-host", "host_calls.hip", "slam_ba_optimize_host_f64", [("slam_io_arena", "slam_ba_optimize_host_f64"),
                                                                               ("slam_workspace", "slam_ba_optimize_host_f64")],
         "oracle.oracle:ba_lm_c", _ba_host),
    Case("pose-normal-equations", "reproj.hip", "slam_pose_normal_eq_f64", [("slam_workspace", "slam_pose_normal_eq_f64")],
         "oracle.oracle:pose_normal_eq_c", _normal_eq),
    Case("sparse-ba", "ba_sparse.hip", "slam_bas_workspace", [], "oracle.oracle:ba_lm_c", _sparse_ba),
    Case("bow-vectors", "bow.hip", "slam_bow_vectors_workspace", [], "bow_ref:vectors_of_words", _bow_vectors),
    Case("bow-train", "bow.hip", "slam_bow_train_seed_workspace", [], "bow_ref:train", _bow_train),
    Case("covis-tables", "covis.hip", "slam_covis_workspace", [], "covis_ref:covisibility_ref", _covis),
]

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
