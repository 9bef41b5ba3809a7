"""Stereo matching on the device: the C entry on blocks the test builds itself (its own keypoint tables, pyramid planes with a
pitch above the width, poisoned outputs with pad rows behind them) against the numpy statement bit for bit; the hand cases of
tests/stereo_cases.py; the chain extractor -> stereo_match on resident buffers against the statement and against the true
disparity; repeatability; the Python layer."""
import ctypes

import numpy as np
import pytest

import stereo_cases as C
import stereo_ref as ref

pytestmark = pytest.mark.gpu
POISON = 0xA5
PAD = 3                                         # rows behind every output that must keep the poison
TYPES = (("right", np.int32), ("u_right", np.float64), ("depth", np.float64), ("orb_dist", np.int32), ("sad", np.int32), ("status", np.uint8))
SMALL = ((48, 40), (40, 33), (33, 28))


class DeviceBlock:
    """A block as the extractor leaves it, built by hand: count, kp, desc and a "workspace" whose image blocks start at `base`,
    lie `stride` apart and hold level l at off[l] with rows pitch[l] > w[l] apart; everything between the planes is poison."""

    def __init__(self, ctx, blk, base=256, extra_pitch=7):
        planes = blk["planes"]
        B = len(planes)
        shapes = [p.shape for p in planes[0]] if B else []
        self.pitch = np.asarray([(w + extra_pitch + 3) // 4 * 4 for _, w in shapes], np.int32)
        self.off, at = np.zeros(len(shapes), np.uint64), 0
        for l, (h, _) in enumerate(shapes):
            self.off[l] = at
            at += (int(self.pitch[l]) * h + 63) // 64 * 64
        self.base, self.stride = base, at + 128
        self.w, self.h = np.asarray([s[1] for s in shapes], np.int32), np.asarray([s[0] for s in shapes], np.int32)
        img = np.full(base + max(B, 1) * self.stride, POISON, np.uint8)
        for b in range(B):
            for l, pl in enumerate(planes[b]):
                h, w = pl.shape
                o = base + b * self.stride + int(self.off[l])
                img[o:o + h * self.pitch[l]].reshape(h, self.pitch[l])[:, :w] = pl
        self.B, self.n_max = B, blk["kp"].shape[1]
        self.bufs = dict(count=ctx.upload(np.ascontiguousarray(np.concatenate([blk["count"], np.zeros(4, np.int32)]))),
                         kp=ctx.upload(np.concatenate([blk["kp"].reshape(-1, 4), np.zeros((4, 4), np.int32)])),
                         desc=ctx.upload(np.concatenate([blk["desc"].reshape(-1, 32), np.zeros((4, 32), np.uint8)])), ws=ctx.upload(img))

    def args(self):
        b = self.bufs
        return (self.B, b["count"].ptr, b["kp"].ptr, b["desc"].ptr, b["ws"].ptr)

    def free(self):
        for v in self.bufs.values():
            v.free()


def run_c(ctx, pairs, L, R, scale, prm):
    """slam_stereo_match on two DeviceBlocks of one layout: the outputs [P, n_max] and counts [P, 2]; asserts that the pad rows
    behind every output kept their poison."""
    pairs = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
    P, n_max = len(pairs), L.n_max
    slots = P * n_max
    need = ctypes.c_uint64(0)
    assert ctx.lib.slam_stereo_workspace(P, n_max, ctypes.byref(need)) == 0
    ws = ctx.malloc(need.value)
    host = {k: np.frombuffer(bytes([POISON]) * (np.dtype(t).itemsize * (slots + PAD)), t).copy() for k, t in TYPES}
    host["counts"] = np.frombuffer(bytes([POISON]) * (4 * (2 * P + PAD)), np.int32).copy()
    dev = {k: ctx.upload(v) for k, v in host.items()}
    sc = np.ascontiguousarray(scale, np.float32)
    try:
        rc = ctx.lib.slam_stereo_match(ctx.handle, P, pairs.ctypes.data if P else None, *L.args(), *R.args(), n_max, len(sc), L.base, L.stride,
                                       L.off.ctypes.data, L.pitch.ctypes.data, L.w.ctypes.data, L.h.ctypes.data, sc.ctypes.data, float(prm["bf"]),
                                       float(prm.get("min_d", 0.0)), float(prm["max_d"]), int(prm.get("th_orb", 75)), int(prm.get("w", 5)),
                                       int(prm.get("Ls", 5)), int(bool(prm.get("reject", True))), ws.ptr, need.value,
                                       *[dev[k].ptr for k, _ in TYPES], dev["counts"].ptr)
        assert rc == 0, ctx.lib.slam_last_error()
        ctx.sync()
        out = {}
        for k, t in TYPES:
            a = dev[k].download(t, (slots + PAD,))
            assert a[slots:].tobytes() == bytes([POISON]) * (PAD * np.dtype(t).itemsize), f"{k}: the rows behind the output were written"
            out[k] = a[:slots].reshape(P, n_max)
        c = dev["counts"].download(np.int32, (2 * P + PAD,))
        assert c[2 * P:].tobytes() == bytes([POISON]) * (4 * PAD), "counts: the rows behind the output were written"
        out["counts"] = c[:2 * P].reshape(P, 2)
        return out
    finally:
        ws.free()
        for v in dev.values():
            v.free()


def same(got, want, what):
    for k, _ in TYPES:
        assert got[k].tobytes() == np.ascontiguousarray(want[k]).tobytes(), (what, k, np.flatnonzero((got[k] != want[k]).ravel())[:8].tolist())
    assert np.array_equal(got["counts"], want["counts"]), (what, got["counts"].tolist(), want["counts"].tolist())


COUNTS_L, COUNTS_R = [0, 1, 63, 64, 65, 257], [257, 64, 0, 65, 1, 63]
CROSS = [(b, b) for b in range(6)] + [(a, 0) for a in range(6)] + [(a, 2) for a in range(6)]
ALL65 = [(a, b) for a in range(6) for b in range(6)] + [(5, 0)] * 2 + [(a, 3) for a in range(6)] * 4 + [(2, 1), (4, 5), (3, 3)]


@pytest.fixture(scope="module")
def blocks():
    return C.random_blocks(11, COUNTS_L, COUNTS_R, 260)


@pytest.fixture(scope="module")
def blocks_dev(gpu_ctx, blocks):
    L, R = DeviceBlock(gpu_ctx, blocks[0]), DeviceBlock(gpu_ctx, blocks[1])
    yield L, R
    L.free()
    R.free()


# ---- the C entry against the statement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pairs", [[(5, 0)], [(5, 5), (3, 3), (1, 0)], CROSS, ALL65], ids=["P1", "P3", "P18", "P65"])
def test_c_entry_equals_the_statement(gpu_ctx, blocks, blocks_dev, pairs):
    assert len(ALL65) == 65
    want = ref.match(pairs, blocks[0], blocks[1], C.SCALE3, **C.PARAMS3)
    same(run_c(gpu_ctx, pairs, *blocks_dev, C.SCALE3, C.PARAMS3), want, len(pairs))


def test_every_status_occurs_and_other_parameters(gpu_ctx):
    left, right = C.random_blocks(1, [257, 65, 64], [257, 63, 1], 260)
    pairs = [(0, 0), (1, 1), (2, 2)]
    L, R = DeviceBlock(gpu_ctx, left), DeviceBlock(gpu_ctx, right)
    try:
        want = ref.match(pairs, left, right, C.SCALE3, **C.PARAMS3)
        assert (np.bincount(want["status"].ravel(), minlength=7) > 0).all(), "the case does not reach every status"
        same(run_c(gpu_ctx, pairs, L, R, C.SCALE3, C.PARAMS3), want, "defaults")
        for prm in (dict(C.PARAMS3, reject=False), dict(C.PARAMS3, w=3, Ls=7, min_d=1.5, th_orb=60), dict(C.PARAMS3, w=15, Ls=15, max_d=9.0),
                    dict(C.PARAMS3, w=1, Ls=1, th_orb=256)):
            same(run_c(gpu_ctx, pairs, L, R, C.SCALE3, prm), ref.match(pairs, left, right, C.SCALE3, **prm), prm)
    finally:
        L.free()
        R.free()


def test_small_planes(gpu_ctx):
    left, right = C.random_blocks(4, [65, 33], [70, 12], 72, sizes=SMALL, shifts=(4, 3, 3))
    L, R = DeviceBlock(gpu_ctx, left), DeviceBlock(gpu_ctx, right)
    try:
        prm = dict(C.PARAMS3, max_d=6.0)
        want = ref.match([(0, 0), (1, 1), (0, 1)], left, right, C.SCALE3, **prm)
        assert (want["status"] == ref.MATCHED).any() and (want["status"] == ref.WINDOW).any()
        same(run_c(gpu_ctx, [(0, 0), (1, 1), (0, 1)], L, R, C.SCALE3, prm), want, "48 x 40")
    finally:
        L.free()
        R.free()


def test_the_same_block_as_left_and_right(gpu_ctx, blocks):
    both = C.joined(*blocks)
    pairs = [(b, 6 + b) for b in range(6)] + [(11, 5), (5, 5)]
    D = DeviceBlock(gpu_ctx, both)
    try:
        same(run_c(gpu_ctx, pairs, D, D, C.SCALE3, C.PARAMS3), ref.match(pairs, both, both, C.SCALE3, **C.PARAMS3), "one block")
    finally:
        D.free()


def test_hand_cases_through_the_device(gpu_ctx):
    for name, scene, prm, expect in C.hand_cases():
        kL, dL, pL, kR, dR, pR, scale = scene
        n_max = max(len(kL), len(kR)) + 2
        left, right = C.block_of(kL, dL, pL, n_max), C.block_of(kR, dR, pR, n_max)
        L, R = DeviceBlock(gpu_ctx, left), DeviceBlock(gpu_ctx, right)
        try:
            out = run_c(gpu_ctx, [(0, 0)], L, R, scale, prm)
            C.check_expect({k: out[k][0] for k in out}, expect, name)
            same(out, ref.match([(0, 0)], left, right, scale, **prm), name)
        finally:
            L.free()
            R.free()


# ---- repeatability and the empty calls ----------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bytes_and_empty_calls_do_nothing(gpu_ctx, blocks, blocks_dev):
    a, b = (run_c(gpu_ctx, ALL65, *blocks_dev, C.SCALE3, C.PARAMS3) for _ in range(2))
    same(a, b, "second run")
    none = run_c(gpu_ctx, np.zeros((0, 2), np.int32), *blocks_dev, C.SCALE3, C.PARAMS3)      # P = 0: run_c checks that nothing was written
    assert none["status"].shape == (0, 260)
    out = run_c(gpu_ctx, [(0, 0), (0, 3), (0, 5)], *blocks_dev, C.SCALE3, C.PARAMS3)            # every left count is 0
    assert (out["status"] == ref.NO_CANDIDATE).all() and (out["right"] == -1).all() and (out["orb_dist"] == ref.NO_DIST).all()
    assert (out["sad"] == -1).all() and np.isnan(out["u_right"]).all() and np.isnan(out["depth"]).all() and not out["counts"].any()


# ---- the extractor chain ------------------------------------------------------------------------------------------------------------
def _chain(gpu_ctx, d, n_levels):
    import slamhip
    from slamhip.orb import OrbExtractor, OrbParams

    P = OrbParams(C.CHAIN_H, C.CHAIN_W, C.CHAIN_FEATURES, n_levels, 1.2, 20)
    ex = OrbExtractor(gpu_ctx, 2, P)
    ex.upload(np.stack(C.chain_images(d)))
    ex.run()
    count, kp, _, desc = ex.download()
    blk = dict(count=count, kp=kp, desc=desc, planes=[[ex.stage(b, l)[0] for l in range(n_levels)] for b in range(2)])
    return slamhip, ex, blk, ref.scale_table(1.2, n_levels)


@pytest.mark.parametrize("n_levels", [1, 3])
@pytest.mark.parametrize("d", [3, 17])
def test_extractor_chain(gpu_ctx, d, n_levels):
    slamhip, ex, blk, sc = _chain(gpu_ctx, d, n_levels)
    try:
        n = int(blk["count"][0])
        assert n > 100
        for reject in (True, False):
            res = slamhip.stereo_match(ex, pairs=[(0, 1)], bf=C.CHAIN_BF, max_d=C.CHAIN_MAX_D, reject=reject)
            want = ref.match([(0, 1)], blk, blk, sc, bf=C.CHAIN_BF, max_d=C.CHAIN_MAX_D, reject=reject)
            for k, _ in TYPES:
                assert getattr(res, k)[0].tobytes() == np.ascontiguousarray(want[k][0, :n]).tobytes(), (k, reject)
            assert np.array_equal(res.counts, want["counts"])
            assert np.array_equal(res.xy[0][:, 0].astype(np.float64), ref.level0(blk["kp"][0, :n, 0], sc[blk["kp"][0, :n, 2]]))
        if n_levels == 1:
            # truth (reject off: see stereo_cases.CHAIN_MEASURED): SAD 0 at the true inc and |delta| <= 1/2 bound the error by 0.5
            got = dict(status=[res.status[0]], sad=[res.sad[0]], u_right=[res.u_right[0]], uL=res.xy[0][:, 0].astype(np.float64))
            rows, err = C.chain_truth(got, d)
            print(f"d={d}: {rows} status-0 rows with SAD 0 (floor {C.CHAIN_FLOOR[d]}, CPU {C.CHAIN_MEASURED[d]}), largest |disp - d| = {err:.4f}")
            assert err <= 0.5
            assert rows >= C.CHAIN_FLOOR[d]
    finally:
        ex.free()


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------
def test_points_point_set_backend_and_arrays(gpu_ctx):
    from backend import Backend

    slamhip, ex, blk, sc = _chain(gpu_ctx, 17, 3)
    try:
        kw = dict(bf=C.CHAIN_BF, max_d=C.CHAIN_MAX_D)
        res = slamhip.stereo_match(ex, pairs=[(0, 1)], **kw)
        via = Backend().stereo_frame(ex, pairs=[(0, 1)], **kw)
        n = int(blk["count"][0])
        arrays = slamhip.stereo_match_arrays([blk["kp"][0, :n]], [blk["desc"][0, :n]], [blk["planes"][0]], [blk["kp"][1, :blk["count"][1]]],
                                             [blk["desc"][1, :blk["count"][1]]], [blk["planes"][1]], sc, ctx=gpu_ctx, **kw)
        for other in (via, arrays):
            for k, _ in TYPES:
                assert getattr(other, k)[0].tobytes() == getattr(res, k)[0].tobytes(), k
            assert np.array_equal(other.counts, res.counts)
        K = (458.654, 457.296, 80.0, 60.0)
        ok = res.status[0] == ref.MATCHED
        assert ok.sum() > 50
        X, close = res.points(0, K)
        z, uv = res.depth[0], res.xy[0].astype(np.float64)
        assert np.isnan(X[~ok]).all() and not close[~ok].any()
        assert np.array_equal(X[ok], np.stack([(uv[ok, 0] - K[2]) * z[ok] / K[0], (uv[ok, 1] - K[3]) * z[ok] / K[1], z[ok]], 1))
        assert np.array_equal(close[ok], z[ok] < 40.0 * C.CHAIN_BF / K[0]) and np.array_equal(res.points(0, K, th_depth=3.0)[1][ok], z[ok] < 3.0)
        c, s = np.cos(0.3), np.sin(0.3)
        T = np.asarray([[c, 0, s, 0.5], [0, 1, 0, -0.2], [-s, 0, c, 1.0]])
        Xw, _ = res.points(0, K, T)
        assert np.allclose(Xw[ok] @ T[:, :3].T + T[:, 3], X[ok], rtol=0, atol=1e-9)
        ps, rows = res.point_set(0, K, T, ctx=gpu_ctx)
        try:
            assert np.array_equal(rows, np.flatnonzero(ok)) and ps.n == ok.sum() and ps.has_range and ps.has_level
            dist = np.linalg.norm(Xw[ok] - (-T[:, :3].T @ T[:, 3]), axis=1)
            dmax = dist * sc.astype(np.float64)[res.level[0][ok]]
            rng = ps.device["range"].download(np.float64, (ps.n, 2))
            assert np.allclose(rng[:, 1], dmax ** 2, rtol=1e-12) and np.allclose(rng[:, 0], (dmax / float(sc[-1])) ** 2, rtol=1e-12)
            assert np.array_equal(ps.device["desc"].download(np.uint8, (ps.n, 32)), res.descriptors[0][ok])
            assert np.array_equal(ps.device["level"].download(np.int32, (ps.n,)), res.level[0][ok])
            assert np.allclose(ps.device["xyz"].download(np.float64, (ps.n, 3)), Xw[ok], rtol=0, atol=0)
        finally:
            ps.free()
    finally:
        ex.free()
