"""Lens distortion on the device (csrc/camera.hip) against the host twin of the same text (tests/camera_twin.py), BIT FOR BIT on
pixels, normalised coordinates, status and map entries for every model: csrc/cam_model.h uses + - * / and sqrt only (its atan and
tan are series of its own), compiled with contraction off on both sides.  The remap is integer arithmetic and is held to the
numpy statement of the header's formula (tests/camera_ref.py) applied to the map the device wrote.  What the twin itself is worth
is tests/test_camera_cpu.py's business."""
import ctypes
import os

import numpy as np
import pytest

import camera_cases as C
import camera_ref as ref
import camera_twin as tw

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
POISON = 0xA5
PAD = 96                                              # rows behind the last point that must keep their poison


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def mixed_points(case, n, seed):
    """n raw pixels of a case: mostly inside, with NaN / inf inputs and pixels beyond the fold (or beyond 1.5 rad) mixed in."""
    rng = np.random.default_rng(seed)
    W, H = case.size
    px = np.stack([rng.uniform(-40, W + 40, n), rng.uniform(-40, H + 40, n)], -1)
    if n >= 8:
        px[rng.integers(0, n, n // 8)] = [np.nan, 3.0]
        px[rng.integers(0, n, n // 16 + 1)] = [5.0, np.inf]
        far = rng.integers(0, n, n // 8)
        px[far] = np.asarray(case.K[2:]) + rng.uniform(2.0, 9.0, (len(far), 2)) * np.asarray(case.K[:2]) * rng.choice([-1, 1], (len(far), 2))
    return px


def device_points(ctx, op, px, cases, offsets=None, cam_index=None, iterations=10, with_norm=True):
    """The C entry on poisoned outputs: (out, norm, status), after checking that nothing behind row n was written."""
    px = np.ascontiguousarray(px, np.float64).reshape(-1, 2)
    n = len(px)
    off = np.asarray([0, n] if offsets is None else offsets, np.int64)
    rec = np.ascontiguousarray(np.stack([C.record(c) for c in cases]))
    idx = None if cam_index is None else np.ascontiguousarray(cam_index, np.int32)
    P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rows = n + PAD
    d_in = ctx.upload(px if n else np.zeros((1, 2)))
    bufs = [ctx.upload(np.full(16 * rows, POISON, np.uint8)), ctx.upload(np.full(16 * rows, POISON, np.uint8)), ctx.upload(np.full(rows, POISON, np.uint8))]
    try:
        args = (ctx.handle, len(off) - 1, P(off), len(rec), P(rec), P(idx))
        tail = (d_in.ptr, bufs[0].ptr, bufs[1].ptr if with_norm else None, bufs[2].ptr)
        rc = ctx.lib.slam_cam_undistort_f64(*args, int(iterations), *tail) if op == 0 else ctx.lib.slam_cam_distort_f64(*args, *tail)
        assert rc == 0, ctx.lib.slam_last_error()
        ctx.sync()
        raw = [b.download(np.uint8, (b.nbytes,)) for b in bufs]
    finally:
        for b in [d_in] + bufs:
            b.free()
    assert (raw[0][16 * n:] == POISON).all() and (raw[1][16 * n if with_norm else 0:] == POISON).all() and (raw[2][n:] == POISON).all()
    return raw[0][:16 * n].view(np.float64).reshape(n, 2), raw[1][:16 * n].view(np.float64).reshape(n, 2) if with_norm else None, raw[2][:n].copy()


# ---- points ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_points_equal_the_twin_bit_for_bit(gpu_ctx, case):
    worst = 0.0
    for n in (0, 1, 63, 64, 65, 257):
        px = mixed_points(case, n, 100 + n)
        for op, fn in ((0, tw.undistort), (1, tw.distort)):
            got = device_points(gpu_ctx, op, px, [case])
            want = fn(C.record(case), px)
            for g, w, name in zip(got, want, ("pixels", "normalised", "status")):
                assert same_bits(g, w), (case.name, n, op, name)
            if n == 257:
                assert op == 1 or {0, 3} <= set(got[2].tolist())
                if case is C.FOLD or case is C.TUMVI:
                    assert op == 1 or 2 in got[2]
                # the bound the equidistant model would need if it called the math library: |d(u - cx)| <= 8 * 2^-52 |u - cx|
                ok = got[2] == 0
                with np.errstate(invalid="ignore", divide="ignore"):
                    rel = np.abs(got[0][ok] - want[0][ok]) / np.abs(want[0][ok] - np.asarray(case.K[2:]))
                worst = max(worst, float(np.nanmax(rel, initial=0.0)) * 2.0 ** 52)
    print(f"{case.name}: max |d(u - cx)| / |u - cx| device against twin = {worst:.2f} ulp")
    assert worst <= 8.0


def test_points_without_normalised_output_and_with_other_iteration_counts(gpu_ctx):
    px = mixed_points(C.EUROC, 130, 7)
    for it in (0, 1, 4, 100):
        got = device_points(gpu_ctx, 0, px, [C.EUROC], iterations=it, with_norm=False)
        want = tw.undistort(C.record(C.EUROC), px, it)
        assert same_bits(got[0], want[0]) and same_bits(got[2], want[2]) and got[1] is None, it
    assert 1 in device_points(gpu_ctx, 0, px, [C.EUROC], iterations=1)[2]


def test_three_sets_with_the_middle_one_empty_and_two_cameras_of_different_models(gpu_ctx):
    a, b = mixed_points(C.EUROC, 300, 1), mixed_points(C.TUMVI, 70, 2)
    px, off = np.concatenate([a, b]), [0, 300, 300, 370]
    for idx, cams in (([0, 1, 1], (C.EUROC, C.TUMVI)), ([1, 0, 0], (C.TUMVI, C.EUROC)), ([0, 0, 1], (C.EUROC, C.TUMVI))):
        for op, fn in ((0, tw.undistort), (1, tw.distort)):
            got = device_points(gpu_ctx, op, px, cams, off, idx)
            for k in range(3):
                want = np.concatenate([fn(C.record(C.EUROC), a)[k], fn(C.record(C.TUMVI), b)[k]])
                assert same_bits(got[k], want), (idx, op, k)
    # no index array: every set uses camera 0; more sets than one launch holds (32), most of them empty or tiny
    many = np.unique(np.concatenate([[0, 370], np.random.default_rng(3).integers(0, 371, 120)]))
    many = np.sort(np.concatenate([many, many[5:9]]))                               # a few empty sets
    assert len(many) - 1 > 64
    got = device_points(gpu_ctx, 0, px, [C.FOLD, C.EUROC], many)
    want = tw.undistort(C.record(C.FOLD), px)
    assert all(same_bits(g, w) for g, w in zip(got, want))
    alt = (np.arange(len(many) - 1) % 2).astype(np.int32)
    got = device_points(gpu_ctx, 0, px, [C.FOLD, C.EUROC], many, alt)
    w0, w1 = tw.undistort(C.record(C.FOLD), px), tw.undistort(C.record(C.EUROC), px)
    pick = np.repeat(alt, np.diff(many)).astype(bool)
    assert all(same_bits(g, np.where(pick.reshape((-1,) + (1,) * (a0.ndim - 1)), a1, a0)) for g, a0, a1 in zip(got, w0, w1))


def test_python_layer_points_bounds_and_backend(gpu_ctx):
    import slamhip
    from backend import Backend

    euroc = slamhip.CameraModel(*C.EUROC.K, C.EUROC.model, C.EUROC.coeffs)
    tumvi = slamhip.CameraModel(*C.TUMVI.K, C.TUMVI.model, C.TUMVI.coeffs)
    a, b = mixed_points(C.EUROC, 100, 4), mixed_points(C.TUMVI, 50, 5)
    out, norm, st = slamhip.undistort_points(np.concatenate([a, b]), [euroc, tumvi], [0, 100, 150], [0, 1], ctx=gpu_ctx)
    wa, wb = tw.undistort(C.record(C.EUROC), a), tw.undistort(C.record(C.TUMVI), b)
    assert same_bits(out, np.concatenate([wa[0], wb[0]])) and same_bits(norm, np.concatenate([wa[1], wb[1]])) and same_bits(st, np.concatenate([wa[2], wb[2]]))
    raw, _, st2 = slamhip.distort_points(wa[0], euroc, ctx=gpu_ctx)
    ok = wa[2] == 0
    near = ok & (np.abs(a - np.asarray(C.EUROC.size) / 2) <= np.asarray(C.EUROC.size) / 2 + 40).all(1)      # the frame the 1e-9 px bound is derived for
    assert near.sum() > 50 and np.abs(raw[near] - a[near]).max() <= 1e-9 and np.array_equal(st2, np.where(ok, 0, 3))
    assert slamhip.image_bounds(euroc, C.EUROC.size, ctx=gpu_ctx) == tw.image_bounds(C.record(C.EUROC), C.EUROC.size)
    be = Backend()
    assert be.image_bounds(euroc, C.EUROC.size) == tw.image_bounds(C.record(C.EUROC), C.EUROC.size)
    o2, s2 = be.undistort_points(a, euroc)
    assert same_bits(o2, wa[0]) and same_bits(s2, wa[2])
    fold = slamhip.CameraModel(*C.FOLD.K, C.FOLD.model, C.FOLD.coeffs)
    with pytest.raises(ValueError, match="corners"):
        slamhip.image_bounds(fold, C.FOLD.size, ctx=gpu_ctx)                         # its corners lie beyond the fold


# ---- the map --------------------------------------------------------------------------------------------------------------
def device_map(ctx, case, size, new_K, R=None):
    import slamhip

    cam = slamhip.CameraModel(*case.K, case.model, case.coeffs)
    m = slamhip.RectifyMap(cam, size, new_K, R, ctx=ctx)
    try:
        return m.download()
    finally:
        m.free()


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_map_equals_the_twin_bit_for_bit(gpu_ctx, case):
    for size in ((1, 1), (70, 41), (64, 64)):
        for R in (None, C.rot_y(0.05)):
            got = device_map(gpu_ctx, case, size, case.K, R)
            want = tw.rectify_map(C.record(case), size, case.K, R)
            assert same_bits(got, want), (case.name, size, R is not None)
    # another K': the whole raw frame seen through a wider pinhole camera
    K2 = (0.6 * case.K[0], 0.6 * case.K[1], 35.0, 20.5)
    assert same_bits(device_map(gpu_ctx, case, (70, 41), K2), tw.rectify_map(C.record(case), (70, 41), K2))


def test_map_sentinels_where_the_ray_points_backwards(gpu_ctx):
    K2, R = (20.0, 20.0, 32.0, 32.0), C.rot_y(1.2)
    for case in (C.EUROC, C.TUMVI):
        got = device_map(gpu_ctx, case, (64, 64), K2, R)
        assert same_bits(got, tw.rectify_map(C.record(case), (64, 64), K2, R))
        s = (got == ref.SENTINEL).all(-1)
        assert 0 < s.sum() < s.size and np.array_equal(s, (got == ref.SENTINEL).any(-1))
    far = device_map(gpu_ctx, C.PINHOLE, (3, 1), (1e-9, 1e-9, 1.0, 0.0))
    assert (far[0, 0] == ref.SENTINEL).all() and (far[0, 2] == ref.SENTINEL).all() and far[0, 1].tolist() == [5136, 3816]


# ---- the remap ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def desk():
    return np.load(os.path.join(HERE, "golden", "orb_desk_320x240.npz"))["image"]


def device_remap(ctx, src, src_pitch, d_map, Wd, Hd, border, dst_pitch, with_mask=True, tail=333):
    """slam_cam_remap_u8 on padded, poisoned buffers: (dst [B,Hd,Wd], mask or None), after checking padding and tail."""
    B, Hs, Ws = src.shape
    padded = np.full((B, Hs, src_pitch), 0x3C, np.uint8)
    padded[:, :, :Ws] = src
    d_src = ctx.upload(padded)
    stride = Hd * dst_pitch + 24                                                        # a gap between the images, too
    outs = [ctx.upload(np.full(B * stride + tail, POISON, np.uint8)) for _ in range(2 if with_mask else 1)]
    try:
        rc = ctx.lib.slam_cam_remap_u8(ctx.handle, d_src.ptr, B, Hs, Ws, src_pitch, Hs * src_pitch, d_map.ptr, Hd, Wd, border, outs[0].ptr, dst_pitch,
                                       stride, outs[1].ptr if with_mask else None)
        assert rc == 0, ctx.lib.slam_last_error()
        ctx.sync()
        raw = [o.download(np.uint8, (o.nbytes,)) for o in outs]
    finally:
        for o in [d_src] + outs:
            o.free()
    res = []
    for r in raw:
        assert (r[B * stride:] == POISON).all()
        img = r[:B * stride].reshape(B, stride)
        assert (img[:, Hd * dst_pitch:] == POISON).all()
        rows = img[:, :Hd * dst_pitch].reshape(B, Hd, dst_pitch)
        assert (rows[:, :, Wd:] == POISON).all()
        res.append(rows[:, :, :Wd].copy())
    return res[0], (res[1] if with_mask else None)


def test_remap_equals_the_integer_formula_on_the_map_the_device_wrote(gpu_ctx, desk):
    import slamhip

    src = np.stack([desk[40:85, 100:167], desk[100:145, 30:97], desk[150:195, 200:267]])          # three 67 x 45 crops
    assert src.shape == (3, 45, 67)
    # a source camera of 67 x 45 seen through destinations that leave the source on all four sides
    cam = slamhip.CameraModel(60.0, 58.0, 33.2, 22.4, "radtan", (-0.25, 0.06, 0.001, -0.002, 0.0))
    maps = {"wide": slamhip.RectifyMap(cam, (70, 41), (40.0, 40.0, 34.5, 20.0), C.rot_y(0.05), ctx=gpu_ctx),
            "shifted": slamhip.RectifyMap(cam.pinhole(), (70, 41), (60.0, 58.0, 40.7, 12.3), ctx=gpu_ctx),
            "one": slamhip.RectifyMap(cam, (1, 1), (60.0, 58.0, 0.3, 0.4), ctx=gpu_ctx),
            "behind": slamhip.RectifyMap(cam, (70, 41), (30.0, 30.0, 35.0, 20.0), C.rot_y(1.0), ctx=gpu_ctx)}
    try:
        for name, m in maps.items():
            host = m.download()
            W, H = m.size
            if name == "wide":
                u, v = host[..., 0] >> 5, host[..., 1] >> 5
                assert (u < -1).any() and (u > 67).any() and (v < -1).any() and (v > 45).any() and ((u >= 0) & (u < 66) & (v >= 0) & (v < 44)).any()
            if name == "behind":
                assert (host == ref.SENTINEL).any() and (host != ref.SENTINEL).any()
            for B in (1, 3):
                for border in (0, 200):
                    for pitch, src_pitch in ((80, 67), (W, 72), (W + 3, 67)):
                        got, gmask = device_remap(gpu_ctx, src[:B], src_pitch, m.buf, W, H, border, pitch)
                        want, wmask = ref.remap(src[:B], host, border)
                        assert same_bits(got, want) and same_bits(gmask, wmask), (name, B, border, pitch)
            got, gmask = device_remap(gpu_ctx, src, 67, m.buf, W, H, 9, W + 2, with_mask=False)
            assert gmask is None and same_bits(got, ref.remap(src, host, 9)[0])
            hi, hm = slamhip.remap_images(src, m, border=200)
            assert same_bits(hi, ref.remap(src, host, 200)[0]) and same_bits(hm, ref.remap(src, host, 200)[1])
            one, none = slamhip.remap_images(src[0], m, with_mask=False)
            assert none is None and same_bits(one, ref.remap(src[:1], host, 0)[0])
    finally:
        for m in maps.values():
            m.free()


def test_remap_by_hand_maps_on_the_device(gpu_ctx, desk):
    """The hand-stated maps of the CPU suite through the kernel: identity, and the last column with a = 0."""
    src = np.ascontiguousarray(desk[10:19, 20:33])[None]
    j, i = np.meshgrid(np.arange(13), np.arange(9))
    for m, border in ((np.stack([32 * j, 32 * i], -1), 77), (np.stack([32 * (j + 3) + 5, 32 * (i - 2) + 31], -1), 200),
                      (np.stack([32 * j + 16, 32 * i + 16], -1), 0), (np.stack([32 * j - 1, 32 * i + 1], -1), 3)):
        m = np.ascontiguousarray(m, np.int32)
        d_map = gpu_ctx.upload(m)
        try:
            got, gmask = device_remap(gpu_ctx, src, 13, d_map, 13, 9, border, 16)
        finally:
            d_map.free()
        want, wmask = ref.remap(src, m, border)
        assert same_bits(got, want) and same_bits(gmask, wmask)
    assert same_bits(ref.remap(src, np.ascontiguousarray(np.stack([32 * j, 32 * i], -1), np.int32), 77)[0], src)


# ---- the hooks --------------------------------------------------------------------------------------------------------------
def test_upload_raw_equals_extraction_of_the_host_remap(gpu_ctx, desk):
    import slamhip
    from slamhip.orb import OrbExtractor, OrbParams, OrbResult, orb_extract_arrays

    frames = np.stack([desk, np.ascontiguousarray(desk[::-1, ::-1])])
    cam = slamhip.CameraModel(230.0, 229.0, 161.3, 118.6, "radtan", (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05))
    m = slamhip.RectifyMap(cam, (320, 240), (150.0, 150.0, 160.0, 120.0), ctx=gpu_ctx)      # a wider pinhole camera: its corners see nothing
    P = OrbParams(240, 320, 100, 2)
    ex = OrbExtractor(gpu_ctx, 2, P)
    try:
        host_img, host_mask = ref.remap(frames, m.download(), 0)
        assert 0 < (host_mask == 0).mean() < 0.5
        ex.upload_raw(frames, m)
        ex.run()
        got = OrbResult(P, *ex.download())
        want = orb_extract_arrays(host_img, mask=host_mask, n_features=100, n_levels=2, ctx=gpu_ctx)
        caller = np.zeros((240, 320), np.uint8)
        caller[:, :200] = 1
        ex.upload_raw(frames, m, border=0, mask=caller)
        ex.run()
        got2 = OrbResult(P, *ex.download())
        want2 = orb_extract_arrays(host_img, mask=np.where(caller[None] != 0, host_mask, 0).astype(np.uint8), n_features=100, n_levels=2, ctx=gpu_ctx)
        for g, w in ((got, want), (got2, want2)):
            assert g.counts.tolist() == w.counts.tolist() and g.counts.min() > 20
            for b in range(2):
                assert same_bits(g.xy_level[b], w.xy_level[b]) and same_bits(g.level[b], w.level[b]) and same_bits(g.bin[b], w.bin[b])
                assert same_bits(g.response[b], w.response[b]) and same_bits(g.descriptors[b], w.descriptors[b])
        with pytest.raises(ValueError):
            ex.upload_raw(frames[:1], m)
        with pytest.raises(ValueError):
            ex.upload_raw(frames, m, border=300)
    finally:
        ex.free()
        m.free()


def test_projection_search_on_undistorted_keypoints_equals_the_numpy_statement(gpu_ctx, desk):
    import proj_match_ref as R
    import slamhip
    from slamhip import proj_match as pm
    from slamhip.orb import orb_extract_arrays

    cam = slamhip.CameraModel(180.0, 179.0, 161.3, 118.6, "radtan", (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05))
    res = orb_extract_arrays(desk, n_features=300, ctx=gpu_ctx)
    xy_un, st = res.undistorted(cam, ctx=gpu_ctx)
    assert not st[0].any() and same_bits(xy_un[0], tw.undistort(cam.record, res.xy[0].astype(np.float64))[0])
    xy32 = xy_un[0].astype(np.float32)                                            # mvKeysUn is float
    bounds = slamhip.image_bounds(cam, (320, 240), ctx=gpu_ctx)
    assert bounds[0] < -20 and bounds[1] > 340 and bounds[2] < -20 and bounds[3] > 260
    # map points: the undistorted keypoints lifted to depths of 2..6 m, seen from a slightly moved camera
    rng = np.random.default_rng(31)
    n = len(xy32)
    z = rng.uniform(2.0, 6.0, n)
    xyz = np.stack([(xy_un[0][:, 0] - cam.cx) / cam.fx * z, (xy_un[0][:, 1] - cam.cy) / cam.fy * z, z], -1)
    A = np.eye(4)[:3].copy()
    A[:, 3] = [0.01, -0.005, 0.02]
    Ow = -A[:, 3]
    scale = R.scale_tables(8, 1.2)
    pts = dict(xyz=xyz, desc=res.descriptors[0], level=res.level[0].astype(np.int64), bins=res.bin[0].astype(np.int64))
    frame = dict(desc=res.descriptors[0], xy=xy32, level=res.level[0].astype(np.int64), bins=res.bin[0].astype(np.int64))
    ps = pm.PointSets(xyz, res.descriptors[0], level=pts["level"], bins=pts["bins"], ctx=gpu_ctx)
    fg = pm.FrameGrids.from_orb(res, xy=xy32, ctx=gpu_ctx)
    try:
        got = pm.search_by_projection(ps, fg, [(0, 0)], [A], [Ow], cam.K, bounds, scale, 7.0, return_tables=True, ctx=gpu_ctx)
    finally:
        ps.free()
        fg.free()
    want = R.search(pts, frame, A, Ow, 7.0, cam.K, bounds, *scale)
    assert np.array_equal(got[0][0], want[0]) and int(got[1][0]) == want[1] and want[1] > 50
    for k in ("status", "u", "v", "lp", "idx", "dist"):
        assert same_bits(got[2][0][k], want[2][k]), k
    # with the raw image as bounds, points whose undistorted pixel lies outside the raw frame are lost: the reason for image_bounds
    lost = R.search(pts, frame, A, Ow, 7.0, cam.K, (0.0, 320.0, 0.0, 240.0), *scale)
    print(f"matches with image_bounds: {want[1]}, with the raw frame as bounds: {lost[1]}")
    assert lost[1] <= want[1]
    # a keypoint without an undistorted image is taken out of every search
    bad = xy32.copy()
    bad[:5] = np.nan
    fg = pm.FrameGrids.from_orb(res, xy=[bad], ctx=gpu_ctx)
    ps = pm.PointSets(xyz, res.descriptors[0], level=pts["level"], bins=pts["bins"], ctx=gpu_ctx)
    try:
        m2 = pm.search_by_projection(ps, fg, [(0, 0)], [A], [Ow], cam.K, bounds, scale, 7.0, ctx=gpu_ctx)[0][0]
    finally:
        ps.free()
        fg.free()
    assert not np.isin(m2, np.arange(5)).any()
