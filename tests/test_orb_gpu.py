"""GPU: slam_orb_* against the numpy restatement of DESIGN.md 4d (tests/orb_ref.py), bit for bit: counts, level coordinates,
bins, R, descriptors, and the stage buffers read back through the layout query.  Shapes are chosen for where the kernels can
break (W not a multiple of 4, partial tiles, levels below 2 BORDER + 1, a constant image, a dense candidate list with ties)."""
import ctypes
import os

import numpy as np
import pytest

import orb_ref as ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def reference(img, P, mask=None):
    return ref.extract(img, P.lh, P.lw, P.quota, P.t, P.table, mask0=mask)


def assert_same(res, b, want, P):
    n = len(want["x"])
    assert int(res.counts[b]) == n
    assert np.array_equal(res.xy_level[b][:, 0], want["x"]) and np.array_equal(res.xy_level[b][:, 1], want["y"])
    assert np.array_equal(res.level[b], want["level"]) and np.array_equal(res.bin[b], want["bin"])
    assert np.array_equal(res.response[b], want["response"])
    assert np.array_equal(res.descriptors[b], want["descriptors"])
    s = np.float32(P.scale) ** np.arange(P.L, dtype=np.float32)
    assert np.array_equal(res.xy[b], np.stack([want["x"], want["y"]], 1).astype(np.float32) * s[want["level"]][:, None])
    assert np.array_equal(res.size[b], np.float32(31) * s[want["level"]])
    assert np.array_equal(res.angle[b], want["bin"].astype(np.float32) * np.float32(11.25))


@pytest.mark.parametrize("h,w,seed", [(83, 97, 11), (70, 131, 12)])
def test_odd_sizes_end_to_end(gpu_ctx, h, w, seed):
    from slamhip import orb

    img = ref.scene(h, w, seed, shapes=80)
    P = orb.OrbParams(h, w, n_features=120)
    assert (P.lw % 4 != 0).any() and (np.minimum(P.lw, P.lh) < 33).any() and (np.minimum(P.lw, P.lh) >= 33).any()
    want = reference(img, P)
    assert len(want["x"]) > 10
    res = orb.orb_extract_arrays(img, n_features=120, ctx=gpu_ctx)
    assert_same(res, 0, want, P)
    raw = orb.orb_extract_arrays(img[None], n_features=120, ctx=gpu_ctx, keep_on_device=True)      # the device entry
    assert_same(raw, 0, want, P)
    raw.free()


def test_stage_buffers_97x83(gpu_ctx):
    from slamhip import orb

    img = ref.scene(83, 97, 11, shapes=80)
    m = np.zeros((83, 97), np.uint8)
    m[:, 20:] = 1
    P = orb.OrbParams(83, 97, n_features=60)
    ex = orb.OrbExtractor(gpu_ctx, 1, P)
    try:
        ex.upload(img[None], m)
        ex.run()
        want = reference(img, P, m)
        for l in range(P.L):
            image, blurred, scores, (R, ys, xs) = ex.stage(0, l)
            w_image, w_blur, w_scores, (wR, wys, wxs) = want["stages"][l]
            assert np.array_equal(image, w_image), f"pyramid level {l}"
            assert np.array_equal(blurred, w_blur), f"blurred level {l}"
            assert np.array_equal(scores, w_scores), f"score map {l}"
            assert sorted(zip(R.tolist(), ys.tolist(), xs.tolist())) == sorted(zip(wR.tolist(), wys.tolist(), wxs.tolist())), f"candidates {l}"
        assert sum(len(s[3][0]) for s in want["stages"]) > 20 and any(s[2].any() for s in want["stages"])
        count, kp, resp, desc = ex.download()
        assert int(count[0]) == len(want["x"]) and np.array_equal(kp[0, :count[0], 0], want["x"])
        assert not kp[0, count[0]:].any() and not resp[0, count[0]:].any() and not desc[0, count[0]:].any()     # unused slots are zero
    finally:
        ex.free()


def test_batch_of_three_with_a_constant_image(gpu_ctx):
    from slamhip import orb

    imgs = np.stack([ref.scene(120, 160, 2, shapes=60), np.full((120, 160), 93, np.uint8), ref.noise(120, 160, 4)])
    P = orb.OrbParams(120, 160, n_features=200)
    res = orb.orb_extract_arrays(imgs, n_features=200, ctx=gpu_ctx)
    wants = [reference(imgs[b], P) for b in range(3)]
    assert len(wants[1]["x"]) == 0 and len(wants[0]["x"]) > 0 and len(wants[2]["x"]) > len(wants[0]["x"])
    for b in range(3):
        assert_same(res, b, wants[b], P)
    again = orb.orb_extract_arrays(imgs, n_features=200, ctx=gpu_ctx)                      # determinism: two runs are identical
    for b in range(3):
        assert_same(again, b, wants[b], P)
        one = orb.orb_extract_arrays(imgs[b], n_features=200, ctx=gpu_ctx)                 # and B = 3 equals three B = 1 calls
        assert_same(one, 0, wants[b], P)


def test_desk_fixture_all_levels(gpu_ctx):
    from slamhip import orb

    img = np.load(os.path.join(HERE, "golden", "orb_desk_320x240.npz"))["image"]
    assert img.shape == (240, 320) and img.dtype == np.uint8
    P = orb.OrbParams(240, 320, n_features=500, n_levels=8)
    want = reference(img, P)
    assert np.bincount(want["level"], minlength=8).tolist() == P.quota.tolist()             # every level is cut by its quota
    assert_same(orb.orb_extract_arrays(img, ctx=gpu_ctx), 0, want, P)


@pytest.mark.parametrize("image", ["noise", "tiled"])
def test_selection_cuts_a_dense_list(gpu_ctx, image):
    from slamhip import orb

    img = ref.noise(128, 128, 3) if image == "noise" else ref.tiled_noise(128, 128, 32, 5)
    for n_features, n_levels in ((40, 1), (1, 1), (90, 3)):
        P = orb.OrbParams(128, 128, n_features=n_features, n_levels=n_levels)
        want = reference(img, P)
        R = want["stages"][0][3][0]
        assert len(R) > 10 * P.quota[0]
        if image == "tiled" and n_levels == 1:                # the cut falls inside a run of equal R: y, x decide
            cut = np.sort(R)[::-1][P.quota[0] - 1]
            assert (R == cut).sum() > 1 and (R >= cut).sum() > P.quota[0]
        assert_same(orb.orb_extract_arrays(img, n_features=n_features, n_levels=n_levels, ctx=gpu_ctx), 0, want, P)
    P = orb.OrbParams(128, 128, n_features=len(R), n_levels=1)                               # exactly quota candidates
    assert_same(orb.orb_extract_arrays(img, n_features=len(R), n_levels=1, ctx=gpu_ctx), 0, reference(img, P), P)
    P = orb.OrbParams(128, 128, n_features=0, n_levels=2)
    assert orb.orb_extract_arrays(img, n_features=0, n_levels=2, ctx=gpu_ctx).counts.tolist() == [0]


@pytest.mark.parametrize("t", [5, 20, 60])
def test_mask_custom_pattern_and_thresholds(gpu_ctx, t):
    from slamhip import orb

    imgs = np.stack([ref.scene(120, 160, 8, shapes=70), ref.noise(120, 160, 9)])
    g = ref._Lcg(77)
    pat = np.zeros((256, 4), np.int8)
    for j in range(256):
        while True:
            p = [g.below(31) - 15 for _ in range(4)]
            if p[0] ** 2 + p[1] ** 2 <= 225 and p[2] ** 2 + p[3] ** 2 <= 225:
                break
        pat[j] = p
    shared = np.zeros((120, 160), np.uint8)
    shared[10:100, 30:150] = 255
    per_image = np.stack([shared, np.ones((120, 160), np.uint8)])
    per_image[1, :, 80:] = 0
    P = orb.OrbParams(120, 160, n_features=150, n_levels=5, fast_threshold=t, pattern=pat)
    for mask in (shared, per_image):
        res = orb.orb_extract_arrays(imgs, mask=mask, n_features=150, n_levels=5, fast_threshold=t, pattern=pat, ctx=gpu_ctx)
        for b in range(2):
            want = reference(imgs[b], P, mask if mask.ndim == 2 else mask[b])
            assert_same(res, b, want, P)
    zero = orb.orb_extract_arrays(imgs, mask=np.zeros((120, 160), np.uint8), n_features=150, fast_threshold=t, ctx=gpu_ctx)
    assert zero.counts.tolist() == [0, 0]
    assert len(want["x"]) > 0


def test_resident_descriptors_feed_the_matcher(gpu_ctx):
    import slamhip
    from slamhip import orb

    imgs = np.stack([ref.scene(120, 160, 2, shapes=60), ref.noise(120, 160, 4)])
    res = orb.orb_extract_arrays(imgs, n_features=200, ctx=gpu_ctx, keep_on_device=True)
    try:
        (dq, nq), (dt, nt) = res.device_descriptors(0), res.device_descriptors(1)
        assert nq == len(res.descriptors[0]) > 2 and nt == len(res.descriptors[1]) > 2
        tab = slamhip.Top2Table(gpu_ctx, nq)
        try:
            slamhip.knn2_device(gpu_ctx, dq, nq, dt, nt, tab.idx, tab.dist)
            idx, dist = tab.download()
        finally:
            tab.free()
        widx, wdist = slamhip.knn_match_arrays(res.descriptors[0], res.descriptors[1], 2, ctx=gpu_ctx)
        assert np.array_equal(idx, widx) and np.array_equal(dist, wdist)
    finally:
        res.free()


def test_detector_drop_in(gpu_ctx):
    from slamhip import orb

    img = np.load(os.path.join(HERE, "golden", "orb_desk_320x240.npz"))["image"]
    det = orb.OrbFeatureDetector(n_features=200)
    kps, desc = det.detect_and_compute(img, mask=None)
    only = det.detect(img)
    assert len(kps) == len(only) == len(desc) == 200 and desc.dtype == np.uint8 and desc.shape[1] == 32
    for a, b in zip(kps, only):
        assert (a.pt, a.size, a.angle, a.response, a.octave) == (b.pt, b.size, b.angle, b.response, b.octave)
    P = orb.OrbParams(240, 320, n_features=200)
    want = reference(img, P)
    assert np.array_equal(desc, want["descriptors"]) and [k.octave for k in kps] == want["level"].tolist()
    assert kps[0].pt == (float(want["x"][0]), float(want["y"][0])) and kps[0].size == 31.0 and kps[0].angle == 11.25 * want["bin"][0]
    m = np.zeros((240, 320), np.uint8)
    m[:, :160] = 255
    left, _ = det.detect_and_compute(img, m)
    assert 0 < len(left) and all(k.pt[0] < 161.0 for k in left)
    rgb = np.stack([img, img, img], 2)                       # gray from equal channels: (77 + 150 + 29) v + 128 >> 8 = v
    assert np.array_equal(det.detect_and_compute(rgb)[1], desc)


def test_abi_refusals_leave_outputs_and_context_intact(gpu_ctx):
    from slamhip import orb

    lib, ctx = gpu_ctx.lib, gpu_ctx
    img = ref.scene(83, 97, 11, shapes=80)
    P = orb.OrbParams(83, 97, n_features=60)
    ex = orb.OrbExtractor(ctx, 1, P)
    try:
        ex.upload(img[None])
        b = ex.bufs
        sentinel = np.full(16 * P.n_max, 0xA5, np.uint8)
        for k in ("kp", "resp", "desc"):
            b[k].upload(np.resize(sentinel, b[k].nbytes))
        b["count"].upload(np.full(4, 0xA5A5A5A5, np.uint32))

        def call(**kw):
            a = dict(ctx=ctx.handle, images=b["images"].ptr, B=1, H=83, W=97, mask=None, batched=0, L=P.L, lw=P.lw.ctypes.data,
                     lh=P.lh.ctypes.data, quota=P.quota.ctypes.data, t=20, table=b["table"].ptr, ws=b["ws"].ptr, ws_bytes=ex.ws_bytes,
                     count=b["count"].ptr, kp=b["kp"].ptr, resp=b["resp"].ptr, desc=b["desc"].ptr)
            a.update(kw)
            return lib.slam_orb_extract_u8(*a.values())

        big = np.full(P.L, 20000, np.int32)
        neg = P.quota.copy(); neg[2] = -1
        refused = [dict(ctx=None), dict(images=None), dict(table=None), dict(ws=None), dict(count=None), dict(desc=None), dict(kp=None),
                   dict(lw=None), dict(quota=None), dict(B=-1), dict(B=65536), dict(H=0), dict(W=8193), dict(H=84), dict(L=0), dict(L=17),
                   dict(ws_bytes=ex.ws_bytes - 1), dict(ws=b["ws"].ptr + 4), dict(quota=big.ctypes.data), dict(quota=neg.ctypes.data),
                   dict(t=0), dict(t=255)]
        for kw in refused:
            assert call(**kw) == -1, kw
            assert lib.slam_last_error()
        ctx.sync()
        for k in ("kp", "resp", "desc"):
            assert (b[k].download(np.uint8, (b[k].nbytes,)) == 0xA5).all(), k                # nothing was written
        assert (b["count"].download(np.uint32, (4,)) == 0xA5A5A5A5).all()
        assert call(B=0) == 0 and call(B=0, images=None, count=None) == 0                   # empty input: not an error, no write
        assert (b["count"].download(np.uint32, (4,)) == 0xA5A5A5A5).all()
        cnt = np.zeros(1, np.int32)
        host = lambda **kw: lib.slam_orb_extract_u8_host(*{**dict(ctx=ctx.handle, images=img.ctypes.data, B=1, H=83, W=97, mask=None, batched=0,
                                                                  L=P.L, lw=P.lw.ctypes.data, lh=P.lh.ctypes.data, quota=P.quota.ctypes.data, t=20,
                                                                  table=P.table.ctypes.data, count=cnt.ctypes.data, kp=None, resp=None, desc=None),
                                                           **kw}.values())
        assert host() == -1 and host(images=None) == -1 and host(L=99) == -1 and host(B=0) == 0
        assert call() == 0                                    # the context still works
        want = reference(img, P)
        count, kp, resp, desc = ex.download()
        assert int(count[0]) == len(want["x"]) and np.array_equal(desc[0, :count[0]], want["descriptors"])
    finally:
        ex.free()
