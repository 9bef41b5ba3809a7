"""GPU: slam_orb_extract_dist_u8 (the quadtree keypoint distribution with an adaptive FAST threshold) bit for bit
against tests/orb_dist_ref.py: counts, level coordinates, levels, bins, R and descriptors, and the stage buffers of a run at the
lower threshold.  Every run starts from a workspace of 0xFF bytes and outputs of 0xA5 bytes and checks that unused slots are zero.
The hand-made cases are those of tests/orb_dist_cases.py, which tests/test_orb_dist_cpu.py holds the statement to."""
import os

import numpy as np
import pytest

import orb_cases as C
import orb_dist_cases as D
import orb_ref as ref
from test_orb_edges_gpu import assert_same, assert_stages, assert_unused_slots_are_zero, fill_with_garbage

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def params(img_shape, quota=None, **kw):
    """OrbParams of the quadtree mode; `quota` replaces the per-level quotas of the geometric rule."""
    from slamhip import orb

    P = orb.OrbParams(img_shape[-2], img_shape[-1], distribution="quadtree", **kw)
    return P if quota is None else C.with_quota(P, quota)


def run(ctx, P, imgs, mask=None, stages=None):
    """One call on a fresh extractor whose workspace and outputs start as garbage; returns the OrbResult."""
    from slamhip import orb

    imgs = np.ascontiguousarray(imgs if imgs.ndim == 3 else imgs[None])
    ex = orb.OrbExtractor(ctx, len(imgs), P)
    try:
        fill_with_garbage(ex)
        ex.upload(imgs, mask)
        ex.run()
        out = ex.download()
        assert_unused_slots_are_zero(*out)
        if stages is not None:
            for b, want in enumerate(stages):
                assert_stages(ex, b, want, P)
        return orb.OrbResult(P, *out)
    finally:
        ex.free()


def check(ctx, imgs, P, mask=None, stages=True):
    imgs = np.ascontiguousarray(imgs if imgs.ndim == 3 else imgs[None])
    wants = [D.reference(imgs[b], P, None if mask is None else (mask if mask.ndim == 2 else mask[b])) for b in range(len(imgs))]
    res = run(ctx, P, imgs, mask, stages=wants if stages else None)
    for b, want in enumerate(wants):
        assert_same(res, b, want, P)
    return wants, res


# ------------------------------------------------------------------------------------------------------------ scenes
@pytest.mark.parametrize("h,w,seed", [(83, 97, 11), (70, 131, 5)])
@pytest.mark.parametrize("t_min", [20, 7])
@pytest.mark.parametrize("masked", [False, True])
def test_scenes_at_eight_levels(gpu_ctx, h, w, seed, t_min, masked):
    img = ref.scene(h, w, seed, shapes=80)
    mask = None
    if masked:
        mask = np.ones((h, w), np.uint8)
        mask[:, w // 3:w // 2] = 0
        mask[h // 2:, :20] = 0
    P = params(img.shape, n_features=60, n_levels=8, fast_threshold_min=t_min)
    assert w % 4 and (np.minimum(P.lh, P.lw) < 33).any() and (np.minimum(P.lh, P.lw) >= 33).any()
    (want,), res = check(gpu_ctx, img, P, mask)
    assert int(res.counts[0]) == sum(min(int(q), n) for q, n in zip(P.quota, want["live"])) > 0
    assert any(n > int(q) > 0 for q, n in zip(P.quota, want["live"]))           # the tree decides on at least one level


@pytest.mark.parametrize("case", D.cases(), ids=lambda c: c.name)
def test_hand_made_case(gpu_ctx, case):
    P = params(case.img.shape, quota=[case.quota], n_features=case.quota, n_levels=1, fast_threshold=case.t_ini, fast_threshold_min=case.t_min)
    (want,), res = check(gpu_ctx, case.img, P)
    assert [tuple(p) for p in res.xy_level[0].tolist()] == case.want


# --------------------------------------------------------------------------------------------------------- long lists
def test_a_list_longer_than_four_strides_of_the_block(gpu_ctx):
    img = C.long_list_image()
    n = len(ref.candidates(img, 20)[0])
    assert n > 4 * C.SEL_THREADS
    for quota in (1100, n - 1, n, n + 500):
        P = params(img.shape, n_features=quota, n_levels=1)
        (want,), res = check(gpu_ctx, img, P, stages=False)
        assert int(res.counts[0]) == min(quota, n)


def test_candidates_tied_on_R(gpu_ctx):
    for quota in C.ALL_TIED_QUOTAS:
        P = params((128, 128), n_features=quota, n_levels=1)
        (want,), res = check(gpu_ctx, C.all_tied_image(), P, stages=False)
        assert int(res.counts[0]) == quota and res.response[0].tolist() == [C.R_255] * quota
    assert [tuple(p) for p in res.xy_level[0].tolist()] == C.ALL_TIED_ORDER          # all 144: one per node, ranked by (y, x)


@pytest.mark.parametrize("n_levels", [1, 8])
def test_desk_fixture(gpu_ctx, n_levels):
    desk = np.load(os.path.join(HERE, "golden", "orb_desk_320x240.npz"))["image"]
    for t_min in (20, 7):
        P = params(desk.shape, n_features=500 if n_levels == 8 else 50, n_levels=n_levels, fast_threshold_min=t_min)
        (want,), res = check(gpu_ctx, desk, P, stages=t_min == 7)
        assert int(res.counts[0]) == P.n_max


# ------------------------------------------------------------------------------------------ equality with the Harris entry
def test_equal_thresholds_and_a_large_quota_equal_the_harris_entry(gpu_ctx):
    from slamhip import orb

    img = ref.scene(83, 97, 11, shapes=80)
    Ph = orb.OrbParams(83, 97, n_features=4000, n_levels=6)
    Pq = params(img.shape, n_features=4000, n_levels=6)
    ex = orb.OrbExtractor(gpu_ctx, 1, Ph)
    try:
        fill_with_garbage(ex)
        ex.upload(img[None])
        ex.run()
        a = ex.download()
        n_cand = [len(ex.stage(0, l)[3][0]) for l in range(6)]
    finally:
        ex.free()
    assert all(n <= int(q) for n, q in zip(n_cand, Ph.quota)) and sum(n_cand) > 50       # a quota at or above every candidate count
    exq = orb.OrbExtractor(gpu_ctx, 1, Pq)
    try:
        fill_with_garbage(exq)
        exq.upload(img[None])
        exq.run()
        b = exq.download()
    finally:
        exq.free()
    assert_unused_slots_are_zero(*b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    assert int(b[0][0]) == sum(n_cand)


# ------------------------------------------------------------------------------------------------------ state and batch
def test_two_runs_on_garbage_are_identical(gpu_ctx):
    from slamhip import orb

    imgs = np.stack([ref.scene(83, 97, 11, shapes=80), ref.noise(83, 97, 21)])
    P = params(imgs.shape, n_features=150, n_levels=4, fast_threshold_min=7)
    ex = orb.OrbExtractor(gpu_ctx, 2, P)
    try:
        outs = []
        for _ in range(2):
            fill_with_garbage(ex)
            ex.upload(imgs)
            ex.run()
            outs.append(ex.download())
            assert_unused_slots_are_zero(*outs[-1])
        for x, y in zip(*outs):
            assert np.array_equal(x, y)
        ex.run()                                                          # and once more on its own leftovers
        for x, y in zip(outs[0], ex.download()):
            assert np.array_equal(x, y)
        res = orb.OrbResult(P, *outs[0])
        for b in range(2):
            assert_same(res, b, D.reference(imgs[b], P), P)
    finally:
        ex.free()


def test_batch_of_three_with_a_constant_image(gpu_ctx):
    imgs = np.stack([ref.scene(83, 97, 11, shapes=80), np.full((83, 97), 140, np.uint8), ref.noise(83, 97, 22)])
    P = params(imgs.shape, n_features=100, n_levels=4, fast_threshold_min=7)
    wants, res = check(gpu_ctx, imgs, P)
    assert int(res.counts[1]) == 0 and int(res.counts[0]) > 0 and int(res.counts[2]) > 0
    for b in (0, 2):                                                      # the batch equals single calls
        one = run(gpu_ctx, P, imgs[b])
        assert_same(one, 0, wants[b], P)


def test_argument_errors_leave_the_outputs_untouched(gpu_ctx):
    from slamhip import orb
    from slamhip._lib import SLAM_ERR_INVALID, addr

    img = ref.scene(83, 97, 11, shapes=80)
    P = params(img.shape, n_features=100, n_levels=3)
    ex = orb.OrbExtractor(gpu_ctx, 1, P)
    try:
        fill_with_garbage(ex)
        ex.upload(img[None])
        b, lib = ex.bufs, gpu_ctx.lib

        def call(t=20, t_min=20, ws_bytes=ex.ws_bytes, ws=b["ws"].ptr, B=1, quota=P.quota, images=b["images"].ptr, count=b["count"].ptr):
            return lib.slam_orb_extract_dist_u8(gpu_ctx.handle, images, B, P.H, P.W, None, 0, P.L, addr(P.lw), addr(P.lh), addr(quota), t, t_min,
                                                b["table"].ptr, ws, ws_bytes, count, b["kp"].ptr, b["resp"].ptr, b["desc"].ptr)

        harris_bytes = orb.OrbParams(83, 97, n_features=100, n_levels=3).workspace(1)[0]
        assert harris_bytes < ex.ws_bytes
        bad_quota = np.asarray([10, -1, 5], np.int32)
        for kw in (dict(t_min=0), dict(t_min=21), dict(t=255, t_min=20), dict(t=0, t_min=0), dict(ws_bytes=ex.ws_bytes - 1),
                   dict(ws_bytes=harris_bytes), dict(ws=b["ws"].ptr + 4), dict(ws=None), dict(B=-1), dict(quota=bad_quota), dict(images=None),
                   dict(count=None)):
            assert call(**kw) == SLAM_ERR_INVALID, kw
        gpu_ctx.sync()
        for k in ("kp", "resp", "desc", "count"):
            assert (b[k].download(np.uint8, (b[k].nbytes,)) == 0xA5).all(), k
        assert (b["ws"].download(np.uint8, (b["ws"].nbytes,)) == 0xFF).all()
        assert call(B=0) == 0                                             # not an error, and nothing happens
        gpu_ctx.sync()
        assert (b["count"].download(np.uint8, (b["count"].nbytes,)) == 0xA5).all()
        assert call() == 0
        res = orb.OrbResult(P, *ex.download())
        assert_same(res, 0, D.reference(img, P), P)
    finally:
        ex.free()


# ------------------------------------------------------------------------------------------------------- Python entries
def test_python_entries_take_the_mode(gpu_ctx):
    from slamhip import orb

    desk = np.load(os.path.join(HERE, "golden", "orb_desk_320x240.npz"))["image"]
    kw = dict(n_features=200, n_levels=4)
    P = params(desk.shape, fast_threshold_min=7, **kw)
    want = D.reference(desk, P)
    for keep in (False, True):
        res = orb.orb_extract_arrays(desk, ctx=gpu_ctx, keep_on_device=keep, distribution="quadtree", fast_threshold_min=7, **kw)
        assert_same(res, 0, want, P)
        if keep:
            buf, n = res.device_descriptors(0)
            assert n == len(want["x"]) and np.array_equal(buf.download(np.uint8, (n, 32)), want["descriptors"])
        res.free()
    det = orb.OrbFeatureDetector.quadtree(200, fast_threshold_min=7)
    try:
        P8 = params(desk.shape, n_features=200, fast_threshold_min=7)
        mask = np.ones(desk.shape, np.uint8)
        mask[:, :100] = 0
        for m in (None, mask, None):                                      # one extractor per shape, with and without a mask
            kps, desc = det.detect_and_compute(desk, m)
            w8 = D.reference(desk, P8, m)
            assert np.array_equal(desc, w8["descriptors"]) and [k.octave for k in kps] == w8["level"].tolist()
        assert len(det._extractors) == 1
        rgb = np.stack([desk[:100, :120]] * 3, axis=2)
        assert len(det.detect(rgb)) > 0 and len(det._extractors) == 2
    finally:
        det.free()
    plain = orb.OrbFeatureDetector(200)                                   # the default path is today's
    kps, desc = plain.detect_and_compute(desk)
    Ph = orb.OrbParams(240, 320, n_features=200)
    assert np.array_equal(desc, C.reference(desk, Ph)["descriptors"]) and not plain._extractors
