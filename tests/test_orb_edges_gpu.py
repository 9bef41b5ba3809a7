"""GPU: slam_orb_* at the limits of its contract, bit for bit against tests/orb_ref.py on the cases of
tests/orb_cases.py: tile seams and the first / last scoreable pixel, a candidate list filled to its proven capacity, levels and
images too small for a feature, the largest side, selection lists longer than the selection block with quotas above it, lists
tied on R, negative R, thresholds 1 and 254 on saturated values, moments on axes and diagonals, one-pixel masks, dirty
workspaces, a context whose shape changes from call to call, a batch above 64.  tests/test_orb_edges_cpu.py asserts, on the
restatement alone, that each case has the property it is here for.  Unless a test says otherwise it runs the host entry
(orb_extract_arrays) and the device entry (OrbExtractor).

Not reached: a moment exactly on a bin boundary (it would have to be an integer multiple of a boundary vector such as
(16305, 1606), which no image this small gives; orb_ref.orientation_bin is pinned there by tests/test_orb_cpu.py), and 256
survivors in one 64 x 16 tile (the tile's list holds 256 = one per 2 x 2 block, which only a perfect lattice of strict maxima
would fill)."""
import os

import numpy as np
import pytest

import orb_cases as C

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ONE = dict(n_features=100, n_levels=1)


# ---------------------------------------------------------------------------------------------------------------- helpers
def assert_same(res, b, want, P):
    """tests/test_orb_gpu.py's comparison, restated: counts, level coordinates, levels, bins, R, descriptors, converted fields."""
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


def assert_stages(ex, b, want, P):
    """Every stage buffer of image b: pyramid, blur and score planes, and the candidate list as a set (its order is the
    arrival order of the append)."""
    for l in range(P.L):
        image, blurred, scores, (R, ys, xs) = ex.stage(b, l)
        w_image, w_blur, w_scores, (wR, wys, wxs) = want["stages"][l]
        assert np.array_equal(image, w_image), f"pyramid level {l}"
        assert np.array_equal(blurred, w_blur), f"blurred level {l}"
        assert np.array_equal(scores, w_scores), f"score map {l}"
        assert sorted(zip(R.tolist(), ys.tolist(), xs.tolist())) == sorted(zip(wR.tolist(), wys.tolist(), wxs.tolist())), f"candidates {l}"


def assert_unused_slots_are_zero(count, kp, resp, desc):
    for b in range(len(count)):
        n = int(count[b])
        assert not kp[b, n:].any() and not resp[b, n:].any() and not desc[b, n:].any(), f"unused slots of image {b}"


def mask_of(mask, b):
    return None if mask is None else (mask if mask.ndim == 2 else mask[b])


def host_entry(ctx, P, imgs, mask=None):
    """slam_orb_extract_u8_host with the parameters of P (orb_extract_arrays with the quotas given, not derived); the output
    arrays start as 0xFF bytes, so a slot the call does not write shows."""
    from slamhip import orb
    from slamhip._lib import addr, check

    a, m, batched = orb._check_images(imgs, mask)
    B = a.shape[0]
    count, kp = np.full(B, -1, np.int32), np.full((B, P.n_max, 4), -1, np.int32)
    resp, desc = np.full((B, P.n_max), -1, np.int64), np.full((B, P.n_max, 32), 0xFF, np.uint8)
    check(ctx.lib.slam_orb_extract_u8_host(ctx.handle, addr(a), B, P.H, P.W, addr(m) if m is not None else None, batched, P.L, addr(P.lw),
                                           addr(P.lh), addr(P.quota), P.t, addr(P.table), addr(count), addr(kp), addr(resp), addr(desc)))
    assert_unused_slots_are_zero(count, kp, resp, desc)
    return orb.OrbResult(P, count, kp, resp, desc)


def device_entry(ctx, P, imgs, mask=None, stages=None, dirty=True):
    """slam_orb_extract_u8 on an OrbExtractor whose outputs (and, with dirty, workspace) start as garbage; with stages = the
    reference results, every stage buffer is compared too."""
    from slamhip import orb

    imgs = np.ascontiguousarray(imgs if imgs.ndim == 3 else imgs[None])
    ex = orb.OrbExtractor(ctx, len(imgs), P)
    try:
        if dirty:
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


def fill_with_garbage(ex):
    b = ex.bufs
    b["ws"].upload(np.full(b["ws"].nbytes, 0xFF, np.uint8))
    for k in ("kp", "resp", "desc", "count"):
        b[k].upload(np.full(b[k].nbytes, 0xA5, np.uint8))


def check_both(ctx, imgs, kw, mask=None, stages=False, P=None):
    """Both entries against the reference for every image of the batch; returns (P, reference results, host result)."""
    from slamhip import orb

    imgs = np.ascontiguousarray(imgs if imgs.ndim == 3 else imgs[None])
    derived = P is None
    P = P or orb.OrbParams(imgs.shape[1], imgs.shape[2], **kw)
    wants = [C.reference(imgs[b], P, mask_of(mask, b)) for b in range(len(imgs))]
    res = host_entry(ctx, P, imgs, mask)
    for b, want in enumerate(wants):
        assert_same(res, b, want, P)
    dev = device_entry(ctx, P, imgs, mask, stages=wants if stages else None)
    for b, want in enumerate(wants):
        assert_same(dev, b, want, P)
    if derived:                                               # and through the Python entry, which derives the same parameters
        top = orb.orb_extract_arrays(imgs, mask=mask, ctx=ctx, **kw)
        for b, want in enumerate(wants):
            assert_same(top, b, want, P)
    return P, wants, res


# ------------------------------------------------------------------------------------------------------------------ 1: seams
def test_dots_on_tile_seams_and_on_the_first_and_last_pixel(gpu_ctx):
    P, (want,), res = check_both(gpu_ctx, C.seam_dots(), ONE, stages=True)
    assert [tuple(p) for p in res.xy_level[0].tolist()] == C.SEAM_ORDER
    assert res.response[0].tolist() == [C.R_255] * 8
    assert [b for b, w in zip(res.bin[0].tolist(), C.SEAM_BINS) if w is not None] == [w for w in C.SEAM_BINS if w is not None]


def test_equal_scores_across_a_seam_both_drop(gpu_ctx):
    from slamhip import orb

    img = C.seam_pairs()
    P, (want,), res = check_both(gpu_ctx, img, ONE, stages=True)
    assert [tuple(p) for p in res.xy_level[0].tolist()] == [C.PAIR_KEPT] and res.bin[0].tolist() == [24]
    ex = orb.OrbExtractor(gpu_ctx, 1, P)
    try:
        fill_with_garbage(ex)
        ex.upload(img[None])
        ex.run()
        scores = ex.stage(0, 0)[2]
        assert [int(scores[y, x]) for x, y in C.PAIR_TIED] == [254] * 4           # both tiles computed the halo score
        assert int(scores[15, 100]) == 0 and int(scores[16, 100]) == 254 and int((scores > 0).sum()) == 5
        ex.upload(C.seam_unequal_pair()[None])
        ex.run()
        scores, (R, ys, xs) = ex.stage(0, 0)[2:]
        assert scores[24, 63:65].tolist() == [254, 199] and (xs.tolist(), ys.tolist()) == ([63], [24])
    finally:
        ex.free()
    P, _, res = check_both(gpu_ctx, C.seam_unequal_pair(), ONE, stages=True)
    assert res.xy_level[0].tolist() == [[63, 24]]


def test_candidate_list_filled_to_its_capacity(gpu_ctx):
    for img, n in C.capacity_cases():
        P, (want,), res = check_both(gpu_ctx, img, ONE, stages=True)
        assert int(P.workspace(1)[1]["capacity"][0]) == n == int(res.counts[0]) == len(want["stages"][0][3][0])


# ------------------------------------------------------------------------------------------------------------------ 2: sizes
@pytest.mark.parametrize("h,w,kw", [(h, w, C.TOO_SMALL_KW) for h, w in C.TOO_SMALL] + [(2, 2, C.TINY_SCALE4_KW)])
def test_images_too_small_for_any_feature(gpu_ctx, h, w, kw):
    P, (want,), res = check_both(gpu_ctx, C.too_small_image(h, w), kw, stages=True)      # planes of dead levels are still computed
    assert res.counts.tolist() == [0] and (np.minimum(P.lh, P.lw) < 33).all() and P.n_max == 50


@pytest.mark.parametrize("h,w", list(C.STRIP_COUNTS))
def test_strips_at_the_largest_side(gpu_ctx, h, w):
    P, (want,), res = check_both(gpu_ctx, C.strip(h, w), C.STRIP_KW, stages=True)
    assert int(res.counts[0]) == C.STRIP_COUNTS[(h, w)] and int(res.xy_level[0].max()) > 8100 and (res.level[0] == 1).any()


@pytest.mark.parametrize("name", list(C.LEVEL_CASES))
def test_sixteen_levels_and_other_scales(gpu_ctx, name):
    P, (want,), res = check_both(gpu_ctx, C.level_image(), C.LEVEL_CASES[name], stages=True)
    if name == "sixteen":
        assert np.bincount(res.level[0], minlength=16).tolist() == C.SIXTEEN_PER_LEVEL


# -------------------------------------------------------------------------------------------------------------- 3: selection
def test_selection_of_a_list_four_times_the_block(gpu_ctx):
    from slamhip import orb

    img = C.long_list_image()
    n = len(C.reference(img, orb.OrbParams(256, 256, n_features=orb.MAX_FEATURES, n_levels=1))["x"])
    assert n > 4096
    for quota in C.long_list_quotas(n):
        P, (want,), res = check_both(gpu_ctx, img, dict(n_features=quota, n_levels=1))
        assert int(res.counts[0]) == min(quota, n)


def test_selection_when_every_candidate_ties_on_R(gpu_ctx):
    for quota in C.ALL_TIED_QUOTAS:
        P, (want,), res = check_both(gpu_ctx, C.all_tied_image(), dict(n_features=quota, n_levels=1))
        assert [tuple(p) for p in res.xy_level[0].tolist()] == C.ALL_TIED_ORDER[:quota]          # decided in the last four digits
        assert res.response[0].tolist() == [C.R_255] * quota and not res.bin[0].any()
        if quota == 50:
            assert res.xy_level[0][-1].tolist() == [28, 52]


def test_negative_R_ranks_last_and_is_cut_first(gpu_ctx):
    img = C.mixed_sign_image()
    P, (want,), res = check_both(gpu_ctx, img, C.MIXED_SIGN_KW)
    R, lv = res.response[0], res.level[0]
    assert len(R) == 193 and int((R < 0).sum()) == 3
    for l in range(3):
        assert (np.diff(R[lv == l]) <= 0).all() and R[lv == l][-1] < 0 and (R[lv == l][:-1] >= 0).all()     # negatives last in their level
    cut = C.quota_above_the_negatives(want)
    _, (wc,), rc = check_both(gpu_ctx, img, None, P=C.with_quota(P, cut))
    assert int(rc.counts[0]) == 190 and (rc.response[0] >= 0).all()
    _, _, rc = check_both(gpu_ctx, img, None, P=C.with_quota(P, cut - 1))                 # and one above the cut
    assert int(rc.counts[0]) == 187 and (rc.response[0] >= 0).all()


def test_saturated_rectangles_large_R_and_ties(gpu_ctx):
    for quota in C.SATURATED_QUOTAS:
        P, (want,), res = check_both(gpu_ctx, C.saturated_rectangles(), dict(n_features=quota, n_levels=1), stages=True)
        assert int(res.counts[0]) == min(quota, 22) and int(res.response[0].max()) > C.R_255


# ------------------------------------------------------------------------------------------------------------ 4: value range
@pytest.mark.parametrize("t", [1, 254])
def test_thresholds_at_both_ends(gpu_ctx, t):
    kw = dict(n_features=1000, n_levels=1, fast_threshold=t)
    P, (want,), res = check_both(gpu_ctx, C.threshold_noise(), kw, stages=True)
    assert int(res.counts[0]) == (179 if t == 1 else 0)
    P, (want,), res = check_both(gpu_ctx, C.threshold_dots(), kw, stages=True)
    assert res.xy_level[0].tolist() == ([[50, 20], [30, 30], [40, 40]] if t == 1 else [[50, 20], [30, 30]])
    assert res.response[0].tolist() == [C.R_255, C.R_255, C.dot_R(254)][:len(res.response[0])]
    P, (want,), res = check_both(gpu_ctx, C.inverse_dots(), kw, stages=True)
    assert res.xy_level[0].tolist() == [[50, 20], [30, 30]] and res.bin[0].tolist() == [0, 0] and res.response[0].tolist() == [C.R_255] * 2


def test_moments_on_axes_and_diagonals(gpu_ctx):
    imgs = C.axis_batch()
    P, wants, res = check_both(gpu_ctx, imgs, C.AXIS_KW, stages=True)
    assert res.counts.tolist() == [1] * 8
    assert [res.bin[b].tolist() for b in range(8)] == [[0], [4], [8], [12], [16], [20], [24], [28]]
    assert all(res.xy_level[b].tolist() == [[32, 32]] and res.response[b].tolist() == [C.R_255] for b in range(8))


# --------------------------------------------------------------------------------------------------------------------- 5: mask
def test_one_pixel_checkerboard_masks(gpu_ctx):
    img = C.mask_image()
    m, inv = C.checkerboard(), C.checkerboard_inverse()
    P, (want,), res = check_both(gpu_ctx, img, C.MASK_KW, mask=m)                          # unbatched, value 7
    assert int(res.counts[0]) == 539
    P, wants, both = check_both(gpu_ctx, np.stack([img, img]), C.MASK_KW, mask=np.stack([m, inv]))
    _, (full,), plain = check_both(gpu_ctx, img, C.MASK_KW)
    key = lambda r, b: set(zip(r.level[b].tolist(), r.xy_level[b][:, 0].tolist(), r.xy_level[b][:, 1].tolist()))
    assert not (key(both, 0) & key(both, 1)) and key(both, 0) | key(both, 1) == key(plain, 0)     # holds without the reference
    assert both.counts.tolist() == [539, 512] and int(plain.counts[0]) == 1051


# ------------------------------------------------------------------------------------------------------- 6: state and batch
def test_dirty_workspace_and_outputs_then_a_second_run(gpu_ctx):
    from slamhip import orb

    imgs = C.dirty_batch()
    P = orb.OrbParams(83, 97, **C.DIRTY_KW)
    ex = orb.OrbExtractor(gpu_ctx, 2, P)
    try:
        fill_with_garbage(ex)
        for batch in (imgs, C.dense_and_constant()):          # the second run starts from the first one's leftovers
            ex.upload(batch)
            ex.run()
            out = ex.download()
            res = orb.OrbResult(P, *out)
            assert_unused_slots_are_zero(*out)
            lay = ex.layout
            for b in range(2):
                want = C.reference(batch[b], P)
                assert_same(res, b, want, P)
                assert_stages(ex, b, want, P)
                for l in range(P.L):                          # bytes between the level's width and its pitch are written as zero
                    h, w, pitch = int(P.lh[l]), int(P.lw[l]), int(lay["pitch"][l])
                    for k in ("image", "blur", "score"):
                        plane = ex.bufs["ws"].view(lay["image_base"] + b * lay["image_stride"] + int(lay[k][l]), pitch * h)
                        assert not plane.download(np.uint8, (h, pitch))[:, w:].any(), (k, l)
        assert int(out[0][1]) == 0 and int(out[0][0]) > 0
        counters = ex.bufs["ws"].view(lay["counts"] + 4 * 16, 4 * P.L).download(np.int32, (P.L,))
        assert counters.tolist() == [0] * P.L                 # the constant image: no candidate on any level
    finally:
        ex.free()


def test_one_context_through_changing_shapes(gpu_ctx):
    from slamhip import orb

    desk = np.load(os.path.join(HERE, "golden", "orb_desk_320x240.npz"))["image"]
    m = np.zeros((83, 97), np.uint8)
    m[:, 20:] = 3
    calls = [(desk, dict(n_features=500, n_levels=8), None), (C.capacity_cases()[0][0], ONE, None),
             (C.strip(40, 8192), C.STRIP_KW, None), (C.level_image(), C.LEVEL_CASES["sixteen"], m),
             (desk, dict(n_features=500, n_levels=8), None)]
    results = []
    for img, kw, mask in calls:                               # the host entry: the context's workspace and staging arena are reused
        P = orb.OrbParams(img.shape[0], img.shape[1], **kw)
        res = orb.orb_extract_arrays(img, mask=mask, ctx=gpu_ctx, **kw)
        assert_same(res, 0, C.reference(img, P, mask), P)
        results.append(res)
    first, last = results[0], results[-1]
    assert int(first.counts[0]) == int(last.counts[0]) == 500
    for k in ("xy_level", "level", "bin", "response", "descriptors"):
        assert np.array_equal(getattr(first, k)[0], getattr(last, k)[0]), k


def test_batch_of_70(gpu_ctx):
    from slamhip import orb

    imgs = C.big_batch()
    P, wants, res = check_both(gpu_ctx, imgs, C.BIG_BATCH_KW)
    assert len(res) == 70 and 10 <= int(res.counts.min()) and int(res.counts.max()) <= 20
    for b in (0, 33, 69):                                     # the batch equals single calls
        one = orb.orb_extract_arrays(imgs[b], ctx=gpu_ctx, **C.BIG_BATCH_KW)
        assert_same(one, 0, wants[b], P)
        for k in ("xy_level", "bin", "response", "descriptors"):
            assert np.array_equal(getattr(one, k)[0], getattr(res, k)[b]), k
