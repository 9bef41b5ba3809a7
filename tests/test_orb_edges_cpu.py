"""CPU: the edge cases of tests/orb_cases.py on the numpy restatement alone.  For every case the condition that makes it bite
(more candidates than selection threads, a full candidate list, a dead level, a negative R among the kept, ...) is asserted
here, where no GPU is needed, and the closed forms of the dot images (score, R, order, bins on axes and diagonals) are checked
against orb_ref.py, which pins the restatement independently of the product.  tests/test_orb_edges_gpu.py then compares the
device with the restatement on the same cases, bit for bit."""
import numpy as np
import pytest

import orb_cases as C
import orb_ref as ref
from slamhip import orb


def params(img, **kw):
    return orb.OrbParams(img.shape[-2], img.shape[-1], **kw)


ONE = dict(n_features=100, n_levels=1)


# ------------------------------------------------------------------------------------------------------------------ 1: seams
def test_closed_forms_of_a_dot():
    for fg, bg in ((255, 0), (0, 255), (254, 0), (200, 0), (77, 140), (140, 77)):
        img = C.dot_image(40, 44, [(20, 19, fg)], bg)
        assert int(ref.fast_scores(img, 1)[19, 20]) == C.dot_score(fg, bg) == abs(fg - bg) - 1
        assert int(ref.harris(img, [19], [20])[0]) == C.dot_R(fg, bg) == 3024 * (fg - bg) ** 4
        assert [int(m[0]) for m in ref.moments(img, [19], [20])] == [0, 0]
        R, ys, xs = ref.candidates(img, 1)
        assert (xs.tolist(), ys.tolist()) == ([20], [19])
    assert C.dot_R(255) == 12786229890000 == C.R_255


def test_seam_dots_sit_on_every_seam_and_on_the_first_and_last_pixel():
    img = C.seam_dots()
    P = params(img, **ONE)
    assert img.shape == (65, 145) and (145 + 3) // 4 * 4 == 148 and (-(-145 // 64), -(-65 // 16)) == (3, 5) and 145 % 64 and 65 % 16
    xs, ys = {d[0] for d in C.SEAM_DOTS}, {d[1] for d in C.SEAM_DOTS}
    assert {16, 63, 64, 127, 128} <= xs and 128 == 145 - 17 and {16, 31, 32, 48} <= ys and 48 == 65 - 17     # 15 is in the border
    r = C.reference(img, P)
    assert C.xy(r) == C.SEAM_ORDER == sorted(((x, y) for x, y, _ in C.SEAM_DOTS), key=lambda p: (p[1], p[0]))
    assert r["response"].tolist() == [C.R_255] * 8                              # all R tie: (y, x) decides the order
    scores = r["stages"][0][2]
    assert [int(scores[y, x]) for x, y in C.SEAM_ORDER] == [254] * 8 and int((scores > 0).sum()) == 8
    by_xy = {(x, y): i for i, (x, y, _) in enumerate(C.SEAM_DOTS)}
    for (x, y), b, want in zip(C.SEAM_ORDER, r["bin"].tolist(), C.SEAM_BINS):
        m = C.dot_moment(C.SEAM_DOTS, by_xy[(x, y)])
        assert [int(v[0]) for v in ref.moments(img, [y], [x])] == list(m)
        if want is not None:                                 # the moment is (0, 0) or on an axis: the bin is known by hand
            assert b == want == C.bin_of_direction(*m)
    assert C.SEAM_BINS.count(0) >= 4 and C.SEAM_BINS.count(None) == 1


def test_pairs_across_a_seam_drop_and_the_border_neighbour_does_not_count():
    img = C.seam_pairs()
    r = C.reference(img, params(img, **ONE))
    scores = r["stages"][0][2]
    assert {(63, 24), (64, 24)} <= set(C.PAIR_TIED) and {(40, 31), (40, 32)} <= set(C.PAIR_TIED)     # one pair per seam direction
    assert [int(scores[y, x]) for x, y in C.PAIR_TIED] == [254] * 4 and int(scores[15, 100]) == 0 and int(scores[16, 100]) == 254
    assert C.xy(r) == [C.PAIR_KEPT] and r["bin"].tolist() == [C.bin_of_direction(*C.dot_moment(C.PAIR_DOTS, 4))] == [24]
    img = C.seam_unequal_pair()
    r = C.reference(img, params(img, **ONE))
    assert C.xy(r) == [(63, 24)] and r["stages"][0][2][24, 63:65].tolist() == [254, 199]


def test_capacity_is_reached_exactly(built):
    for img, n in C.capacity_cases():
        P = params(img, **ONE)
        r = C.reference(img, P)
        h, w = img.shape
        assert len(r["x"]) == len(r["stages"][0][3][0]) == n == C.capacity(h, w) == -(-(w - 32) // 2) * -(-(h - 32) // 2)
        assert int(P.workspace(1)[1]["capacity"][0]) == n
    assert C.xy(C.reference(C.capacity_cases()[0][0], params(C.capacity_cases()[0][0], **ONE))) == [(16, 16)]
    r = C.reference(C.capacity_cases()[1][0], params(C.capacity_cases()[1][0], **ONE))
    assert C.xy(r) == [(16, 16), (18, 16), (16, 18), (18, 18)] and len(set(r["response"].tolist())) == 1


# ------------------------------------------------------------------------------------------------------------------ 2: sizes
def test_images_too_small_for_any_feature():
    for h, w in C.TOO_SMALL:
        P = orb.OrbParams(h, w, **C.TOO_SMALL_KW)
        assert (np.minimum(P.lh, P.lw) < 33).all() and max(h, w) >= 1
        r = C.reference(C.too_small_image(h, w), P)
        assert len(r["x"]) == 0 and all(s[0].shape == s[1].shape == (P.lh[l], P.lw[l]) for l, s in enumerate(r["stages"]))
    assert any(max(h, w) >= 33 for h, w in C.TOO_SMALL) and (33, 4) in C.TOO_SMALL              # one side alive is not enough
    P = orb.OrbParams(2, 2, **C.TINY_SCALE4_KW)
    assert ref.level_sizes(2, 2, 3, 4.0)[0].tolist() == [2, 0, 0] and P.lh.tolist() == P.lw.tolist() == [2, 1, 1]   # clamped by the binding
    assert len(C.reference(C.too_small_image(2, 2), P)["x"]) == 0


@pytest.mark.parametrize("h,w", list(C.STRIP_COUNTS))
def test_strips_at_the_largest_side(h, w):
    P = orb.OrbParams(h, w, **C.STRIP_KW)
    assert max(h, w) == orb.MAX_SIDE == 8192 and min(P.lh[1], P.lw[1]) == 33 and -(-8192 // 64) == 128
    r = C.reference(C.strip(h, w), P)
    assert len(r["x"]) == C.STRIP_COUNTS[(h, w)] and len(r["x"]) < P.quota.min()
    assert max(int(r["x"].max()), int(r["y"].max())) > 8100 and C.per_level(r, 2)[1] > 0       # x | y << 16 above 4096; level 1 alive


def test_dead_and_live_levels():
    img = C.level_image()
    P = params(img, **C.LEVEL_CASES["sixteen"])
    r = C.reference(img, P)
    assert (np.minimum(P.lh, P.lw)[:6] >= 33).all() and (np.minimum(P.lh, P.lw)[6:] < 33).all() and P.L == 16
    assert C.per_level(r, 16) == C.SIXTEEN_PER_LEVEL
    P = params(img, **C.LEVEL_CASES["scale2"])
    r = C.reference(img, P)
    assert (P.lh.tolist(), P.lw.tolist()) == ([83, 42, 21], [97, 48, 24])
    n = C.per_level(r, 3)
    assert n[0] > 0 and n[1] > 0 and n[2] == 0
    P = params(img, **C.LEVEL_CASES["scale1.05"])
    r = C.reference(img, P)
    assert (np.minimum(P.lh, P.lw) >= 33).all() and min(C.per_level(r, 16)) > 0


# -------------------------------------------------------------------------------------------------------------- 3: selection
def long_list_count():
    img = C.long_list_image()
    return len(C.reference(img, params(img, n_features=orb.MAX_FEATURES, n_levels=1))["x"])


def test_long_list_runs_every_strided_loop_more_than_once():
    img = C.long_list_image()
    n = long_list_count()
    assert n > 4096 == 4 * C.SEL_THREADS and n <= C.capacity(256, 256)
    q = C.long_list_quotas(n)
    assert n > q[0] > C.SEL_THREADS and q[1] == n - 1 and q[2] == n and q[3] > n and q[3] <= orb.MAX_FEATURES and q[4] == 1
    full = C.reference(img, params(img, n_features=orb.MAX_FEATURES, n_levels=1))
    assert sorted(set(full["bin"].tolist())) == list(range(32))                 # every bin and every row of the steered table
    for quota in q:
        r = C.reference(img, params(img, n_features=quota, n_levels=1))
        assert len(r["x"]) == min(quota, n) and C.xy(r) == C.xy(full)[:quota]


def test_all_tied_list_is_cut_in_raster_order():
    img = C.all_tied_image()
    for quota in C.ALL_TIED_QUOTAS:
        r = C.reference(img, params(img, n_features=quota, n_levels=1))
        R = r["stages"][0][3][0]
        assert len(R) == 144 and R.tolist() == [C.R_255] * 144                  # all eight leading key digits equal
        assert C.xy(r) == C.ALL_TIED_ORDER[:quota] and set(r["bin"].tolist()) == {0}
    assert C.ALL_TIED_ORDER[49] == (28, 52) and C.ALL_TIED_QUOTAS == [1, 50, 143, 144]


def test_mixed_signs_among_the_kept():
    img = C.mixed_sign_image()
    P = params(img, **C.MIXED_SIGN_KW)
    r = C.reference(img, P)
    R, lv = r["response"], r["level"]
    assert len(R) == 193 and int((R < 0).sum()) == 3 and (R > 0).any()
    for l in range(3):
        neg = np.nonzero(R[lv == l] < 0)[0]
        assert len(neg) == 0 or neg.tolist() == list(range((lv == l).sum() - len(neg), (lv == l).sum()))      # negatives last
    cut = C.quota_above_the_negatives(r)
    have = np.asarray([len(s[3][0]) for s in r["stages"]])
    assert (cut < have).any() and (cut > 0).all()                               # the radix select runs with a negative R left out
    rc = C.reference(img, C.with_quota(P, cut))
    assert len(rc["x"]) == cut.sum() == 190 and (rc["response"] >= 0).all()


def test_saturated_rectangles_have_large_and_tied_R():
    img = C.saturated_rectangles()
    assert set(np.unique(img).tolist()) == {0, 255} and np.array_equal(img, img[:, ::-1])
    r = C.reference(img, params(img, n_features=1000, n_levels=1))
    R = r["response"]
    assert len(R) == 22 and int(R.max()) > C.R_255 == 3024 * 255 ** 4 and C.R_255 in R.tolist()
    vals, counts = np.unique(R, return_counts=True)
    assert (counts >= 2).all() and len(vals) >= 5                               # ties by symmetry
    assert len({int(v) >> 40 for v in vals}) >= 5                               # the leading key digits differ among candidates
    assert set(r["stages"][0][2][r["stages"][0][2] > 0].tolist()) == {254}      # every corner of a saturated image scores 254
    assert max(C.SATURATED_QUOTAS) > 22 and 22 in C.SATURATED_QUOTAS and 2 in C.SATURATED_QUOTAS
    assert (R == R.max()).sum() == 4                                            # quota 2 cuts inside the leading tie


# ------------------------------------------------------------------------------------------------------------ 4: value range
def test_thresholds_1_and_254():
    img = C.threshold_noise()
    assert len(C.reference(img, params(img, n_features=1000, n_levels=1, fast_threshold=1))["x"]) == 179
    assert len(C.reference(img, params(img, n_features=1000, n_levels=1, fast_threshold=254))["x"]) == 0
    img = C.threshold_dots()
    lo = C.reference(img, params(img, n_features=1000, n_levels=1, fast_threshold=1))
    assert C.xy(lo) == [(50, 20), (30, 30), (40, 40)] and lo["response"].tolist() == [C.R_255, C.R_255, C.dot_R(254)]
    assert int((lo["stages"][0][2] > 0).sum()) == 3                             # at t = 1 nothing else in a dot image is a corner
    hi = C.reference(img, params(img, n_features=1000, n_levels=1, fast_threshold=254))
    assert C.xy(hi) == [(50, 20), (30, 30)] and int(hi["stages"][0][2][40, 40]) == 0 and C.dot_score(254) == 253
    assert lo["bin"].tolist() == [0, 4, 20] == [C.bin_of_direction(*C.dot_moment(C.THRESHOLD_DOTS, i)) for i in (1, 0, 2)]
    img = C.inverse_dots()
    inv = C.reference(img, params(img, n_features=1000, n_levels=1, fast_threshold=254))
    assert C.xy(inv) == [(50, 20), (30, 30)] and inv["bin"].tolist() == [0, 0] and inv["response"].tolist() == [C.R_255] * 2
    assert int(img.min()) == 0 and int(img.max()) == 255 and int((img == 0).sum()) == 2       # p + t = 254: the brighter arc


def test_moments_on_axes_and_diagonals():
    imgs = C.axis_batch()
    assert C.AXIS_BINS == [0, 4, 8, 12, 16, 20, 24, 28]
    for k, img in enumerate(imgs):
        r = C.reference(img, params(img, **C.AXIS_KW))
        m10, m01 = (int(v[0]) for v in ref.moments(img, [32], [32]))
        assert (m10 == 0 or m01 == 0 or abs(m10) == abs(m01)) and (m10, m01) != (0, 0)
        assert C.xy(r) == [(32, 32)] and r["bin"].tolist() == [C.AXIS_BINS[k]] == [C.bin_of_direction(m10, m01)]
        assert r["response"].tolist() == [C.R_255]                              # the patch is outside the Harris window


# --------------------------------------------------------------------------------------------------------------------- 5: mask
def test_checkerboard_mask_and_its_inverse():
    img = C.mask_image()
    P = params(img, **C.MASK_KW)
    m, inv = C.checkerboard(), C.checkerboard_inverse()
    assert set(np.unique(m).tolist()) == {0, 7} and np.array_equal(m != 0, inv == 0) and m[0, 1] == 7 and m[0, 0] == 0
    full, a, b = C.reference(img, P), C.reference(img, P, m), C.reference(img, P, inv)
    assert (P.quota > np.asarray([len(s[3][0]) for s in full["stages"]])).all()
    assert len(full["x"]) == 1051 and len(a["x"]) == 539 and len(b["x"]) == 1051 - 539
    key = lambda r: set(zip(r["level"].tolist(), r["x"].tolist(), r["y"].tolist()))
    assert not (key(a) & key(b)) and key(a) | key(b) == key(full)
    for l in range(P.L):
        assert 0 < C.per_level(a, P.L)[l] < C.per_level(full, P.L)[l]           # every level keeps some and drops some
    for x, y, l in zip(a["x"], a["y"], a["level"]):                             # kept exactly where the level-0 position is allowed
        assert (int(ref.level0_position(x, 112, P.lw[l])) + int(ref.level0_position(y, 96, P.lh[l]))) % 2 == 1


# ------------------------------------------------------------------------------------------------------- 6: state and batch
def test_state_and_batch_cases_have_what_they_need():
    imgs = C.dirty_batch()
    P = params(imgs, **C.DIRTY_KW)
    first = [C.reference(i, P) for i in imgs]
    assert all(0 < len(r["x"]) < P.n_max for r in first)                        # used and unused slots in both images
    dense, const = (C.reference(i, P) for i in C.dense_and_constant())
    assert len(dense["x"]) > len(first[0]["x"]) and len(const["x"]) == 0
    assert all(len(s[3][0]) == 0 for s in const["stages"])
    batch = C.big_batch()
    Pb = params(batch, **C.BIG_BATCH_KW)
    counts = [len(C.reference(i, Pb)["x"]) for i in batch]
    assert len(batch) == 70 > 64 and 10 <= min(counts) and max(counts) <= 20
