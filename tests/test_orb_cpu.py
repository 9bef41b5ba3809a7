"""CPU: the ORB specification of DESIGN.md 4d as restated in tests/orb_ref.py, against hand-derived truths (no self-comparison),
plus the host-side pieces of slamhip.orb (quotas, tables, validation) that need no GPU."""
import numpy as np
import pytest

import orb_ref as ref
from slamhip import orb


def ring_image(positions, centre=100, ring=150, size=40):
    img = np.full((size, size), centre, np.uint8)
    for i in positions:
        dx, dy = ref.RING[i % 16]
        img[20 + dy, 20 + dx] = ring
    return img


def test_segment_test_hand_cases():
    nine = ring_image(range(3, 12))
    s = ref.fast_scores(nine, 20)
    assert s[20, 20] == 49                                   # 150 > 100 + t'  <=>  t' <= 49
    assert ref.fast_scores(nine, 49)[20, 20] == 49 and ref.fast_scores(nine, 50)[20, 20] == 0
    assert ref.fast_scores(ring_image(range(3, 11)), 20)[20, 20] == 0        # 8 contiguous: not a corner
    wrap = ring_image(list(range(12, 16)) + list(range(0, 5)))              # positions 12..4 through the wrap: 9 contiguous
    assert ref.fast_scores(wrap, 20)[20, 20] == 49
    dark = ring_image(range(3, 12), centre=150, ring=100)
    assert ref.fast_scores(dark, 20)[20, 20] == 49
    assert ref.fast_scores(ring_image(range(3, 11), centre=150, ring=100), 20)[20, 20] == 0
    mixed = ring_image(range(0, 9), ring=150)
    mixed[20 + ref.RING[4][1], 20 + ref.RING[4][0]] = 130                   # the weakest pixel of the arc sets the score
    assert ref.fast_scores(mixed, 20)[20, 20] == 29


def test_scores_stay_out_of_the_border_and_small_levels_yield_nothing():
    img = ref.noise(50, 60, 1)
    s = ref.fast_scores(img, 5)
    assert s[16:-16, 16:-16].any()
    assert not s[:16].any() and not s[-16:].any() and not s[:, :16].any() and not s[:, -16:].any()
    assert not ref.fast_scores(ref.noise(32, 200, 1), 5).any() and not ref.fast_scores(ref.noise(200, 32, 1), 5).any()
    assert ref.fast_scores(ref.noise(33, 33, 1), 1).shape == (33, 33)


def test_nms_drops_equal_neighbours():
    s = np.zeros((9, 9), np.uint8)
    s[4, 4] = s[4, 5] = 30
    s[1, 1] = 12
    s[7, 6], s[7, 7] = 40, 41
    keep = ref.nms(s)
    assert not keep[4, 4] and not keep[4, 5]                 # two equal adjacent scores: both dropped
    assert keep[1, 1] and keep[7, 7] and not keep[7, 6]
    assert keep.sum() == 2


def test_harris_equals_big_integer_arithmetic():
    img = ref.noise(40, 40, 7)
    for (y, x) in ((20, 20), (17, 22), (22, 16)):
        a = b = c = 0
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                p = lambda j, i: int(img[y + dy + j, x + dx + i])
                ix = (p(-1, 1) + 2 * p(0, 1) + p(1, 1)) - (p(-1, -1) + 2 * p(0, -1) + p(1, -1))
                iy = (p(1, -1) + 2 * p(1, 0) + p(1, 1)) - (p(-1, -1) + 2 * p(-1, 0) + p(-1, 1))
                a, b, c = a + ix * ix, b + ix * iy, c + iy * iy
        assert int(ref.harris(img, [y], [x])[0]) == 25 * (a * c - b * b) - (a + c) ** 2
    worst = np.zeros((40, 40), np.uint8)                     # the largest gradients an image can have stay inside int64
    worst[:, 20:] = 255
    a = 49 * 1020 ** 2
    assert int(ref.harris(worst, [20], [20])[0]) < 0 and abs(25 * a * a) < 2 ** 63


def test_orientation_bins():
    half = np.zeros((41, 41), np.uint8)
    half[:, 21:] = 200                                       # bright on the +x side: the centroid points along +x
    for k, want in enumerate((0, 8, 16, 24)):
        img = np.rot90(half, -k)                             # (x, y) -> (-y, x) per step, y down
        m10, m01 = ref.moments(img, [20], [20])
        assert int(ref.orientation_bin(m10, m01)[0]) == want
    d = ref.angle_boundaries()
    assert d[:8].tolist() == [[16305, 1606], [15679, 4756], [14449, 7723], [12665, 10394], [10394, 12665], [7723, 14449], [4756, 15679],
                              [1606, 16305]]
    for k in range(32):
        assert int(ref.orientation_bin(d[k, 0], d[k, 1])[0]) == (k + 1) % 32         # exactly on a boundary: the upper interval
        assert int(ref.orientation_bin(7 * d[k, 0], 7 * d[k, 1])[0]) == (k + 1) % 32
        c = d[k] + d[(k + 1) % 32]                            # between boundaries k and k+1: bin k+1
        assert int(ref.orientation_bin(c[0], c[1])[0]) == (k + 1) % 32
    assert int(ref.orientation_bin(0, 0)[0]) == 0
    assert int(ref.orientation_bin(1000, 0)[0]) == 0 and int(ref.orientation_bin(0, 1000)[0]) == 8
    assert int(ref.orientation_bin(-1000, 0)[0]) == 16 and int(ref.orientation_bin(0, -1000)[0]) == 24


def test_quarter_turn_equivariance_is_exact():
    n = 112
    img = ref.scene(n, n, 7, shapes=120)
    table = orb.steered_table()
    lh, lw = ref.level_sizes(n, n, 1)
    a = ref.extract(img, lh, lw, [10 ** 6], 20, table)
    b = ref.extract(np.rot90(img, -1).copy(), lh, lw, [10 ** 6], 20, table)
    assert len(a["x"]) > 20 and len(a["x"]) == len(b["x"])
    key = lambda r, xs, ys, bins: sorted(zip(xs.tolist(), ys.tolist(), bins.tolist(), r["response"].tolist(), map(bytes, r["descriptors"])))
    mapped = key(a, n - 1 - a["y"], a["x"], (a["bin"] + 8) % 32)              # (x, y) -> (n - 1 - y, x)
    assert mapped == key(b, b["x"], b["y"], b["bin"])


def test_quotas_order_and_no_top_up():
    for n, L in ((500, 8), (200, 8), (2000, 8), (1000, 4), (7, 3), (0, 8), (123, 1)):
        q = orb.level_quotas(n, L)
        assert q.sum() == n and len(q) == L and (q >= 0).all()
        assert np.array_equal(q, ref.quotas(n, L))
    assert orb.level_quotas(500, 8).tolist() == [109, 90, 75, 63, 52, 44, 36, 31]
    assert orb.level_sizes(480, 752)[1].tolist() == [752, 627, 522, 435, 363, 302, 252, 210]
    img = ref.scene(120, 160, 2, shapes=60)
    P = orb.OrbParams(120, 160, n_features=100)
    r = ref.extract(img, P.lh, P.lw, P.quota, 20, P.table)
    avail = [len(s[3][0]) for s in r["stages"]]
    got = np.bincount(r["level"], minlength=P.L)
    assert got.tolist() == [min(a, q) for a, q in zip(avail, P.quota)]
    assert any(a < q for a, q in zip(avail, P.quota)) and any(a > q for a, q in zip(avail, P.quota))   # short levels are not topped up
    assert (np.diff(r["level"]) >= 0).all()
    for l in range(P.L):
        sel = r["level"] == l
        rows = list(zip((-r["response"][sel]).tolist(), r["y"][sel].tolist(), r["x"][sel].tolist()))
        assert rows == sorted(rows)
        R, ys, xs = r["stages"][l][3]                        # and they are the best ones
        if len(R) > P.quota[l]:
            assert min(r["response"][sel]) >= np.sort(R)[::-1][P.quota[l] - 1]


def test_mask():
    img = ref.scene(120, 160, 2, shapes=60)
    P = orb.OrbParams(120, 160, n_features=300, n_levels=4)
    assert len(ref.extract(img, P.lh, P.lw, P.quota, 20, P.table, mask0=np.zeros((120, 160), np.uint8))["x"]) == 0
    m = np.zeros((120, 160), np.uint8)
    m[30:90, 40:130] = 255
    r = ref.extract(img, P.lh, P.lw, P.quota, 20, P.table, mask0=m)
    full = ref.extract(img, P.lh, P.lw, P.quota, 20, P.table)
    assert 0 < len(r["x"]) < len(full["x"]) and (r["level"] > 0).any()
    for x, y, l in zip(r["x"], r["y"], r["level"]):
        x0, y0 = ref.level0_position(x, 160, P.lw[l]), ref.level0_position(y, 120, P.lh[l])
        assert 40 <= x0 < 130 and 30 <= y0 < 90
    assert int(ref.level0_position(5, 100, 10)) == 50 and int(ref.level0_position(9, 95, 10)) == 86 and int(ref.level0_position(9, 91, 10)) == 82


def test_resample_and_blur_hand_cases():
    img = ref.noise(37, 53, 2)
    assert np.array_equal(ref.resample(img, 37, 53), img)                    # level 0 maps to itself
    flat = np.full((20, 30), 77, np.uint8)
    assert (ref.resample(flat, 17, 25) == 77).all() and (ref.blur(flat) == 77).all()
    two = np.zeros((4, 8), np.uint8)
    two[:, 4:] = 200
    half = ref.resample(two, 2, 4)                           # centres at 0.5, 2.5, 4.5, 6.5: each the mean of two equal pixels
    assert half.tolist() == [[0, 0, 200, 200]] * 2
    spike = np.zeros((15, 15), np.uint8)
    spike[7, 7] = 255
    want = np.outer(ref.BLUR_TAPS, ref.BLUR_TAPS) * 255
    assert np.array_equal(ref.blur(spike)[4:11, 4:11], (want + 2048) >> 12)
    assert np.array_equal(ref.blur(spike.T), ref.blur(spike).T)              # one rounding: the two passes commute
    r = ref.noise(21, 22, 9)
    assert np.array_equal(ref.blur(np.rot90(r, -1)), np.rot90(ref.blur(r), -1))


def test_pattern_tables():
    p = orb.DEFAULT_PATTERN
    assert p.shape == (256, 4) and p.dtype == np.int8
    q = p.astype(int)
    assert (q[:, 0] ** 2 + q[:, 1] ** 2 <= 225).all() and (q[:, 2] ** 2 + q[:, 3] ** 2 <= 225).all()
    assert p[:2].tolist() == [[-2, 2, 4, -6], [7, -6, 11, 7]]                # the committed numbers
    t = orb.steered_table().astype(int)
    assert t.shape == (32, 256, 4) and np.abs(t).max() <= 15 and np.array_equal(t[0], q)
    assert np.array_equal(t, ref.steered_table(p).astype(int))
    for b in range(32):                                      # 4-fold symmetry, also through the wrap 31 -> 7
        nxt = t[(b + 8) % 32]
        assert np.array_equal(nxt[:, 0], -t[b][:, 1]) and np.array_equal(nxt[:, 1], t[b][:, 0])
        assert np.array_equal(nxt[:, 2], -t[b][:, 3]) and np.array_equal(nxt[:, 3], t[b][:, 2])
    far = np.zeros((256, 4), np.int8)
    far[:, 0], far[:, 1] = 15, 0                             # radius exactly 15 at every angle stays within [-15, 15]
    assert np.abs(orb.steered_table(far).astype(int)).max() == 15


def test_descriptor_bit_order():
    img = np.zeros((40, 40), np.uint8)
    img[20, 25] = 9                                          # only b of test 0 and a of test 9 are bright
    pat = np.zeros((1, 256, 4), np.int8)
    pat[0, :, 0] = 1                                         # every other test compares two dark pixels: bit 0
    pat[0, 0] = (0, 1, 5, 0)
    pat[0, 9] = (5, 0, 0, 1)
    pat[0, 10] = (1, 0, 5, 0)
    d = ref.describe(img, [20], [20], [0], pat)[0]
    assert d[0] == 1 and d[1] == 4 and not d[2:].any()       # test 0 -> bit 0 of byte 0; test 10 -> bit 2 of byte 1; test 9 is a > b


def test_binding_validation_errors():
    img = np.zeros((64, 64), np.uint8)
    bad = [dict(images=img.astype(np.float32)), dict(images=np.zeros((2, 2, 64, 64), np.uint8)), dict(images=np.zeros(64, np.uint8)),
           dict(images=img, mask=np.ones((64, 63), np.uint8)), dict(images=img[None], mask=np.ones((2, 64, 64), np.uint8)),
           dict(images=img, mask=np.ones((64, 64), np.float32)), dict(images=img, n_levels=0), dict(images=img, n_levels=17),
           dict(images=img, fast_threshold=0), dict(images=img, fast_threshold=255), dict(images=img, n_features=-1),
           dict(images=img, n_features=1 << 20), dict(images=img, scale=1.0), dict(images=img, pattern=np.zeros((255, 4), np.int8)),
           dict(images=img, pattern=np.zeros((256, 4), np.float32)), dict(images=np.zeros((0, 64), np.uint8))]
    far = np.zeros((256, 4), np.int8)
    far[17] = (0, 0, 12, 10)                                 # 144 + 100 > 225
    bad.append(dict(images=img, pattern=far))
    for kw in bad:
        with pytest.raises(ValueError):
            orb.orb_extract_arrays(**kw)
    ok = np.zeros((256, 4), np.int8)
    ok[:, 2:] = (9, 12)                                      # norm exactly 15 is allowed
    assert orb.check_pattern(ok).dtype == np.int8
    empty = orb.orb_extract_arrays(np.zeros((0, 64, 64), np.uint8))          # B = 0: no device needed, no error
    assert len(empty) == 0
    with pytest.raises(ValueError):
        orb.to_gray(np.zeros((4, 4, 2), np.uint8))
    rgb = np.zeros((2, 2, 3), np.uint8)
    rgb[0, 0], rgb[0, 1], rgb[1, 0], rgb[1, 1] = (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255)
    assert orb.to_gray(rgb).tolist() == [[255, 77], [149, 29]]     # (150 * 255 + 128) >> 8 = 38378 >> 8 = 149


def test_detector_signatures_mirror_the_reference():
    import inspect

    d = orb.OrbFeatureDetector
    assert list(inspect.signature(d.__init__).parameters) == ["self", "n_features"]
    assert inspect.signature(d.__init__).parameters["n_features"].default == 500
    for name in ("detect", "detect_and_compute"):
        sig = inspect.signature(getattr(d, name))
        assert list(sig.parameters) == ["self", "img", "mask"] and sig.parameters["mask"].default is None
    k = orb.KeyPoint(1.5, 2.5, 31.0, 45.0, 7.0, 2)
    assert (k.pt, k.size, k.angle, k.response, k.octave) == ((1.5, 2.5), 31.0, 45.0, 7.0, 2)
    with pytest.raises(AttributeError):
        k.other = 1


def test_workspace_query_needs_no_device_and_refuses_bad_shapes(built):
    import ctypes

    import slamhip

    lib = slamhip.load()
    P = orb.OrbParams(83, 97)
    nbytes, lay = P.workspace(3)
    assert nbytes > 3 * lay["image_stride"] and (lay["pitch"] % 4 == 0).all() and (lay["pitch"] >= P.lw).all()
    assert lay["capacity"].tolist() == [((w - 31) // 2) * ((h - 31) // 2) if w >= 33 and h >= 33 else 0 for w, h in zip(P.lw, P.lh)]
    ends = lay["candidates"] + 16 * lay["capacity"]
    assert (np.diff(np.r_[lay["image"], ends[-1]]) > 0).all() and ends[-1] <= lay["image_stride"]
    n = ctypes.c_uint64(0)
    call = lambda B, H, W, L, lw, lh, nmax: lib.slam_orb_workspace(B, H, W, L, lw.ctypes.data, lh.ctypes.data, nmax, ctypes.byref(n), None)
    assert call(1, 83, 97, 8, P.lw, P.lh, 500) == 0
    assert call(0, 83, 97, 8, P.lw, P.lh, 500) == 0                          # B = 0 is not an error
    for args in ((-1, 83, 97, 8, P.lw, P.lh, 500), (1, 83, 97, 0, P.lw, P.lh, 500), (1, 83, 97, 17, P.lw, P.lh, 500),
                 (1, 84, 97, 8, P.lw, P.lh, 500), (1, 83, 97, 8, P.lw, P.lh, (1 << 16) + 1), (1, 83, 9000, 8, P.lw, P.lh, 500),
                 (1, 83, 97, 8, P.lw[::-1].copy(), P.lh, 500), (70000, 83, 97, 8, P.lw, P.lh, 500)):
        assert call(*args) == -1, args
    assert lib.slam_orb_workspace(1, 83, 97, 8, None, P.lh.ctypes.data, 500, ctypes.byref(n), None) == -1
    assert b"null level size" in lib.slam_last_error()
