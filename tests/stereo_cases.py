"""Scenes for the stereo matching tests: random blocks (their own keypoint tables and pyramid planes), hand cases whose answers
are known without running anything, and the shifted texture of the extractor chain."""
from __future__ import annotations

import numpy as np

import stereo_ref as ref

SIZES3 = ((96, 64), (80, 53), (67, 44))          # (w, h) of the three levels of the random blocks; the smallest test uses 48 x 40
SCALE3 = ref.scale_table(1.2, 3)
PARAMS3 = dict(bf=40.0, min_d=0.0, max_d=7.0, th_orb=75, w=5, Ls=5, reject=True)

# The extractor chain: a smoothed random texture T of 120 x (160 + d); left = T[:, :160], right = T[:, d:d + 160].
CHAIN_SEED = 20261021
CHAIN_H, CHAIN_W = 120, 160
CHAIN_FEATURES = 300
CHAIN_BF, CHAIN_MAX_D = 47.9, 40.0
# Status-0 rows with a best SAD of 0 that the statement yields on the CPU for the committed seed at n_levels = 1 and reject = 0,
# with the keypoints of tests/orb_ref.py (tests/test_stereo_cpu.py checks these two numbers), and the floor the GPU test holds the
# device to: half.  With the rejection on, the median of these scenes is 0 - the true inc costs nothing - and 10 SAD < 21 * 0
# holds for no row: every row is rejected, as ORB-SLAM's float form rejects them.  The truth test therefore runs without it.
CHAIN_MEASURED = {3: 292, 17: 261}
CHAIN_FLOOR = {d: n // 2 for d, n in CHAIN_MEASURED.items()}


def texture(rng, h, w, k=3):
    """A box-smoothed random field stretched to u8: enough contrast for FAST, smooth enough for a SAD minimum to be a basin."""
    f = rng.uniform(0.0, 1.0, (h + 2 * k, w + 2 * k))
    c = np.cumsum(np.cumsum(np.pad(f, ((1, 0), (1, 0))), 0), 1)
    n = 2 * k + 1
    s = c[n:, n:] - c[:-n, n:] - c[n:, :-n] + c[:-n, :-n]
    s = (s - s.min()) / (s.max() - s.min())
    return np.clip(np.rint(255.0 * s), 0, 255).astype(np.uint8)


def chain_images(d, seed=CHAIN_SEED):
    T = texture(np.random.default_rng(seed), CHAIN_H, CHAIN_W + d, 2)
    return np.ascontiguousarray(T[:, :CHAIN_W]), np.ascontiguousarray(T[:, d:d + CHAIN_W])


def chain_cpu(d, n_levels, seed=CHAIN_SEED):
    """The chain without a device: tests/orb_ref.py (the extractor's numpy statement) on both images -> a block of two images
    (0 = left, 1 = right) and the scale table."""
    import orb_ref
    from slamhip.orb import OrbParams

    P = OrbParams(CHAIN_H, CHAIN_W, CHAIN_FEATURES, n_levels, 1.2, 20)
    blk = dict(count=np.zeros(2, np.int32), kp=np.zeros((2, P.n_max, 4), np.int32), desc=np.zeros((2, P.n_max, 32), np.uint8), planes=[])
    for b, img in enumerate(chain_images(d, seed)):
        r = orb_ref.extract(img, P.lh, P.lw, P.quota, P.t, P.table)
        n = len(r["x"])
        blk["count"][b] = n
        blk["kp"][b, :n] = np.stack([r["x"], r["y"], r["level"], r["bin"]], 1)
        blk["desc"][b, :n] = r["descriptors"]
        blk["planes"].append([st[0] for st in r["stages"]])
    return blk, ref.scale_table(1.2, n_levels)


def chain_truth(out, d):
    """(rows of status 0 with a best SAD of 0, the largest |disp - d| among them) of pair 0 of a chain result; disp = uL - u_right
    needs the left pixels, which the caller passes as out["uL"]."""
    ok = (out["status"][0] == ref.MATCHED) & (out["sad"][0] == 0)
    err = np.abs((out["uL"][ok] - out["u_right"][0][ok]) - d)
    return int(ok.sum()), float(err.max()) if ok.any() else 0.0


def flip(rng, desc, n):
    """`desc` u8 [32] with `n` distinct bits flipped."""
    bits = np.unpackbits(desc)
    bits[rng.choice(256, n, replace=False)] ^= 1
    return np.packbits(bits)


def random_image_pair(rng, nL, nR, n_max, sizes=SIZES3, shifts=(6, 6, 4)):
    """One left and one right image: planes (right = left shifted by shifts[l] columns on level l, its lower third noisy),
    left rows anywhere in their level, right rows partly twins of left rows (moved by the shift and a jitter, some bits of the
    descriptor flipped), partly random.  Rows past the counts hold rows that look valid: nobody may read them."""
    planesL, planesR = [], []
    for (w, h), s in zip(sizes, shifts):
        T = texture(rng, h, w + s + 8)
        R = np.clip(T[:, s:s + w].astype(np.int64) + rng.integers(-2, 3, (h, w)), 0, 255).astype(np.uint8)
        noisy = slice(2 * h // 3, h)
        R[noisy] = np.clip(R[noisy].astype(np.int64) + rng.integers(-40, 41, R[noisy].shape), 0, 255).astype(np.uint8)
        planesL.append(np.ascontiguousarray(T[:, :w]))
        planesR.append(R)
    L = len(sizes)

    def rows(n):
        lev = rng.integers(0, L, n)
        wh = np.asarray(sizes)[lev]
        kp = np.stack([rng.integers(0, wh[:, 0]), rng.integers(0, wh[:, 1]), lev, rng.integers(0, 32, n)], 1).astype(np.int32)
        return kp, rng.integers(0, 256, (n, 32), dtype=np.uint8)

    kpL, descL = rows(n_max)
    kpR, descR = rows(n_max)
    for j in range(min(nR, nL) * 3 // 4):
        i = int(rng.integers(0, nL))
        x, y, l, _ = kpL[i]
        jx = int(rng.choice([-1, 0, 0, 0, 0, 1, 2, 5]))
        xr = int(np.clip(x - shifts[l] + jx, 0, sizes[l][0] - 1))
        yr = int(np.clip(y + rng.integers(-2, 3), 0, sizes[l][1] - 1))
        kpR[j] = (xr, yr, l, 0)
        descR[j] = flip(rng, descL[i], int(rng.choice([0, 3, 10, 30, 60, 74, 75, 90])))
    return planesL, planesR, kpL, descL, kpR, descR


def random_blocks(seed, counts_left, counts_right, n_max, sizes=SIZES3, shifts=(6, 6, 4)):
    """(left block, right block) of len(counts) images each; image b of the left block belongs with image b of the right."""
    rng = np.random.default_rng(seed)
    B = len(counts_left)
    left = dict(count=np.asarray(counts_left, np.int32), kp=np.zeros((B, n_max, 4), np.int32), desc=np.zeros((B, n_max, 32), np.uint8), planes=[])
    right = dict(count=np.asarray(counts_right, np.int32), kp=np.zeros((B, n_max, 4), np.int32), desc=np.zeros((B, n_max, 32), np.uint8), planes=[])
    for b in range(B):
        pL, pR, kL, dL, kR, dR = random_image_pair(rng, int(counts_left[b]), int(counts_right[b]), n_max, sizes, shifts)
        left["kp"][b], left["desc"][b], right["kp"][b], right["desc"][b] = kL, dL, kR, dR
        left["planes"].append(pL)
        right["planes"].append(pR)
    return left, right


def joined(left, right):
    """One block of 2B images: the left images, then the right ones (the same block passed as left and right)."""
    return dict(count=np.concatenate([left["count"], right["count"]]), kp=np.concatenate([left["kp"], right["kp"]]),
                desc=np.concatenate([left["desc"], right["desc"]]), planes=left["planes"] + right["planes"])


def block_of(kp, desc, planes, n_max=None):
    """A block of one image from its rows."""
    kp, desc = np.asarray(kp, np.int32).reshape(-1, 4), np.asarray(desc, np.uint8).reshape(-1, 32)
    n = len(kp)
    n_max = n if n_max is None else n_max
    blk = dict(count=np.asarray([n], np.int32), kp=np.zeros((1, n_max, 4), np.int32), desc=np.zeros((1, n_max, 32), np.uint8), planes=[list(planes)])
    blk["kp"][0, :n], blk["desc"][0, :n] = kp, desc
    return blk


# ---- hand cases ---------------------------------------------------------------------------------------------------------------
# Each is (name, scene, params, expect): scene = (kpL, descL, planesL, kpR, descR, planesR, scale); expect maps an output to the
# values of its first rows, written down from the specification.  NAN stands for "NaN here".
NAN = float("nan")
ONE = np.zeros(32, np.uint8)                      # every row of a hand case carries this descriptor unless it says otherwise


def _kp(rows):
    return np.asarray([(x, y, l, 0) for x, y, l in rows], np.int32).reshape(-1, 4)


def _flat(sizes, v=90):
    return [np.full((h, w), v, np.uint8) for w, h in sizes]


def _search_case(name, left, right, scale, expect_right, descR=None, **kw):
    """A case that stops at step 2 (th_orb = 0: every distance is >= it): `right` says which row the search took."""
    sizes = [(64, 64)] * len(scale)
    prm = dict(bf=1.0, min_d=0.0, max_d=1000.0, th_orb=0, w=5, Ls=5, reject=True)
    prm.update(kw)
    kL, kR = _kp(left), _kp(right)
    dR = np.tile(ONE, (len(kR), 1)) if descR is None else np.asarray(descR, np.uint8)
    exp_r = np.asarray(expect_right, np.int32)
    return (name, (kL, np.tile(ONE, (len(kL), 1)), _flat(sizes), kR, dR, _flat(sizes), np.asarray(scale, np.float32)), prm,
            dict(right=exp_r, status=np.where(exp_r < 0, ref.NO_CANDIDATE, ref.ORB_DISTANCE).astype(np.uint8),
                 sad=np.full(len(kL), -1, np.int32)))


def stripes(h, w, cols, rows=None, value=100, extra=()):
    """A plane of zeros with vertical stripes of `value` at `cols` (on `rows`, a slice; default all) and single pixels
    extra = ((y, x, v), ...)."""
    p = np.zeros((h, w), np.uint8)
    for c in cols:
        p[rows if rows is not None else slice(None), c] = value
    for y, x, v in extra:
        p[y, x] = v
    return p


def _sad_case(name, left_xy, right_xy, IL, IR, expect, **kw):
    """One level of scale 1; left and right rows at level 0 with the descriptor ONE."""
    prm = dict(bf=10.0, min_d=0.0, max_d=30.0, th_orb=75, w=1, Ls=5, reject=False)
    prm.update(kw)
    kL, kR = _kp([(x, y, 0) for x, y in left_xy]), _kp([(x, y, 0) for x, y in right_xy])
    return (name, (kL, np.tile(ONE, (len(kL), 1)), [IL], kR, np.tile(ONE, (len(kR), 1)), [IR], np.ones(1, np.float32)), prm, expect)


def _median_case(name, sads, expect_status, reject=True):
    """Rows on image rows 3, 7, 11, ...: a stripe at column 30 on the left and at 24 on the right (disparity 6, found at
    inc = 0 from a right keypoint at 24), and the right stripe's pixel above the centre, (y - 1, 24), lowered to 100 - k:
    A(-1, 0) = 0 and Q(-1, 0) = -k, so the best SAD is k; the two neighbours of inc = 0 cost the same (the change is on the
    axis of symmetry), so delta = 0 and u_right = 24."""
    n = len(sads)
    ys = [3 + 4 * i for i in range(n)]
    H = 4 * n + 4
    IL = stripes(H, 64, [30])
    IR = stripes(H, 64, [24], extra=[(y - 1, 24, 100 - k) for y, k in zip(ys, sads)])
    st = np.asarray(expect_status, np.uint8)
    ok = st == 0
    return _sad_case(name, [(30, y) for y in ys], [(24, y) for y in ys], IL, IR,
                     dict(status=st, sad=np.asarray(sads, np.int32), right=np.arange(n, dtype=np.int32),
                          u_right=np.where(ok, 24.0, NAN), depth=np.where(ok, 10.0 / 6.0, NAN),
                          counts=np.asarray([ok.sum(), n], np.int32)), reject=reject)


def hand_cases():
    S12 = ref.scale_table(1.2, 3)
    S2 = ref.scale_table(2.0, 5)
    cases = []
    # level 1 of scale 1.2f: a right row at y = 10 has vR = 12.0000005, r = 2.4000001: the band is [floor(9.6), ceil(14.4)] =
    # [9, 15].  Left rows at level 1 with y = 7, 8, 12, 13, 14 have trunc(vL) = 8, 9, 14, 15, 16: out, in (at the floor), in,
    # in (at the ceil), out.
    cases.append(_search_case("band_floor_and_ceil", [(20, y, 1) for y in (7, 8, 12, 13, 14)], [(10, 10, 1)], S12, [-1, 0, 0, 0, -1]))
    # scale 1 at level 0: r = 2, the band of a right row at y = 10 is [8, 12] exactly
    cases.append(_search_case("band_integer_edges", [(20, y, 0) for y in (7, 8, 12, 13)], [(10, 10, 0)], S2, [-1, 0, 0, -1]))
    # left at level 2 (scale 4, y = 5: trunc(vL) = 20); right rows at levels 0..4 placed on vR = 20: levels 1, 2, 3 are in and
    # the lowest row of them wins (all distances are 0); with only levels 0 and 4 on offer there is no candidate
    cases.append(_search_case("level_gate_in", [(15, 5, 2)], [(3, 20, 0), (3, 10, 1), (3, 5, 2), (0, 3, 3), (0, 1, 4)], S2, [1]))
    cases.append(_search_case("level_gate_out", [(15, 5, 2)], [(3, 20, 0), (0, 1, 4)], S2, [-1]))
    cases.append(_search_case("level_gate_plus_one", [(15, 5, 2)], [(3, 20, 0), (0, 3, 3), (0, 1, 4)], S2, [1]))
    # uL = 40, min_d = 3, max_d = 10: uR must lie in [30, 37]; rows at 29, 38 are out, 30 and 37 are in
    for name, xs, want in (("disparity_low_bound_in", [29, 30], [1]), ("disparity_high_bound_in", [38, 37], [1]),
                           ("disparity_bounds_out", [29, 38], [-1])):
        cases.append(_search_case(name, [(40, 10, 0)], [(x, 10, 0) for x in xs], S2, want, min_d=3.0, max_d=10.0))
    # uL - min_d = 2 - 3 < 0: no candidates, whatever the right image holds
    cases.append(_search_case("left_of_min_d", [(2, 10, 0)], [(0, 10, 0), (2, 10, 0)], S2, [-1], min_d=3.0, max_d=10.0))
    # duplicate right descriptors: rows 1 and 2 are equal and nearest, the lower one wins; row 0 is further
    far = ONE.copy()
    far[0] = 0xFF
    cases.append(_search_case("duplicate_descriptors", [(40, 10, 0)], [(30, 10, 0), (31, 10, 0), (32, 10, 0)], S2, [1], descR=[far, ONE, ONE]))

    # ---- SAD: one level of scale 1, w = 1, Ls = 5.  A left stripe (100 on 0) at column 30; A(dy, dx) = -100 off the stripe.
    IL = stripes(12, 64, [30])
    # the right stripe at 22 seen from a right keypoint at 24: SAD(-2) = 0 and SAD(-3) = SAD(-1) = 900 (three pixels of 100 and
    # three of 200): delta = 0, u_right = 22, disp = 8
    cases.append(_sad_case("symmetric_profile", [(30, 5)], [(24, 5)], IL, stripes(12, 64, [22]),
                           dict(status=[0], sad=[0], u_right=[22.0], depth=[10.0 / 8.0], right=[0], counts=[1, 1])))
    # a flat pair of images: every SAD is 0, the lowest inc is -Ls: slide border.  (With the lowest inc winning ties, d1 > d2
    # whenever the best is interior, so den > 0 there: den = 0 is reachable only through st_parabola itself.)
    flat = np.full((12, 64), 77, np.uint8)
    cases.append(_sad_case("flat_patch", [(30, 5)], [(24, 5)], flat, flat, dict(status=[4], sad=[0], u_right=[NAN], depth=[NAN], right=[0], counts=[0, 0])))
    cases.append(_sad_case("best_at_minus_Ls", [(30, 5)], [(24, 5)], IL, stripes(12, 64, [19]), dict(status=[4], sad=[0], u_right=[NAN], counts=[0, 0])))
    cases.append(_sad_case("best_at_plus_Ls", [(30, 5)], [(24, 5)], IL, stripes(12, 64, [29]), dict(status=[4], sad=[0], u_right=[NAN], counts=[0, 0])))
    cases.append(_sad_case("best_next_to_the_border", [(30, 5)], [(24, 5)], IL, stripes(12, 64, [28]),
                           dict(status=[0], sad=[0], u_right=[28.0], depth=[10.0 / 2.0], counts=[1, 1])))
    # stripes at 22 and 27: SAD(-2) = SAD(3) = 0, the lower inc wins: u_right = 22
    cases.append(_sad_case("equal_sad_lower_inc_wins", [(30, 5)], [(24, 5)], IL, stripes(12, 64, [22, 27]),
                           dict(status=[0], sad=[0], u_right=[22.0], depth=[10.0 / 8.0], counts=[1, 1])))
    # an asymmetric profile: the right stripe at 23 and one pixel of 40 at (4, 23): SAD(-1) = 60 (|-100 - (40 - 100)| + ... see
    # below), worked out here by hand: at inc = -1 the centre is on the stripe, Q(-1, 0) = 40 - 100 = -60 against A(-1, 0) = 0:
    # SAD = 60.  At inc = -2 (centre 22, stripe at dx = +1): dx = -1: 3 x 100, dx = +1: 2 x 200 + |-100 - 40| = 540: 840.  At
    # inc = 0 (centre 24, stripe at dx = -1): 2 x 200 + 140 + 3 x 100 = 840.  den = 840 + 840 - 120 = 1560, delta = 0.
    cases.append(_sad_case("noisy_symmetric", [(30, 5)], [(24, 5)], IL, stripes(12, 64, [23], extra=[(4, 23, 40)]),
                           dict(status=[0], sad=[60], u_right=[23.0], depth=[10.0 / 7.0], counts=[1, 1])))
    # delta != 0: one extra pixel of 50 at (5, 20) = the background two columns left of the stripe at 22.  inc = -2: SAD 0
    # (the pixel is at dx = -2, outside the patch).  inc = -3 (centre 21 = 0, stripe at dx = +1, pixel at dx = -1, dy = 0):
    # 2 x 100 + |-100 - 50| + 3 x 200 = 950.  inc = -1 (centre 23, stripe at dx = -1): 900.  delta = (950 - 900) / (2 x 1850).
    d = 50.0 / 3700.0
    cases.append(_sad_case("parabola_offset", [(30, 5)], [(24, 5)], IL, stripes(12, 64, [22], extra=[(5, 20, 50)]),
                           dict(status=[0], sad=[0], u_right=[22.0 + d], depth=[10.0 / (30.0 - (22.0 + d))], counts=[1, 1])))
    # the column test, w = 1, Ls = 5: c0 = 5 gives c0 - Ls - w = -1 (window), c0 = 6 gives 0 (goes on: stripe at 6, inc = 0)
    cases.append(_sad_case("window_left_minus_one", [(12, 5)], [(5, 5)], stripes(12, 64, [12]), stripes(12, 64, [5]),
                           dict(status=[3], sad=[-1], right=[0], u_right=[NAN], counts=[0, 0])))
    cases.append(_sad_case("window_left_zero", [(12, 5)], [(6, 5)], stripes(12, 64, [12]), stripes(12, 64, [6]),
                           dict(status=[0], sad=[0], u_right=[6.0], depth=[10.0 / 6.0], counts=[1, 1])))
    # level_w = 64: c0 = 57 gives c0 + Ls + w + 1 = 64 = level_w (window); c0 = 56 gives level_w - 1 (goes on)
    cases.append(_sad_case("window_right_level_w", [(60, 5)], [(57, 5)], stripes(12, 64, [60]), stripes(12, 64, [57]),
                           dict(status=[3], sad=[-1], u_right=[NAN], counts=[0, 0])))
    cases.append(_sad_case("window_right_level_w_minus_one", [(60, 5)], [(56, 5)], stripes(12, 64, [60]), stripes(12, 64, [56]),
                           dict(status=[0], sad=[0], u_right=[56.0], depth=[10.0 / 4.0], counts=[1, 1])))
    # the rows y +- w and the left patch inside the level (the addition to ORB-SLAM's test): y = 0 and y = 11 of 12 rows, x = 63
    cases.append(_sad_case("window_rows_and_left_patch", [(30, 0), (30, 11), (63, 5)], [(24, 0), (24, 11), (50, 5)], IL, stripes(12, 64, [24]),
                           dict(status=[3, 3, 3], sad=[-1, -1, -1], right=[0, 1, 2], counts=[0, 0])))
    # disp <= 0: both stripes at 30, min_d = -3: disp = 0 becomes 0.01
    cases.append(_sad_case("disparity_zero_becomes_0_01", [(30, 5)], [(31, 5)], IL, stripes(12, 64, [30]),
                           dict(status=[0], sad=[0], u_right=[30.0 - 0.01], depth=[10.0 / 0.01], counts=[1, 1]), min_d=-3.0))
    # disparity out of range after the slide: the keypoint at 24 passes the gate (disp 6 < 7), the stripe at 22 gives 8
    cases.append(_sad_case("disparity_out_of_range", [(30, 5)], [(24, 5)], IL, stripes(12, 64, [22]),
                           dict(status=[5], sad=[0], u_right=[NAN], depth=[NAN], counts=[0, 0]), max_d=7.0))
    # ---- the median: n = 1 (m is the row's own SAD: kept when it is positive), 2, 3, 4
    cases.append(_median_case("median_n1_kept", [7], [0]))
    cases.append(_median_case("median_n1_zero_sad_rejected", [0], [6]))
    cases.append(_median_case("median_n2", [10, 4], [0, 0]))                    # m = 10
    cases.append(_median_case("median_n3", [50, 10, 20], [6, 0, 0]))            # m = 20: 500 >= 420
    cases.append(_median_case("median_n4_equality_rejected", [30, 63, 10, 20], [0, 6, 0, 0]))    # m = 30: 630 = 630
    cases.append(_median_case("median_n4_one_below_kept", [30, 62, 10, 20], [0, 0, 0, 0]))
    cases.append(_median_case("median_off", [50, 10, 20], [0, 0, 0], reject=False))
    return cases


def check_expect(out, expect, name):
    """Every expected entry against the first rows of the output (NaN matches NaN; floats must be equal to the last bit)."""
    for key, want in expect.items():
        got = np.asarray(out[key])
        want = np.asarray(want, got.dtype)
        assert np.array_equal(got[:len(want)], want, equal_nan=got.dtype.kind == "f"), (name, key, got[:len(want)].tolist(), want.tolist())
