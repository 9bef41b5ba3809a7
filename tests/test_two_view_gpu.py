"""Two-view geometry on the GPU (slam_tv_*) against the numpy statement in tests/two_view_ref.py, which takes another route
to the roots (action-matrix eigenvectors against the kernel's degree-10 polynomial) and imports nothing of the product.

Tolerances: where a bound cannot be derived (it depends on the conditioning of random samples) the numpy solver's own worst
value on the same samples is the yardstick and the kernel is allowed 16 x it; the yardsticks were measured on the CPU and are
the constants of tests/test_two_view_cpu.py (asserted there on the numpy solver alone)."""
import os

import numpy as np
import pytest

import two_view_ref as tv
from test_two_view_cpu import CAP, DOUBLE_ROOT, ILL_CONDITIONED, TWIN_WORST_CLEAN, TWIN_WORST_NOISY

pytestmark = pytest.mark.gpu
K = tv.EUROC
FACTOR = 16.0
BAND = 1e-9


def _band_split(E, px1, px2, threshold=1.0):
    d = tv.sampson_sq(E, tv.normalise(px1, K), tv.normalise(px2, K))
    t2 = tv.threshold_sq(threshold, K)
    with np.errstate(invalid="ignore"):
        return d < t2, np.abs(d - t2) <= BAND * t2


# ------------------------------------------------------------------------------------------------ 1. the solver
def test_solver_properties_against_the_numpy_solver(gpu_ctx):
    import slamhip

    for seed, S, noise, worst in ((1, 2000, 0.0, TWIN_WORST_CLEAN), (2, 1000, 0.5, TWIN_WORST_NOISY)):
        x1, x2, Eg = tv.make_samples(seed, S, noise)
        E, n = slamhip.fivepoint_arrays(x1, x2, ctx=gpu_ctx)
        Et, nt, zt = tv.fivepoint(x1, x2)
        assert E.shape == (S, 10, 9) and n.shape == (S,) and n.min() >= 0 and n.max() <= 10
        for s in range(S):
            assert not E[s, n[s]:].any()                               # unused slots are zero
        q, comp = tv.solver_quantities(E, n, x1, x2, Eg if noise == 0 else None)
        qt, compt = tv.solver_quantities(Et, nt, x1, x2, Eg if noise == 0 else None)
        print(f"noise {noise}: kernel {q}\n           numpy  {qt}")
        for k in ("epipolar", "cubic", "det", "frobenius"):
            assert q[k] <= FACTOR * worst[k], (k, q[k], worst[k])
        zz = np.sort(np.where(np.isnan(zt), np.inf, zt), 1)
        with np.errstate(invalid="ignore"):
            gap = np.nanmin(np.where(np.isfinite(zz[:, 1:]), np.diff(zz, axis=1), np.nan), axis=1, initial=np.inf)
        double = gap < DOUBLE_ROOT
        assert double.mean() <= CAP
        mismatch = n != nt
        print(f"           root-count mismatches {int(mismatch.sum())}, numpy double roots {int(double.sum())}")
        assert not (mismatch & ~double).any(), np.flatnonzero(mismatch & ~double)[:10]
        if noise == 0:
            ill = compt > ILL_CONDITIONED
            assert ill.mean() <= CAP
            print(f"           completeness: kernel {comp[~ill].max():.3e} numpy {compt[~ill].max():.3e}")
            assert comp[~ill].max() <= FACTOR * worst["completeness"]


# ------------------------------------------------------------------------------------------------ 2. + 3. scoring and argmax
@pytest.fixture(scope="module")
def scored_scene(gpu_ctx):
    import slamhip

    sc = tv.make_scene(np.random.default_rng(21), 3000, 0.5, 0.3)
    E, mask, st = slamhip.find_essential_offsets(sc["px1"], sc["px2"], [0, 3000], K, 256, 1.0, 7, ctx=gpu_ctx)
    return sc, E[0], mask, st[0]


def test_mask_and_count_are_the_stated_scoring_of_the_returned_matrix(scored_scene):
    sc, E, mask, st = scored_scene
    assert abs(np.linalg.norm(E) - 1) < 1e-14
    want, band = _band_split(E, sc["px1"], sc["px2"])
    print("matches in the 1e-9 band:", int(band.sum()), "inliers", int(mask.sum()), "of", len(mask))
    assert band.mean() <= 0.005
    assert np.array_equal(mask[~band], want[~band])
    assert st[0] == mask.sum()
    assert st[0] >= 0.6 * 0.9 * len(mask)                # 70 % true inliers at 0.5 px noise against a 1 px threshold


def test_winner_is_the_argmax_over_every_root_of_every_reproduced_draw(gpu_ctx, scored_scene):
    import slamhip

    sc, E, mask, st = scored_scene
    x1, x2 = tv.normalise(sc["px1"], K), tv.normalise(sc["px2"], K)
    idx = np.array([tv.draw_sample(7, 0, h, len(x1)) for h in range(256)])
    Es, nr = slamhip.fivepoint_arrays(x1[idx], x2[idx], ctx=gpu_ctx)
    assert st[3] == nr.sum()
    assert np.array_equal(Es[st[1], st[2]], E)           # the solver entry and the RANSAC run the same arithmetic
    t2 = tv.threshold_sq(1.0, K)
    best = None
    near = []
    for h in range(256):
        for r in range(nr[h]):
            d = tv.sampson_sq(Es[h, r], x1, x2)
            band = np.abs(d - t2) <= BAND * t2
            cnt, fuzzy = int(((d < t2) & ~band).sum()), int(band.sum())
            if best is None or cnt > best[0]:
                best = (cnt, h, r)
            near.append((cnt, fuzzy, h, r))
    rivals = [(c, f, h, r) for c, f, h, r in near if c + f >= best[0] and (h, r) != (best[1], best[2])]
    if not any(f for _, f, _, _ in rivals):              # nothing in a band could change the order: the winner is determined
        assert (st[1], st[2]) == (best[1], best[2]) and st[0] == best[0]
    else:
        assert (st[1], st[2]) in [(best[1], best[2])] + [(h, r) for _, _, h, r in rivals]


# ------------------------------------------------------------------------------------------------ 4. determinism and batching
def _ragged_pairs(rng, B, special, where):
    sizes = [0, 4, 5, 6, 200, 2000]
    pairs = []
    for b in range(B):
        if b == where:
            pairs.append(special)
            continue
        n = sizes[b % len(sizes)]
        sc = tv.make_scene(rng, max(n, 1), 0.5, 0.3)
        pairs.append((sc["px1"][:n], sc["px2"][:n]))
    return pairs


def test_result_is_bit_identical_alone_and_at_either_end_of_ragged_batches(gpu_ctx):
    import slamhip

    sc = tv.make_scene(np.random.default_rng(31), 200, 0.5, 0.3)
    special = (sc["px1"], sc["px2"])
    E0, m0, s0 = slamhip.find_essential_batch([special], K, seed=5, ctx=gpu_ctx)
    assert s0[0, 0] > 100 and s0[0, 1] >= 0
    for B in (2, 17, 256):
        for where in (0, B - 1):
            pairs = _ragged_pairs(np.random.default_rng(100 + B), B, special, where)
            E, masks, st = slamhip.find_essential_batch(pairs, K, seed=5, ctx=gpu_ctx)
            assert np.array_equal(E[where], E0[0]) and np.array_equal(masks[where], m0[0]) and np.array_equal(st[where], s0[0]), (B, where)
            for b, (p1, _) in enumerate(pairs):
                if len(p1) < 5:
                    assert not E[b].any() and not masks[b].any() and st[b].tolist() == [0, -1, -1, 0]
                else:
                    assert st[b, 0] == masks[b].sum() and st[b, 0] >= 5 and st[b, 3] > 0
    E1, m1, s1 = slamhip.find_essential_batch([special], K, seed=5, ctx=gpu_ctx)
    assert np.array_equal(E1, E0) and np.array_equal(s1, s0)           # run to run
    E2, _, s2 = slamhip.find_essential_batch([special], K, seed=6, ctx=gpu_ctx)
    assert (s2[0, 1], s2[0, 2]) != (s0[0, 1], s0[0, 2]) or not np.array_equal(E2, E0)      # another seed, other draws
    assert tv.draw_sample(5, 0, int(s0[0, 1]), 200) != tv.draw_sample(6, 0, int(s0[0, 1]), 200)


def test_bad_offsets_never_leave_the_arrays_and_are_counted(gpu_ctx):
    import ctypes

    import slamhip

    sc = tv.make_scene(np.random.default_rng(32), 300, 0.5, 0.0)
    n = ctypes.c_int64(-1)
    gpu_ctx.lib.slam_index_errors(gpu_ctx.handle, ctypes.byref(n))     # clear
    off = np.array([-50, 100, 10 ** 6, 300], np.int32)                  # starts before 0; leaves the arrays; descends
    E, mask, st = slamhip.find_essential_offsets(sc["px1"], sc["px2"], off, K, 64, 1.0, 0, ctx=gpu_ctx)
    pose, good, ps = slamhip.recover_pose_offsets(E, sc["px1"], sc["px2"], off, K, None, ctx=gpu_ctx)
    assert gpu_ctx.lib.slam_index_errors(gpu_ctx.handle, ctypes.byref(n)) == 0
    assert n.value == 6                                                 # three clamped pairs, seen by each of the two calls
    assert st[0, 0] == mask[:100].sum() and st[0, 0] > 50               # pair 0 shrank to [0, 100)
    assert st[1, 0] == mask[100:].sum() and st[1, 0] > 100              # pair 1 shrank to [100, 300)
    assert st[2].tolist() == [0, -1, -1, 0]                             # pair 2 shrank to nothing
    assert np.isfinite(pose).all()
    gpu_ctx.lib.slam_index_errors(gpu_ctx.handle, ctypes.byref(n))
    assert n.value == 0


# ------------------------------------------------------------------------------------------------ 5. end to end
def test_end_to_end_against_ground_truth_and_the_numpy_ransac(gpu_ctx):
    import slamhip

    scenes = [(share, tv.make_scene(np.random.default_rng(40 + i), 200, 0.5, share)) for i, share in enumerate((0.0, 0.3, 0.5) * 3)]
    R, t, masks, counts = slamhip.verify_pairs([(sc["px1"], sc["px2"]) for _, sc in scenes], K, seed=0, ctx=gpu_ctx)

    def twin(sc, seed):
        E, mask, _ = tv.ransac(sc["px1"], sc["px2"], K, 256, 1.0, seed)
        Rt, tt, _, _ = tv.recover_pose(E, sc["px1"], sc["px2"], K)
        return (tv.rotation_angle_deg(Rt, sc["R"]), tv.direction_angle_deg(tt, sc["t"]),
                float(mask[sc["true_inlier"]].mean()))

    a = [twin(sc, 0) for _, sc in scenes]
    b = [twin(sc, 1) for _, sc in scenes]
    margin = np.abs(np.array(a) - np.array(b)).max(0)      # the method's own noise: two seeds on the same scenes
    print("margins (rot deg, dir deg, inlier share):", margin)
    for i, (share, sc) in enumerate(scenes):
        rot, dr = tv.rotation_angle_deg(R[i], sc["R"]), tv.direction_angle_deg(t[i], sc["t"])
        rec = float(masks[i][sc["true_inlier"]].mean())
        print(f"outliers {share}: product rot {rot:.4f} dir {dr:.4f} recovered {rec:.3f} | numpy {a[i][0]:.4f} {a[i][1]:.4f} {a[i][2]:.3f}")
        assert rot <= a[i][0] + margin[0] and dr <= a[i][1] + margin[1] and rec >= a[i][2] - margin[2]
        assert counts[i] == masks[i].sum()
        assert abs(np.linalg.norm(t[i]) - 1) < 1e-12 and np.abs(R[i].T @ R[i] - np.eye(3)).max() < 1e-12


def test_recover_pose_picks_the_true_candidate_from_the_true_matrix(gpu_ctx):
    import slamhip

    rng = np.random.default_rng(50)
    scenes = [tv.make_scene(rng, 60, 0.0, 0.0) for _ in range(64)]
    E = np.stack([sc["E"] * (1 if i % 2 else -1) for i, sc in enumerate(scenes)])       # either sign of E is the same matrix
    R, t, masks, st = slamhip.recover_pose_batch(E, [(sc["px1"], sc["px2"]) for sc in scenes], K, ctx=gpu_ctx)
    for i, sc in enumerate(scenes):
        assert np.abs(R[i] - sc["R"]).max() < 1e-9 and np.abs(t[i] - sc["t"]).max() < 1e-9, i
        assert st[i, 0] == 60 and masks[i].all() and 0 <= st[i, 1] < 4
        Rt, tt, _, ts = tv.recover_pose(E[i], sc["px1"], sc["px2"], K)
        assert np.abs(Rt - R[i]).max() < 1e-9 and np.abs(tt - t[i]).max() < 1e-9         # the same pose as numpy (which of the two
        # rotations an SVD calls R1 is its own business: the candidate NUMBER is not comparable, with OpenCV neither)
    n, R1, t1, m1 = slamhip.recover_pose_arrays(np.zeros((3, 3)), scenes[0]["px1"], scenes[0]["px2"], K, ctx=gpu_ctx)
    assert n == 0 and np.array_equal(R1, np.eye(3)) and not m1.any()


# ------------------------------------------------------------------------------------------------ 6. triangulation
def test_triangulation_against_truth_numpy_and_the_residual_kernel(gpu_ctx):
    import slamhip
    from backend import Backend

    sc = tv.make_scene(np.random.default_rng(60), 1000, 0.0, 0.0)
    P1, P2 = np.eye(4)[:3], np.c_[sc["R"], sc["t"]]
    x1, x2 = tv.normalise(sc["px1"], K), tv.normalise(sc["px2"], K)
    X, w = slamhip.triangulate_arrays(P1, P2, x1, x2, ctx=gpu_ctx)
    # noise-free: the smallest singular value is 0; through A^T A the vector is good to eps * cond^2, with cond <= 1e3 for a unit
    # baseline at depth <= 20: 1e-10 relative
    assert np.abs(X - sc["X"]).max() <= 1e-10 * 20 * 10 and (w > 0).all()
    noisy = tv.make_scene(np.random.default_rng(61), 1000, 0.5, 0.0)
    P2 = np.c_[noisy["R"], noisy["t"]]
    x1, x2 = tv.normalise(noisy["px1"], K), tv.normalise(noisy["px2"], K)
    X, w = slamhip.triangulate_arrays(P1, P2, x1, x2, ctx=gpu_ctx)
    Xs, ws = tv.triangulate(P1, P2, x1, x2)
    Xe, we = tv.triangulate_eig(P1, P2, x1, x2)
    scale = np.linalg.norm(Xs, axis=1)
    own = (np.linalg.norm(Xe - Xs, axis=1) / scale).max()              # numpy: SVD of A against eigenvectors of A^T A
    got = (np.linalg.norm(X - Xs, axis=1) / scale).max()
    print(f"triangulation: kernel vs SVD {got:.3e}, numpy eigh vs SVD {own:.3e}")
    assert got <= FACTOR * own and np.abs(w - ws).max() <= FACTOR * max(np.abs(we - ws).max(), 1e-16)
    Xb, xb = Backend().triangulate(np.eye(4), np.vstack([P2, [0, 0, 0, 1]]), noisy["px1"], noisy["px2"], *K)
    assert Xb.shape == (1000, 3) and xb.shape == (1000, 2) and np.array_equal(Xb, X) and np.array_equal(xb, x1)
    err = slamhip.mean_reprojection_error(X, noisy["px1"], np.eye(4), K, ctx=gpu_ctx)
    proj = np.stack([K[0] * X[:, 0] / X[:, 2] + K[2], K[1] * X[:, 1] / X[:, 2] + K[3]], 1)
    assert abs(err - np.linalg.norm(proj - noisy["px1"], axis=1).mean()) < 1e-9
    assert 0 < err < 1.0


# ------------------------------------------------------------------------------------------------ 7. the real image pair
def test_real_image_pair_runs_end_to_end(gpu_ctx):
    import slamhip

    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "image_descriptors.npz"))
    q, t, _ = slamhip.ratio_test_arrays(z["desc2"], z["desc1"], 0.75, ctx=gpu_ctx)       # current frame = query, last frame = train
    assert len(q) >= 20
    px1, px2 = z["kp1"][t].astype(np.float64), z["kp2"][q].astype(np.float64)
    Kd = (520.9, 521.0, 325.1, 249.7)
    R, tr, mask = slamhip.estimate_two_view(px1, px2, Kd, ctx=gpu_ctx)
    assert np.abs(R.T @ R - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12 and abs(np.linalg.norm(tr) - 1) < 1e-12
    E, m2 = slamhip.find_essential_arrays(px1, px2, Kd, ctx=gpu_ctx)
    assert np.array_equal(m2, mask)
    d = tv.sampson_sq(E.reshape(9), tv.normalise(px1, Kd), tv.normalise(px2, Kd))
    t2 = tv.threshold_sq(1.0, Kd)
    band = np.abs(d - t2) <= BAND * t2
    assert not band.any() and int((d < t2).sum()) == int(mask.sum())
    print("real pair:", len(q), "matches,", int(mask.sum()), "inliers")


# ------------------------------------------------------------------------------------------------ the batch amortises the launch
def test_a_batch_of_256_pairs_takes_less_than_256_single_calls(gpu_ctx):
    rng = np.random.default_rng(70)
    scenes = [tv.make_scene(rng, 200, 0.5, 0.3) for _ in range(256)]
    px1 = np.concatenate([s["px1"] for s in scenes])
    px2 = np.concatenate([s["px2"] for s in scenes])
    off = np.arange(257, dtype=np.int32) * 200
    d1, d2, do = gpu_ctx.upload(px1), gpu_ctx.upload(px2), gpu_ctx.upload(off)
    dE, dm, ds = gpu_ctx.malloc(256 * 72), gpu_ctx.malloc(len(px1)), gpu_ctx.malloc(256 * 16)
    lib, h = gpu_ctx.lib, gpu_ctx.handle

    def batch():
        assert lib.slam_tv_essential_ransac_f64(h, 256, do.ptr, d1.ptr, d2.ptr, len(px1), *K, 256, 1.0, 0, dE.ptr, dm.ptr, ds.ptr) == 0

    def singles():
        for b in range(256):
            assert lib.slam_tv_essential_ransac_f64(h, 1, do.ptr + 4 * b, d1.ptr, d2.ptr, len(px1), *K, 256, 1.0, 0,
                                                    dE.ptr + 72 * b, dm.ptr, ds.ptr + 16 * b) == 0

    def timed(fn):
        gpu_ctx.timer_start()
        fn()
        return gpu_ctx.timer_stop()

    try:
        timed(batch), timed(singles)                      # warm-up
        tb = np.median([timed(batch) for _ in range(5)])
        Eb = dE.download(np.float64, (256, 9))
        ts = np.median([timed(singles) for _ in range(5)])
        print(f"256 pairs x 200 matches, H = 256: batch {tb:.3f} ms, 256 single calls {ts:.3f} ms")
        assert np.array_equal(dE.download(np.float64, (256, 9)), Eb)
        assert tb < ts
    finally:
        for o in (d1, d2, do, dE, dm, ds):
            o.free()
