"""Sim(3) alignment on the GPU (slam_sim3_*) against the host twin of csrc/sim3.hip (tests/sim3_twin.py), BIT FOR BIT: the file
is compiled with contraction off and uses + - * / sqrt only, and the refit's sums are formed in the order the header states,
so the device must give what the host build of the same source gives - no tolerance anywhere.  What the twin itself is worth
is tests/test_sim3_cpu.py's business (numpy on another route, 16 x yardsticks).  Then batching, the kernels' own boundaries,
the Python layer and one relative timing."""
import ctypes

import numpy as np
import pytest

import sim3_ref as ref
import sim3_twin as tw

pytestmark = pytest.mark.gpu
K = ref.EUROC
CHUNK = 256                                    # S3_CHUNK of csrc/sim3.hip: correspondences staged in LDS at a time
BLOCK = 256                                    # S3_THREADS: hypotheses per block
NONE = [0, -1, -1, 0]


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


def _model(s, R, t, b=0):
    return ref.pack(s[b], R[b], t[b])


def _ransac_is_the_twin(gpu_ctx, X1, X2, H, seed, sigma2=None, fix_scale=False):
    import slamhip

    s, R, t, mask, st, rs = slamhip.estimate_sim3_offsets(X1, X2, [0, len(X1)], K, H, ref.CHI2, sigma2, fix_scale, seed, refit=False, ctx=gpu_ctx)
    mt, maskt, stt = tw.ransac(X1, X2, K, H, ref.CHI2, seed, sigma2, fix_scale)
    assert rs is None and _bits(_model(s, R, t), mt) and np.array_equal(mask, maskt) and st[0].tolist() == stt.tolist(), (st[0], stt)
    return st[0]


@pytest.fixture(scope="module")
def families():
    return ref.family_scenes()


# ------------------------------------------------------------------------------------------------ device == twin
def test_solver_is_the_twin_bit_for_bit(gpu_ctx):
    import slamhip

    X1, X2, _ = ref.solver_samples()
    for fix in (False, True):
        s, R, t, ok = slamhip.sim3_threepoint_arrays(X1, X2, fix, ctx=gpu_ctx)
        mt, okt = tw.threepoint(X1, X2, fix)
        st, Rt, tt = tw.split(mt)
        assert np.array_equal(ok, okt) and ok.all() and _bits(s, st) and _bits(R, Rt) and _bits(t, tt)
        assert not fix or (s == 1.0).all()
    s1, R1, t1, ok1 = slamhip.sim3_threepoint_arrays(X1[7], X2[7], ctx=gpu_ctx)             # one sample, [3,3]
    assert ok1[0] == 1 and _bits(_model(s1, R1, t1), tw.threepoint(X1[7], X2[7])[0][0])
    D1, D2, _ = ref.solver_samples(8, ref.SEED + 3)                                         # no model: identity, s = 1, ok = 0
    D1[0, 1] = D1[0, 0]; D2[1, 2] = D2[1, 0] - 0.5 * (D2[1, 1] - D2[1, 0]); D1[2, 0, 1] = np.nan; D2[3, 1, 1] = np.inf; D1[4, 2, 0] = 1e150
    s, R, t, ok = slamhip.sim3_threepoint_arrays(D1, D2, ctx=gpu_ctx)
    mt, okt = tw.threepoint(D1, D2)
    assert ok.tolist() == [0] * 5 + [1] * 3 and np.array_equal(ok, okt)
    assert all(_bits(_model(s, R, t, b), mt[b]) for b in range(8)) and all(np.array_equal(mt[b], ref.IDENTITY) for b in range(5))


@pytest.mark.parametrize("with_sigma", [False, True])
def test_ransac_is_the_twin_bit_for_bit_on_every_family(gpu_ctx, families, with_sigma):
    import slamhip

    sg = np.random.default_rng(2).choice([1.0, 1.44, 2.0736], (200, 2))
    cands = [(sc["X1"], sc["X2"]) + ((sg,) if with_sigma else ()) for sc in families.values()]
    s, R, t, masks, st, rs = slamhip.estimate_sim3_batch(cands, K, refit=False, ctx=gpu_ctx)
    assert rs is None
    for i, (name, sc) in enumerate(families.items()):
        mt, maskt, stt = tw.ransac(sc["X1"], sc["X2"], K, 256, ref.CHI2, 0, sg if with_sigma else None)
        print(name, st[i])
        assert _bits(_model(s, R, t, i), mt) and np.array_equal(masks[i], maskt) and st[i].tolist() == stt.tolist(), name
        assert st[i, 0] == masks[i].sum()
        if name.startswith("outliers"):
            assert masks[i][sc["true_inlier"]].all()


@pytest.mark.parametrize("n", [3, 4, CHUNK - 1, CHUNK, CHUNK + 1, 600])
def test_sizes_across_the_lds_chunk(gpu_ctx, n):
    sc = ref.make_scene(np.random.default_rng(300 + n), n, 1.3, 0.001, 0.0 if n < 5 else 0.3)
    st = _ransac_is_the_twin(gpu_ctx, sc["X1"], sc["X2"], 64, 2)
    assert st[0] >= 3


@pytest.mark.parametrize("H", [1, BLOCK - 1, BLOCK, BLOCK + 1, 1024])
def test_hypothesis_counts_across_the_block(gpu_ctx, families, H):
    sc = families["outliers_50"]
    st = _ransac_is_the_twin(gpu_ctx, sc["X1"], sc["X2"], H, 9)
    assert 0 <= st[1] < H and st[3] == H
    _ransac_is_the_twin(gpu_ctx, sc["X1"], sc["X2"], H, 9, fix_scale=True)


def test_refit_is_the_twin_bit_for_bit_with_and_without_a_mask(gpu_ctx):
    import slamhip

    X1s, X2s, masks, off = [], [], [], [0]
    for n in ref.REFIT_SIZES:
        for offset in (0.0, 1e4):
            sc = ref.refit_cloud(n, offset)
            X1s.append(sc["X1"]); X2s.append(sc["X2"]); off.append(off[-1] + n)
            masks.append(np.random.default_rng(n).random(n) < 0.7)
    X1, X2, mask = np.concatenate(X1s), np.concatenate(X2s), np.concatenate(masks)
    for mk in (None, mask):
        for fix in (False, True):
            s, R, t, st = slamhip.fit_sim3_offsets(X1, X2, off, mk, fix, ctx=gpu_ctx)
            for b in range(len(X1s)):
                mt, stt = tw.refit(X1s[b], X2s[b], None if mk is None else masks[b], fix)
                assert _bits(_model(s, R, t, b), mt) and st[b].tolist() == stt.tolist(), (b, mk is None, fix)
            assert st[:, 1].all() or mk is not None                     # (a mask may leave fewer than 3 of 3 or 4 points)
    sc = ref.refit_cloud(1000, 1e4)                                     # one candidate alone: the same bits as inside the batch
    ok, s1, R1, t1 = slamhip.fit_sim3(sc["X1"], sc["X2"], ctx=gpu_ctx)
    assert ok and _bits(ref.pack(s1, R1, t1), tw.refit(sc["X1"], sc["X2"])[0])


# ------------------------------------------------------------------------------------------------ batching
def test_one_candidate_and_three_with_an_empty_middle(gpu_ctx, families):
    import slamhip

    a, b = families["general"], families["outliers_30"]
    empty = (np.zeros((0, 3)), np.zeros((0, 3)))
    one = slamhip.estimate_sim3_batch([(a["X1"], a["X2"])], K, 64, seed=4, refit=False, ctx=gpu_ctx)
    three = slamhip.estimate_sim3_batch([(a["X1"], a["X2"]), empty, (b["X1"], b["X2"])], K, 64, seed=4, refit=False, ctx=gpu_ctx)
    assert _bits(_model(*one[:3]), _model(*three[:3])) and np.array_equal(one[3][0], three[3][0]) and np.array_equal(one[4][0], three[4][0])
    assert three[4][1].tolist() == NONE and np.array_equal(_model(*three[:3], 1), ref.IDENTITY) and len(three[3][1]) == 0
    mt, maskt, stt = tw.ransac(b["X1"], b["X2"], K, 64, ref.CHI2, 4)
    assert _bits(_model(*three[:3], 2), mt) and np.array_equal(three[3][2], maskt) and three[4][2].tolist() == stt.tolist()


def test_the_same_bits_alone_and_as_member_200_of_256(gpu_ctx, families):
    import slamhip

    sc = families["outliers_30"]
    special = (sc["X1"], sc["X2"])
    alone = slamhip.estimate_sim3_batch([special], K, 64, seed=5, refit=True, ctx=gpu_ctx)
    assert alone[4][0, 0] > 100 and alone[5][0].tolist() == [int(alone[3][0].sum()), 1]
    rng = np.random.default_rng(100)
    sizes = [0, 2, 3, 4, 100, 300]
    cands = []
    for b in range(256):
        n = sizes[b % len(sizes)]
        s = ref.make_scene(rng, max(n, 1), 1.1, 0.001, 0.3)
        cands.append(special if b == 200 else (s["X1"][:n], s["X2"][:n]))
    out = slamhip.estimate_sim3_batch(cands, K, 64, seed=5, refit=True, ctx=gpu_ctx)
    assert _bits(_model(*out[:3], 200), _model(*alone[:3])) and np.array_equal(out[3][200], alone[3][0])
    assert np.array_equal(out[4][200], alone[4][0]) and np.array_equal(out[5][200], alone[5][0])
    mt, stt = tw.refit(sc["X1"], sc["X2"], alone[3][0])                 # the refit ran on the RANSAC mask, on the device
    assert _bits(_model(*alone[:3]), mt) and stt.tolist() == alone[5][0].tolist()
    for b, (Xb, _) in enumerate(cands):
        if len(Xb) < 3:
            assert out[4][b].tolist() == NONE and np.array_equal(_model(*out[:3], b), ref.IDENTITY) and not out[3][b].any()
        else:
            assert out[4][b, 0] == out[3][b].sum()
    again = slamhip.estimate_sim3_batch([special], K, 64, seed=5, refit=True, ctx=gpu_ctx)      # run to run
    assert _bits(_model(*again[:3]), _model(*alone[:3])) and np.array_equal(again[4], alone[4])


def test_a_non_finite_candidate_changes_no_other_candidate(gpu_ctx):
    import slamhip

    rng = np.random.default_rng(11)
    base = [(s["X1"], s["X2"]) for s in (ref.make_scene(rng, 50 + (b % 5) * 40, 1.2, 0.001, 0.3) for b in range(32))]
    empty = (np.zeros((0, 3)), np.zeros((0, 3)))
    line = base[0][0][0] + np.arange(10)[:, None] * np.array([0.25, -0.5, 0.125])
    bad = {"all_nan": (np.full((10, 3), np.nan),) * 2, "inf": (np.full((10, 3), np.inf), base[0][1][:10]), "collinear": (line, base[0][1][:10])}
    for where in (0, 15, 31):
        for name, cand in bad.items():
            a, b = list(base), list(base)
            a[where], b[where] = cand, empty
            ra = slamhip.estimate_sim3_batch(a, K, 64, ctx=gpu_ctx)
            rb = slamhip.estimate_sim3_batch(b, K, 64, ctx=gpu_ctx)
            for k in range(32):
                if k != where:
                    assert _bits(_model(*ra[:3], k), _model(*rb[:3], k)) and np.array_equal(ra[3][k], rb[3][k]) \
                        and np.array_equal(ra[4][k], rb[4][k]) and np.array_equal(ra[5][k], rb[5][k]), (where, name, k)
            assert np.isfinite(ra[0]).all() and np.isfinite(ra[1]).all() and np.isfinite(ra[2]).all()
            assert ra[4][where].tolist() == NONE and np.array_equal(_model(*ra[:3], where), ref.IDENTITY) and ra[5][where, 1] == 0


def test_degenerate_candidates_are_the_twin(gpu_ctx):
    import slamhip

    sc = ref.make_scene(np.random.default_rng(12), 40, 1.2)
    for n in (0, 2):
        st = _ransac_is_the_twin(gpu_ctx, sc["X1"][:n], sc["X2"][:n], 32, 0)
        assert st.tolist() == NONE
    assert _ransac_is_the_twin(gpu_ctx, sc["X1"][:3], sc["X2"][:3], 32, 0).tolist() == [3, 0, 0, 32]
    assert _ransac_is_the_twin(gpu_ctx, sc["X1"], sc["X2"], 1, 0).tolist() == [40, 0, 0, 1]
    assert _ransac_is_the_twin(gpu_ctx, np.tile(sc["X1"][:1], (10, 1)), np.tile(sc["X2"][:1], (10, 1)), 32, 0).tolist() == NONE
    for val in (np.nan, np.inf, 1e150):
        X1, X2 = sc["X1"].copy(), sc["X2"].copy()
        X1[0, 0] = val; X2[1, 2] = -val; X1[2] = val
        st = _ransac_is_the_twin(gpu_ctx, X1, X2, 64, 0)
        assert st[0] == 37 and 0 < st[3] < 64
    two = ref.make_scene(np.random.default_rng(13), 100, 2.0)           # fix_scale on data whose true scale is 2
    ok, s, R, t, mask = slamhip.estimate_sim3(two["X1"], two["X2"], K, 32, fix_scale=True, ctx=gpu_ctx)
    assert ok and s == 1.0
    ok, s, R, t = slamhip.fit_sim3(two["X1"], two["X2"], fix_scale=True, ctx=gpu_ctx)
    assert ok and s == 1.0
    for X1, X2 in ((sc["X1"][:2], sc["X2"][:2]), (sc["X1"][[0, 0, 1]], sc["X2"][[0, 0, 1]]), (np.full((10, 3), np.nan), sc["X2"][:10])):
        ok, s, R, t = slamhip.fit_sim3(X1, X2, ctx=gpu_ctx)
        assert not ok and np.array_equal(ref.pack(s, R, t), ref.IDENTITY)


def test_bad_offsets_never_leave_the_arrays_and_are_counted(gpu_ctx):
    import slamhip

    sc = ref.make_scene(np.random.default_rng(32), 300, 1.4, 0.001)
    n = ctypes.c_int64(-1)
    gpu_ctx.lib.slam_index_errors(gpu_ctx.handle, ctypes.byref(n))     # clear
    off = np.array([-50, 100, 10 ** 6, 300], np.int32)                  # starts before 0; leaves the arrays; descends
    s, R, t, mask, st, _ = slamhip.estimate_sim3_offsets(sc["X1"], sc["X2"], off, K, 64, refit=False, ctx=gpu_ctx)
    assert gpu_ctx.lib.slam_index_errors(gpu_ctx.handle, ctypes.byref(n)) == 0
    assert n.value == 3                                                 # three clamped candidates
    m0, k0, s0 = tw.ransac(sc["X1"][:100], sc["X2"][:100], K, 64, ref.CHI2, 0)     # candidate 0 shrank to [0, 100)
    m1, k1, s1 = tw.ransac(sc["X1"][100:], sc["X2"][100:], K, 64, ref.CHI2, 0)     # candidate 1 shrank to [100, 300)
    assert _bits(_model(s, R, t, 0), m0) and np.array_equal(mask[:100], k0) and st[0].tolist() == s0.tolist()
    assert _bits(_model(s, R, t, 1), m1) and np.array_equal(mask[100:], k1) and st[1].tolist() == s1.tolist()
    assert st[2].tolist() == NONE and np.array_equal(_model(s, R, t, 2), ref.IDENTITY)          # candidate 2 shrank to nothing
    fs, fR, ft, fst = slamhip.fit_sim3_offsets(sc["X1"], sc["X2"], off, ctx=gpu_ctx)             # the refit counts alike
    gpu_ctx.lib.slam_index_errors(gpu_ctx.handle, ctypes.byref(n))
    assert n.value == 3 and fst.tolist() == [[100, 1], [200, 1], [0, 0]]
    assert _bits(_model(fs, fR, ft, 1), tw.refit(sc["X1"][100:], sc["X2"][100:])[0])
    s, R, t, mask, st, rs = slamhip.estimate_sim3_offsets(sc["X1"], sc["X2"], [50, 100, 280], K, 64, ctx=gpu_ctx)
    assert not mask[:50].any() and not mask[280:].any()                 # a table that leaves gaps is fine: entries outside are 0
    gpu_ctx.lib.slam_index_errors(gpu_ctx.handle, ctypes.byref(n))
    assert n.value == 0


# ------------------------------------------------------------------------------------------------ the Python layer
def test_refit_by_default_and_trajectory_alignment(gpu_ctx, families):
    import slamhip

    sc = families["outliers_30"]
    ok, s, R, t, mask = slamhip.estimate_sim3(sc["X1"], sc["X2"], K, ctx=gpu_ctx)               # refit=True by default
    _, _, _, _, mask0 = slamhip.estimate_sim3(sc["X1"], sc["X2"], K, refit=False, ctx=gpu_ctx)
    assert ok and np.array_equal(mask, mask0) and mask[sc["true_inlier"]].all()                 # the mask stays the RANSAC vote
    assert _bits(ref.pack(s, R, t), tw.refit(sc["X1"], sc["X2"], mask)[0])
    tr = ref.trajectory()
    s, R, t, aligned, rmse = slamhip.align_trajectory(tr["est"], tr["gt"], ctx=gpu_ctx)
    assert _bits(ref.pack(s, R, t), tw.refit(tr["est"], tr["gt"])[0]) and aligned.shape == (200, 3)
    print(f"ATE of a planted similarity of 200 poses: {rmse:.3e}")
    assert rmse <= 16 * 2.068e-15           # profiles/sim3_edges.log: "ate path200 rmse 2.068e-15 7.905e-16" (numpy, twin)
    s1, R1, t1, _, rmse1 = slamhip.align_trajectory(tr["est"], tr["gt"], fix_scale=True, ctx=gpu_ctx)
    assert s1 == 1.0 and rmse1 > 0.1                                    # SE(3) cannot absorb the planted scale of 0.37
    with pytest.raises(ValueError):
        slamhip.align_trajectory(np.arange(30.0).reshape(10, 3), np.arange(30.0).reshape(10, 3), ctx=gpu_ctx)      # poses on one line
    edges, meas, info, scales = slamhip.loop_edges_from_sim3([[0, 1]], (np.array([1.0]), R[None], t[None]), [50])
    assert edges.tolist() == [[0, 1]] and scales.tolist() == [1.0]


# ------------------------------------------------------------------------------------------------ the batch amortises the launch
def test_a_batch_of_256_candidates_takes_less_than_256_single_calls(gpu_ctx):
    rng = np.random.default_rng(70)
    sc = [ref.make_scene(rng, 200, 1.2, 0.001, 0.3) for _ in range(256)]
    X1 = np.concatenate([s["X1"] for s in sc])
    X2 = np.concatenate([s["X2"] for s in sc])
    off = np.arange(257, dtype=np.int32) * 200
    d1, d2, do = gpu_ctx.upload(X1), gpu_ctx.upload(X2), gpu_ctx.upload(off)
    dT, dm, ds = gpu_ctx.malloc(256 * 104), gpu_ctx.malloc(len(X1)), gpu_ctx.malloc(256 * 16)
    lib, h = gpu_ctx.lib, gpu_ctx.handle

    def batch():
        assert lib.slam_sim3_ransac_f64(h, 256, do.ptr, d1.ptr, d2.ptr, len(X1), None, *K, 256, ref.CHI2, 0, 0, dT.ptr, dm.ptr, ds.ptr) == 0

    def singles():
        for b in range(256):
            assert lib.slam_sim3_ransac_f64(h, 1, do.ptr + 4 * b, d1.ptr, d2.ptr, len(X1), None, *K, 256, ref.CHI2, 0, 0, dT.ptr + 104 * b,
                                            dm.ptr, ds.ptr + 16 * b) == 0

    def timed(fn):
        gpu_ctx.timer_start()
        fn()
        return gpu_ctx.timer_stop()

    try:
        timed(batch), timed(singles)                      # warm-up
        tb = np.median([timed(batch) for _ in range(5)])
        Tb = dT.download(np.float64, (256, 13))
        ts = np.median([timed(singles) for _ in range(5)])
        print(f"256 candidates x 200 correspondences, H = 256: batch {tb:.3f} ms, 256 single calls {ts:.3f} ms")
        assert np.array_equal(dT.download(np.float64, (256, 13)), Tb)
        assert tb < ts
    finally:
        for o in (d1, d2, do, dT, dm, ds):
            o.free()
