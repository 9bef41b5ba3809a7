"""Sim(3) refinement by reprojection error on the GPU (slam_sim3_optimize_f64) against the host twin of csrc/sim3_opt.hip
(tests/sim3_opt_twin.py), BIT FOR BIT on model, mask, chi2 and stats: the file is compiled with contraction off and uses
+ - * / sqrt only, and the sums are formed in the order the header states, so the device must give what the host build of
the same source gives - no tolerance anywhere.  What the twin itself is worth is tests/test_sim3_opt_cpu.py's business (numpy
on another route, 16 x yardsticks).  Then batching, the LDS / global boundary, the contract's edges, the Python layer and
one relative timing."""
import ctypes

import numpy as np
import pytest

import sim3_opt_ref as ref
import sim3_opt_twin as tw

pytestmark = pytest.mark.gpu
K = ref.EUROC
STAGE = 512                                    # SLAM_SIM3_OPT_STAGE: pairs kept in LDS
SIZES = [0, 1, 9, 10, 11, STAGE - 1, STAGE, STAGE + 1, 600]


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


def _chi2_same(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and _bits(np.where(na, 0.0, a), np.where(nb, 0.0, b))


def _cand(sc, sigma=True):
    return (sc["X1"], sc["X2"], sc["px1"], sc["px2"]) + ((sc["sigma2"],) if sigma else ())


def _twin(sc, start, sigma=True, **kw):
    return tw.optimize(sc["X1"], sc["X2"], sc["px1"], sc["px2"], start, K, sc["sigma2"] if sigma else None, **kw)


def _is_the_twin(out, b, twin, what=""):
    s, R, t, masks, st, chi2 = out
    m, mask, c, stt = twin
    assert _bits(ref.pack(s[b], R[b], t[b]), m), (what, b, "model")
    assert np.array_equal(masks[b], mask) and st[b].tolist() == stt.tolist(), (what, b, st[b], stt)
    assert _chi2_same(chi2[b], c), (what, b, "chi2")


def _sized(n, seed=0):
    """A noisy scene of n pairs (30 % planted outliers from 50 pairs up) and a moved start."""
    rng = np.random.default_rng(900 + n + 7919 * seed)
    sc = ref.make_scene(rng, n, 1.2, 1.0, 0.3 if n >= 50 else 0.0, with_sigma=bool(seed % 2))
    return sc, ref.moved(rng, sc["model"])


@pytest.fixture(scope="module")
def scenes():
    return ref.scene_list()


@pytest.fixture(scope="module")
def mixed():
    """64 candidates of mixed sizes with their twin results: computed once, shared, never changed."""
    sizes = [SIZES[b % len(SIZES)] if b % 4 else 40 + 7 * b for b in range(64)]      # (9 and 4 are coprime: every size occurs)
    items = [_sized(n, b) for b, n in enumerate(sizes)]
    return items, [_twin(sc, start) for sc, start in items]


# ------------------------------------------------------------------------------------------------ device == twin
@pytest.mark.parametrize("fix_scale", [False, True])
@pytest.mark.parametrize("with_sigma", [False, True])
def test_every_scene_is_the_twin_bit_for_bit(gpu_ctx, scenes, with_sigma, fix_scale):
    import slamhip

    names = list(scenes)
    out = slamhip.optimize_sim3_batch([_cand(scenes[n][0], with_sigma) for n in names], np.stack([scenes[n][1] for n in names]), K,
                                      fix_scale=fix_scale, ctx=gpu_ctx)
    for b, n in enumerate(names):
        sc, start, _ = scenes[n]
        _is_the_twin(out, b, _twin(sc, start, with_sigma, fix_scale=fix_scale), n)
        print(n, out[4][b])
        assert out[4][b, 0] == out[3][b].sum() >= 100 and (not fix_scale or out[0][b].tobytes() == start[12].tobytes())


@pytest.mark.parametrize("n", SIZES)
def test_sizes_across_min_pairs_and_the_lds_stage(gpu_ctx, n):
    import slamhip

    sc, start = _sized(n)
    ok, s, R, t, mask, st, chi2 = slamhip.optimize_sim3(sc["X1"], sc["X2"], sc["px1"], sc["px2"], start, K, ctx=gpu_ctx)
    m, maskt, c, stt = _twin(sc, start, sigma=False)
    assert _bits(ref.pack(s, R, t), m) and np.array_equal(mask, maskt) and st.tolist() == stt.tolist() and _chi2_same(chi2, c)
    assert ok == (n >= 10) and (ok or _bits(m, start)) and (not ok or st[0] >= 0.6 * n)


def test_a_batch_of_64_mixed_sizes_is_64_single_results(gpu_ctx, mixed):
    import slamhip

    items, twins = mixed
    out = slamhip.optimize_sim3_batch([_cand(sc) for sc, _ in items], np.stack([st for _, st in items]), K, ctx=gpu_ctx)
    for b in range(64):
        _is_the_twin(out, b, twins[b], "batch")
    for b in (0, 5, 17, 23, 40, 62, 63):                                # alone on the device: the same bits as member b of 64
        sc, start = items[b]
        one = slamhip.optimize_sim3_batch([_cand(sc)], start[None], K, ctx=gpu_ctx)
        _is_the_twin(one, 0, twins[b], "single")
    again = slamhip.optimize_sim3_batch([_cand(sc) for sc, _ in items], np.stack([st for _, st in items]), K, ctx=gpu_ctx)      # run to run
    assert _bits(again[0], out[0]) and _bits(again[1], out[1]) and _bits(again[2], out[2]) and np.array_equal(again[4], out[4])
    assert all(np.array_equal(a, b) for a, b in zip(again[3], out[3])) and all(_chi2_same(a, b) for a, b in zip(again[5], out[5]))


@pytest.mark.parametrize("fix_scale", [False, True])
def test_extreme_finite_data_is_the_twin_bit_for_bit(gpu_ctx, fix_scale):
    import slamhip

    cases = ref.extreme_cases()
    out = slamhip.optimize_sim3_batch([_cand(sc) for sc, _ in cases.values()], np.stack([st for _, st in cases.values()]), K,
                                      fix_scale=fix_scale, ctx=gpu_ctx)
    for b, (name, (sc, start)) in enumerate(cases.items()):
        print(name, out[4][b])
        _is_the_twin(out, b, _twin(sc, start, fix_scale=fix_scale), name)
    assert np.isfinite(out[0]).all() and np.isfinite(out[1]).all() and np.isfinite(out[2]).all() and (out[0] > 0).all()


def test_bad_offsets_never_leave_the_arrays_and_are_counted(gpu_ctx):
    import slamhip

    sc, start = _sized(300)
    n = ctypes.c_int64(-1)
    gpu_ctx.lib.slam_index_errors(gpu_ctx.handle, ctypes.byref(n))     # clear
    off = np.array([-50, 100, 10 ** 6, 300], np.int32)                  # starts before 0; leaves the arrays; descends
    starts = np.stack([start] * 3)
    s, R, t, mask, st, chi2 = slamhip.optimize_sim3_offsets(sc["X1"], sc["X2"], sc["px1"], sc["px2"], off, starts, K, ctx=gpu_ctx)
    assert gpu_ctx.lib.slam_index_errors(gpu_ctx.handle, ctypes.byref(n)) == 0 and n.value == 3
    sub = lambda a, b: {k: sc[k][a:b] for k in ("X1", "X2", "px1", "px2", "sigma2")}
    for b, (lo, hi) in enumerate(((0, 100), (100, 300), (300, 300))):   # each candidate shrank to the part inside
        m, maskt, c, stt = _twin(sub(lo, hi), start, sigma=False)
        assert _bits(ref.pack(s[b], R[b], t[b]), m) and np.array_equal(mask[lo:hi], maskt) and st[b].tolist() == stt.tolist()
        assert _chi2_same(chi2[lo:hi], c)
    assert st[2, 3] & ref.REJECTED
    s, R, t, mask, st, chi2 = slamhip.optimize_sim3_offsets(sc["X1"], sc["X2"], sc["px1"], sc["px2"], [50, 100, 280], starts[:2], K, ctx=gpu_ctx)
    assert not mask[:50].any() and not mask[280:].any() and np.isnan(chi2[:50]).all() and np.isnan(chi2[280:]).all()
    gpu_ctx.lib.slam_index_errors(gpu_ctx.handle, ctypes.byref(n))
    assert n.value == 0                                                 # a table that leaves gaps is fine


def test_a_nan_pair_and_an_invalid_model_beside_clean_candidates(gpu_ctx, mixed):
    import slamhip

    items, twins = mixed
    pick = [4, 7, 8, 13, 16, 20]                                        # 68, 513, 96, 11, 152, 180 pairs
    cands, starts = [_cand(items[b][0]) for b in pick], np.stack([items[b][1] for b in pick])
    clean = slamhip.optimize_sim3_batch(cands, starts, K, ctx=gpu_ctx)
    dirty_sc = {k: v.copy() for k, v in items[pick[2]][0].items() if k in ("X1", "X2", "px1", "px2", "sigma2")}
    dirty_sc["X1"][1] = np.nan; dirty_sc["px2"][3, 0] = np.inf; dirty_sc["sigma2"][5, 1] = 0.0; dirty_sc["X2"][6, 2] = -1.0
    cands2, starts2 = list(cands), starts.copy()
    cands2[2] = _cand(dirty_sc)
    starts2[4, 12] = -2.0                                               # an invalid model
    starts2[0, 5] = np.nan                                              # and a non-finite one
    out = slamhip.optimize_sim3_batch(cands2, starts2, K, ctx=gpu_ctx)
    for b in (1, 3, 5):                                                 # the clean ones: untouched by their neighbours
        _is_the_twin(out, b, twins[pick[b]], "clean")
        assert _bits(out[1][b], clean[1][b]) and np.array_equal(out[4][b], clean[4][b])
    _is_the_twin(out, 2, _twin(dirty_sc, starts2[2]), "dirty")
    assert not out[3][2][[1, 3, 5, 6]].any() and np.isnan(out[5][2][[1, 3, 5, 6]]).all() and out[4][2, 0] > 0
    for b in (0, 4):
        assert out[4][b].tolist() == [0, 0, 0, ref.REJECTED | ref.BAD_MODEL] and not out[3][b].any() and np.isnan(out[5][b]).all()
        assert np.array_equal(ref.pack(out[0][b], out[1][b], out[2][b]), ref.base.IDENTITY)
    assert np.isfinite(out[0]).all() and np.isfinite(out[1]).all() and np.isfinite(out[2]).all()


@pytest.mark.parametrize("poison", [0x00, 0xFF, 0x7F])
def test_poisoned_output_buffers_are_overwritten_where_the_contract_says(gpu_ctx, poison):
    sc, start = _sized(300)
    big, bstart = _sized(600)                                           # one staged candidate, a gap, one on the global path
    X1, X2 = np.concatenate([sc["X1"], big["X1"]]), np.concatenate([sc["X2"], big["X2"]])
    p1, p2 = np.concatenate([sc["px1"], big["px1"]]), np.concatenate([sc["px2"], big["px2"]])
    off = np.array([20, 300, 300], np.int32)
    off2 = np.array([300, 900], np.int32)
    M = 900
    bufs = [gpu_ctx.upload(a) for a in (X1, X2, p1, p2, off, off2, np.stack([start, start]), bstart[None])]
    d1, d2, dp1, dp2, do, do2, dz, dz2 = bufs
    outs = [gpu_ctx.upload(np.full(nb, poison, np.uint8)) for nb in (3 * 104, M, M * 16, 3 * 16)]
    dT, dm, dc, ds = outs
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    try:
        assert lib.slam_sim3_optimize_f64(h, 2, do.ptr, d1.ptr, d2.ptr, dp1.ptr, dp2.ptr, M, None, dz.ptr, *K, 10.0, 5, 10, 5, 10, 0, dT.ptr,
                                          dm.ptr, dc.ptr, ds.ptr) == 0
        T, mask, chi2, st = dT.download(np.float64, (3, 13)), dm.download(np.uint8, (M,)), dc.download(np.float64, (M, 2)), ds.download(np.int32, (3, 4))
        word = np.frombuffer(bytes([poison]) * 8, np.float64)[0]
        m, maskt, c, stt = tw.optimize(sc["X1"][20:], sc["X2"][20:], sc["px1"][20:], sc["px2"][20:], start, K)
        assert _bits(T[0], m) and np.array_equal(mask[20:300], maskt) and _chi2_same(chi2[20:300], c) and st[0].tolist() == stt.tolist()
        assert _bits(T[1], start) and st[1].tolist() == [0, 0, 0, ref.REJECTED | ref.STALLED]           # the empty candidate
        assert not mask[:20].any() and not mask[300:].any()             # the mask is 0 outside every candidate ...
        assert _bits(chi2[:20], np.full((20, 2), word)) and _bits(chi2[300:], np.full((600, 2), word))    # ... chi2 is not written there
        assert _bits(T[2], np.full(13, word)) and st[2].tobytes() == bytes([poison]) * 16               # nor anything of a candidate beyond B
        for o, nb in zip(outs, (3 * 104, M, M * 16, 3 * 16)):
            o.upload(np.full(nb, poison, np.uint8))
        assert lib.slam_sim3_optimize_f64(h, 1, do2.ptr, d1.ptr, d2.ptr, dp1.ptr, dp2.ptr, M, None, dz2.ptr, *K, 10.0, 5, 10, 5, 10, 0, dT.ptr,
                                          dm.ptr, dc.ptr, ds.ptr) == 0   # the global path leaves its flags in d_inlier meanwhile
        T, mask, chi2, st = dT.download(np.float64, (3, 13)), dm.download(np.uint8, (M,)), dc.download(np.float64, (M, 2)), ds.download(np.int32, (3, 4))
        m, maskt, c, stt = _twin(big, bstart, sigma=False)
        assert _bits(T[0], m) and np.array_equal(mask[300:], maskt) and _chi2_same(chi2[300:], c) and st[0].tolist() == stt.tolist()
        assert not mask[:300].any() and set(np.unique(mask)) <= {0, 1}
    finally:
        for o in bufs + outs:
            o.free()


# ------------------------------------------------------------------------------------------------ the Python layer
def test_compute_sim3_accepts_a_planted_loop_and_rejects_outliers(gpu_ctx):
    import slamhip
    from backend import Backend

    rng = np.random.default_rng(77)
    loop = ref.make_scene(rng, 200, 1.15, 1.0, 0.3)
    junk = ref.make_scene(rng, 200, 0.9, 1.0, 1.0)                      # every match is wrong
    small = ref.make_scene(rng, 15, 1.0, 1.0)                           # a true loop with too few matches to accept
    cands = [_cand(loop), _cand(junk, False), _cand(small, False)]
    models, masks, counts, accepted = Backend().compute_sim3(cands, K)
    s0, R0, t0, rmasks, _, _ = slamhip.estimate_sim3_batch([(c[0], c[1]) for c in cands], K, ctx=gpu_ctx)
    print("counts", counts, "ransac", [int(m.sum()) for m in rmasks])
    assert accepted.tolist() == [True, False, False] and counts[0] >= 20 and counts[1] < 20 and counts[2] <= 15
    assert counts[0] == masks[0].sum() and not masks[0][~loop["true_inlier"]].any() and masks[0][loop["true_inlier"]].mean() >= 0.9
    assert not (masks[0] & ~rmasks[0]).any()                            # over the candidate's own indexing: a subset of the RANSAC vote
    refined, start = ref.pack(models[0][0], models[1][0], models[2][0]), ref.pack(s0[0], R0[0], t0[0])
    cost = lambda m: float(ref.chi2(m, loop, K)[0][masks[0]].sum())
    print(f"reprojection cost over the final inliers: RANSAC + refit {cost(start):.2f}, refined {cost(refined):.2f}")
    assert cost(refined) < cost(start)
    edges, meas, info = slamhip.sim3_edges_from_sim3([[0, 9], [1, 9], [2, 9]], models, counts)      # the models go on unchanged
    assert edges.tolist() == [[0, 9]] and _bits(meas[0], refined)
    S12 = slamhip.sim3_to_s12(models)
    assert S12.shape == (3, 3, 4) and np.abs(loop["X2"][masks[0]] @ S12[0][:, :3].T + S12[0][:, 3] - loop["X1"][masks[0]]).max() < 0.5
    full = slamhip.compute_sim3(cands, K, ctx=gpu_ctx)
    assert _bits(full[0][0], models[0]) and np.array_equal(full[2], counts) and full[4].shape == (3, 4)


# ------------------------------------------------------------------------------------------------ the batch amortises the launch
def test_a_batch_of_64_candidates_takes_less_than_64_single_calls(gpu_ctx):
    rng = np.random.default_rng(70)
    sc = [ref.make_scene(rng, 200, 1.2, 1.0, 0.3) for _ in range(64)]
    cat = lambda k: np.concatenate([s[k] for s in sc])
    starts = np.stack([ref.moved(rng, s["model"]) for s in sc])
    off = np.arange(65, dtype=np.int32) * 200
    M = 64 * 200
    bufs = [gpu_ctx.upload(a) for a in (cat("X1"), cat("X2"), cat("px1"), cat("px2"), off, starts)]
    d1, d2, dp1, dp2, do, dz = bufs
    outs = [gpu_ctx.malloc(64 * 104), gpu_ctx.malloc(M), gpu_ctx.malloc(M * 16), gpu_ctx.malloc(64 * 16)]
    dT, dm, dc, ds = outs
    lib, h = gpu_ctx.lib, gpu_ctx.handle

    def batch():
        assert lib.slam_sim3_optimize_f64(h, 64, do.ptr, d1.ptr, d2.ptr, dp1.ptr, dp2.ptr, M, None, dz.ptr, *K, 10.0, 5, 10, 5, 10, 0, dT.ptr,
                                          dm.ptr, dc.ptr, ds.ptr) == 0

    def singles():
        for b in range(64):
            assert lib.slam_sim3_optimize_f64(h, 1, do.ptr + 4 * b, d1.ptr, d2.ptr, dp1.ptr, dp2.ptr, M, None, dz.ptr + 104 * b, *K, 10.0, 5, 10,
                                              5, 10, 0, dT.ptr + 104 * b, dm.ptr, dc.ptr, ds.ptr + 16 * b) == 0

    def timed(fn):
        gpu_ctx.timer_start()
        fn()
        return gpu_ctx.timer_stop()

    try:
        timed(batch), timed(singles)                      # warm-up
        tb = np.median([timed(batch) for _ in range(5)])
        Tb = dT.download(np.float64, (64, 13))
        ts = np.median([timed(singles) for _ in range(5)])
        print(f"64 candidates x 200 pairs: batch {tb:.3f} ms, 64 single calls {ts:.3f} ms")
        assert _bits(dT.download(np.float64, (64, 13)), Tb)
        assert tb < ts
    finally:
        for o in bufs + outs:
            o.free()
