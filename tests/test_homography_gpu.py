"""Homography estimation on the GPU (slam_hg_*) against the host twin of csrc/homography.hip (tests/hg_twin.py), BIT FOR BIT:
the file is compiled with contraction off and uses + - * / sqrt only, so the device must give what the host build of the same
source gives; what the twin itself is worth is tests/test_homography_cpu.py's business (numpy on another route, 16 x yardsticks,
exact rational quadrilaterals).  Then batching, the kernel's own boundaries, the end-to-end choice and one relative timing."""
import ctypes

import numpy as np
import pytest

import hg_twin as tw
import homography_ref as hr
import two_view_ref as ref

pytestmark = pytest.mark.gpu
K = ref.EUROC
CHUNK = 256                                    # HG_CHUNK of csrc/homography.hip: matches staged in LDS at a time


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.fixture(scope="module")
def samples():
    p1, p2, _ = hr.fourpoint_samples(0, 2000)
    p1, p2 = p1.copy(), p2.copy()
    p1[5, 2] = p1[5, 0]                         # a repeated point, a NaN, 1e150, a triangle turned over: no model
    p2[70, 1, 0] = np.nan
    p1[130, 3] = [1e150, 1.0]
    p2[200, [0, 1]] = p2[200, [1, 0]]
    return p1, p2, tw.fourpoint(p1, p2)


@pytest.mark.parametrize("S", [1, 63, 64, 65, 2000])
def test_solver_is_the_twin_bit_for_bit(gpu_ctx, samples, S):
    import slamhip

    p1, p2, (Ht, okt) = samples
    H, ok = slamhip.fourpoint_homography_arrays(p1[:S], p2[:S], ctx=gpu_ctx)
    assert _bits(H.reshape(S, 9), Ht[:S]) and np.array_equal(ok, okt[:S] != 0) and np.isfinite(H).all()
    if S == 2000:
        assert not ok[[5, 70, 130, 200]].any() and ok.sum() == 1996 and not H[[5, 70, 130, 200]].any()


@pytest.fixture(scope="module")
def scenes():
    from oracle import oracle

    out = []
    for name, sc in hr.family_scenes() + [(f"planar_noisy/{s['variant']}", s) for s in hr.scenes_planar_noisy()]:
        H, mask, st = tw.ransac(sc["px1"], sc["px2"], 256, 3.0, 0)
        E, emask, est = oracle.tv_twin_ransac(sc["px1"], sc["px2"], sc["K"], 256, 1.0, 0)
        out.append(dict(name=name, sc=sc, H=H, mask=mask, st=st, E=E, emask=emask, est=est))
    return out


def test_ransac_decomposition_and_scores_are_the_twin_on_every_family_scene(gpu_ctx, scenes):
    import slamhip

    pairs = [(s["sc"]["px1"], s["sc"]["px2"]) for s in scenes]
    H, masks, st = slamhip.find_homography_batch(pairs, ctx=gpu_ctx)
    dec = slamhip.decompose_homography_batch(H, pairs, K, inliers=masks, ctx=gpu_ctx)
    px1, px2 = np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])
    off = np.arange(len(pairs) + 1) * 200
    score, ratio = slamhip.model_scores_offsets(H, np.array([s["E"] for s in scenes]), px1, px2, off, K, ctx=gpu_ctx)
    for i, s in enumerate(scenes):
        sc = s["sc"]
        assert _bits(H[i].reshape(9), s["H"]) and np.array_equal(masks[i], s["mask"]) and np.array_equal(st[i], s["st"]), s["name"]
        d = tw.decompose(sc["px1"], sc["px2"], K, s["H"], s["mask"])
        for k in ("pose_all", "normal_all", "pose", "sv"):
            assert _bits(dec[k][i], d[k]), (s["name"], k)
        assert np.array_equal(dec["count"][i], d["count"]) and np.array_equal(dec["stats"][i], d["stats"]) and np.array_equal(dec["good"][i], d["good"])
        ts, tr = tw.model_score(sc["px1"], sc["px2"], K, s["H"], s["E"])
        print(f"{s['name']:28s} stats {st[i]} decomposition {dec['stats'][i]} counts {dec['count'][i]} S_H {score[i, 0]} S_E {score[i, 1]} R_H {ratio[i]:.4f}")
        assert np.array_equal(score[i], ts) and _bits(ratio[i], tr), s["name"]
    # all matches (no selection) and a single pair through the one-pair wrappers
    s = scenes[1]
    P, N, cnt, sd = slamhip.decompose_homography_arrays(s["H"], s["sc"]["px1"], s["sc"]["px2"], K, ctx=gpu_ctx)
    d = tw.decompose(s["sc"]["px1"], s["sc"]["px2"], K, s["H"])
    assert _bits(P, d["pose_all"]) and _bits(N, d["normal_all"]) and np.array_equal(cnt, d["count"]) and np.array_equal(sd, d["stats"])
    H1, m1 = slamhip.find_homography_arrays(s["sc"]["px1"], s["sc"]["px2"], ctx=gpu_ctx)
    assert _bits(H1.reshape(9), s["H"]) and np.array_equal(m1, s["mask"])


# ------------------------------------------------------------------------------------------------ the kernel's own boundaries
@pytest.fixture(scope="module")
def big_planar():
    return hr.scenes_planar_noisy(seed=3, n=2 * CHUNK + 1)[1]


@pytest.mark.parametrize("n", [0, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
def test_sizes_across_the_lds_chunk(gpu_ctx, big_planar, n):
    import slamhip

    a, b = big_planar["px1"][:n], big_planar["px2"][:n]
    H, mask, st = slamhip.find_homography_offsets(a, b, [0, n], 64, 3.0, 2, ctx=gpu_ctx)
    Ht, mt, stt = tw.ransac(a, b, 64, 3.0, 2)
    assert _bits(H[0], Ht) and np.array_equal(mask, mt) and np.array_equal(st[0], stt)
    if n < 4:
        assert st[0].tolist() == [0, -1, -1, 0] and not H.any()
    else:
        assert st[0, 1] == -1 or st[0, 0] >= 4                     # a model counts at least its own sample


@pytest.mark.parametrize("H", [1, 255, 256, 257, 1024])
def test_hypothesis_counts_across_the_block(gpu_ctx, scenes, H):
    import slamhip

    sc = scenes[-1]["sc"]                       # planar, 0.5 px noise, 30 % outliers: the winner is not hypothesis 0
    Hm, mask, st = slamhip.find_homography_offsets(sc["px1"], sc["px2"], [0, 200], H, 3.0, 9, ctx=gpu_ctx)
    Ht, mt, stt = tw.ransac(sc["px1"], sc["px2"], H, 3.0, 9)
    assert _bits(Hm[0], Ht) and np.array_equal(mask, mt) and np.array_equal(st[0], stt)
    assert 0 <= st[0, 1] < H or st[0, 1] == -1


# ------------------------------------------------------------------------------------------------ batching
def _ragged(rng, B, special, where):
    sizes = [0, 3, 4, 5, 200, 300]
    base = hr.scenes_planar_noisy(seed=int(rng.integers(1 << 30)), n=300)[0]
    out = []
    for b in range(B):
        n = sizes[b % len(sizes)]
        out.append(special if b in where else (base["px1"][:n] + b, base["px2"][:n] + b))
    return out


def test_result_is_bit_identical_alone_and_anywhere_in_ragged_batches(gpu_ctx, scenes):
    import slamhip

    s = scenes[-2]
    special = (s["sc"]["px1"], s["sc"]["px2"])
    alone = slamhip.find_homography_batch([special], seed=5, ctx=gpu_ctx)
    assert alone[2][0, 0] > 100 and alone[2][0, 1] >= 0
    for B in (2, 17, 256):
        where = sorted({0, B // 2, B - 1})
        pairs = _ragged(np.random.default_rng(100 + B), B, special, where)
        H, masks, st = slamhip.find_homography_batch(pairs, seed=5, ctx=gpu_ctx)
        dec = slamhip.decompose_homography_batch(H, pairs, K, inliers=masks, ctx=gpu_ctx)
        for w in where:
            assert _bits(H[w], alone[0][0]) and np.array_equal(masks[w], alone[1][0]) and np.array_equal(st[w], alone[2][0]), (B, w)
            assert _bits(dec["pose_all"][w], dec["pose_all"][where[0]]) and np.array_equal(dec["stats"][w], dec["stats"][where[0]])
        for b, (a, _) in enumerate(pairs):
            if len(a) < 4:
                assert not H[b].any() and not masks[b].any() and st[b].tolist() == [0, -1, -1, 0] and dec["stats"][b].tolist() == [0, -1, 0, 0]
            else:
                assert st[b, 0] == masks[b].sum() and np.isfinite(H[b]).all()
    again = slamhip.find_homography_batch([special], seed=5, ctx=gpu_ctx)
    assert _bits(again[0], alone[0]) and np.array_equal(again[2], alone[2])            # run to run


def test_a_degenerate_or_empty_pair_changes_no_other_pair(gpu_ctx):
    import slamhip

    fam = {f"{s['family']}/{s['variant']}": s for f in ("duplicates", "collinear", "non_finite", "off_image") for s in ref.FAMILIES[f]()}
    base_sc = hr.scenes_planar_noisy(seed=11, n=250)[1]
    base = [(base_sc["px1"][: 50 + (b % 5) * 40] + b, base_sc["px2"][: 50 + (b % 5) * 40] + b) for b in range(32)]
    Es = np.tile(ref.essential_from_pose(base_sc["R"], base_sc["t"]), (32, 1))
    empty = (np.zeros((0, 2)), np.zeros((0, 2)))

    def run(pairs):
        H, masks, st = slamhip.find_homography_batch(pairs, 64, ctx=gpu_ctx)
        dec = slamhip.decompose_homography_batch(H, pairs, K, inliers=masks, ctx=gpu_ctx)
        off = np.r_[0, np.cumsum([len(p[0]) for p in pairs])]
        score, ratio = slamhip.model_scores_offsets(H, Es, np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs]), off, K,
                                                    ctx=gpu_ctx)
        assert np.isfinite(H).all() and np.isfinite(dec["pose_all"]).all() and np.isfinite(ratio).all()
        return H, masks, st, dec, score, ratio

    ref_run = None
    for where in (0, 15, 31):
        for name in ("duplicates/1distinct", "collinear/both", "non_finite/some", "off_image/1e150", None):
            pairs = list(base)
            pairs[where] = empty if name is None else (fam[name]["px1"], fam[name]["px2"])
            r = run(pairs)
            if ref_run is None:
                ref_run = run(base)
            for k in range(32):
                if k == where:
                    continue
                assert _bits(r[0][k], ref_run[0][k]) and np.array_equal(r[1][k], ref_run[1][k]) and np.array_equal(r[2][k], ref_run[2][k]), (where, name, k)
                assert _bits(r[3]["pose_all"][k], ref_run[3]["pose_all"][k]) and np.array_equal(r[3]["stats"][k], ref_run[3]["stats"][k])
                assert np.array_equal(r[4][k], ref_run[4][k]) and _bits(r[5][k], ref_run[5][k])


def test_bad_offsets_never_leave_the_arrays_and_are_counted(gpu_ctx):
    import slamhip

    sc = hr.scenes_planar_noisy(seed=32, n=300)[0]
    a, b = sc["px1"], sc["px2"]
    n = ctypes.c_int64(-1)
    gpu_ctx.lib.slam_index_errors(gpu_ctx.handle, ctypes.byref(n))     # clear
    off = np.array([-50, 100, 10 ** 6, 300], np.int32)                  # starts before 0; leaves the arrays; descends
    H, mask, st = slamhip.find_homography_offsets(a, b, off, 64, 3.0, 0, ctx=gpu_ctx)
    assert gpu_ctx.lib.slam_index_errors(gpu_ctx.handle, ctypes.byref(n)) == 0
    assert n.value == 3                                                 # three clamped pairs
    H0, m0, s0 = tw.ransac(a[:100], b[:100], 64, 3.0, 0)                # pair 0 shrank to [0, 100)
    H1, m1, s1 = tw.ransac(a[100:], b[100:], 64, 3.0, 0)                # pair 1 shrank to [100, 300)
    assert _bits(H[0], H0) and np.array_equal(mask[:100], m0) and np.array_equal(st[0], s0)
    assert _bits(H[1], H1) and np.array_equal(mask[100:], m1) and np.array_equal(st[1], s1)
    assert st[2].tolist() == [0, -1, -1, 0] and not H[2].any()          # pair 2 shrank to nothing
    dec = slamhip.decompose_homography_offsets(H, a, b, off, K, mask, ctx=gpu_ctx)
    score, _ = slamhip.model_scores_offsets(H, np.zeros((3, 9)), a, b, off, K, ctx=gpu_ctx)
    gpu_ctx.lib.slam_index_errors(gpu_ctx.handle, ctypes.byref(n))
    assert n.value == 6
    d0 = tw.decompose(a[:100], b[:100], K, H0, m0)
    assert _bits(dec["pose_all"][0], d0["pose_all"]) and np.array_equal(dec["stats"][0], d0["stats"]) and dec["stats"][2].tolist() == [0, -1, 0, 0]
    assert score[0, 0] == tw.model_score(a[:100], b[:100], K, H0, np.zeros(9))[0][0] and score[:, 1].tolist() == [0, 0, 0]
    H, mask, st = slamhip.find_homography_offsets(a, b, [50, 100, 280], 64, 3.0, 0, ctx=gpu_ctx)
    assert not mask[:50].any() and not mask[280:].any()                 # a table that leaves gaps is fine: entries outside are 0
    gpu_ctx.lib.slam_index_errors(gpu_ctx.handle, ctypes.byref(n))
    assert n.value == 0


# ------------------------------------------------------------------------------------------------ end to end
def _compose(s, ratio=0.45):
    """estimate_two_view_auto from the twins' pieces."""
    from oracle import oracle

    sc = s["sc"]
    score, r = tw.model_score(sc["px1"], sc["px2"], K, s["H"], s["E"])
    d = tw.decompose(sc["px1"], sc["px2"], K, s["H"], s["mask"])
    if r > ratio and d["stats"][1] != -1:
        return "H", r, d["pose"], s["mask"], d
    pose = oracle.tv_twin_recover_pose(s["E"], sc["px1"], sc["px2"], K)[0]
    return "E", r, pose, s["emask"], d


def test_estimate_two_view_auto_is_the_composition_of_the_twins(gpu_ctx, scenes):
    import slamhip

    for s in scenes:
        sc = s["sc"]
        r = slamhip.estimate_two_view_auto(sc["px1"], sc["px2"], K, ctx=gpu_ctx)
        model, ratio, pose, mask, d = _compose(s)
        print(f"{s['name']:28s} model {r['model']} R_H {r['ratio']:.4f} rotation_only {r['rotation_only']} ambiguous {r['ambiguous']} counts {r['counts']}")
        assert r["model"] == model and _bits(r["ratio"], ratio) and _bits(r["pose"], pose) and np.array_equal(r["inliers"], mask), s["name"]
        assert _bits(r["H"].reshape(9), s["H"]) and _bits(r["E"].reshape(9), s["E"])
        if model == "H":
            nc = d["stats"][3]
            assert _bits(r["candidates"], d["pose_all"][:nc]) and np.array_equal(r["counts"], d["count"][:nc])
            assert r["rotation_only"] == (d["stats"][1] == -2)
            assert r["ambiguous"] == (d["stats"][1] >= 0 and d["stats"][0] > 0 and d["stats"][2] >= 0.75 * d["stats"][0])
        else:
            assert len(r["candidates"]) == 0 and not r["rotation_only"] and not r["ambiguous"]
    by = {s["name"]: slamhip.estimate_two_view_auto(s["sc"]["px1"], s["sc"]["px2"], K, ctx=gpu_ctx) for s in scenes[:3]}
    t60, fr, rot = by["planar/tilt60"], by["planar/fronto"], by["pure_rotation/t0"]
    sc = scenes[1]["sc"]
    assert t60["model"] == "H" and not t60["ambiguous"] and np.linalg.norm(t60["pose"] - np.c_[sc["R"], sc["t"]]) < 1e-12      # the E path: 10.7 degrees off
    assert fr["model"] == "H" and fr["ambiguous"] and fr["counts"].tolist().count(200) == 2
    assert rot["model"] == "H" and rot["rotation_only"] and not rot["t"].any() and np.linalg.norm(rot["R"] - scenes[2]["sc"]["R"]) < 1e-13
    # the existing path is untouched: the E branch is verify_pairs' answer
    g = next(s for s in scenes if s["name"] == "general/clean")
    R, t, masks, _ = slamhip.verify_pairs([(g["sc"]["px1"], g["sc"]["px2"])], K, ctx=gpu_ctx)
    e = slamhip.estimate_two_view_auto(g["sc"]["px1"], g["sc"]["px2"], K, ctx=gpu_ctx)
    assert e["model"] == "E" and np.array_equal(e["R"], R[0]) and np.array_equal(e["t"], t[0]) and np.array_equal(e["inliers"], masks[0])


def test_verify_pairs_auto_on_64_mixed_pairs_equals_64_single_calls(gpu_ctx, scenes):
    import slamhip

    pairs = []
    for b in range(64):
        sc = scenes[b % len(scenes)]["sc"]
        n = (200, 150, 4, 3, 0, 77)[b % 6]
        pairs.append((sc["px1"][:n], sc["px2"][:n]))
    batch = slamhip.verify_pairs_auto(pairs, K, hypotheses=64, seed=3, ctx=gpu_ctx)
    assert len(batch) == 64 and {r["model"] for r in batch} == {"H", "E"}
    for b in range(64):
        one = slamhip.estimate_two_view_auto(pairs[b][0], pairs[b][1], K, hypotheses=64, seed=3, ctx=gpu_ctx)
        r = batch[b]
        assert one["model"] == r["model"] and _bits(one["ratio"], r["ratio"]) and _bits(one["pose"], r["pose"]), b
        assert np.array_equal(one["inliers"], r["inliers"]) and _bits(one["candidates"], r["candidates"]) and np.array_equal(one["counts"], r["counts"])
        assert one["rotation_only"] == r["rotation_only"] and one["ambiguous"] == r["ambiguous"] and np.array_equal(one["score"], r["score"])
        assert np.isfinite(r["pose"]).all()


# ------------------------------------------------------------------------------------------------ the batch amortises the launch
def test_a_batch_of_256_pairs_takes_less_than_256_single_calls(gpu_ctx):
    rng = np.random.default_rng(70)
    base = hr.scenes_planar_noisy(seed=70, n=200)[1]
    px1 = np.concatenate([base["px1"] + rng.normal(0, 0.2, (200, 2)) for _ in range(256)])
    px2 = np.concatenate([base["px2"] + rng.normal(0, 0.2, (200, 2)) for _ in range(256)])
    off = np.arange(257, dtype=np.int32) * 200
    d1, d2, do = gpu_ctx.upload(px1), gpu_ctx.upload(px2), gpu_ctx.upload(off)
    dH, dm, ds = gpu_ctx.malloc(256 * 72), gpu_ctx.malloc(len(px1)), gpu_ctx.malloc(256 * 16)
    lib, h = gpu_ctx.lib, gpu_ctx.handle

    def batch():
        assert lib.slam_hg_ransac_f64(h, 256, do.ptr, d1.ptr, d2.ptr, len(px1), 256, 3.0, 0, dH.ptr, dm.ptr, ds.ptr) == 0

    def singles():
        for b in range(256):
            assert lib.slam_hg_ransac_f64(h, 1, do.ptr + 4 * b, d1.ptr, d2.ptr, len(px1), 256, 3.0, 0, dH.ptr + 72 * b, dm.ptr, ds.ptr + 16 * b) == 0

    def timed(fn):
        gpu_ctx.timer_start()
        fn()
        return gpu_ctx.timer_stop()

    try:
        timed(batch), timed(singles)                      # warm-up
        tb = np.median([timed(batch) for _ in range(5)])
        Hb = dH.download(np.float64, (256, 9))
        ts = np.median([timed(singles) for _ in range(5)])
        print(f"256 pairs x 200 matches, H = 256: batch {tb:.3f} ms, 256 single calls {ts:.3f} ms")
        assert np.array_equal(dH.download(np.float64, (256, 9)), Hb)
        assert tb < ts
    finally:
        for o in (d1, d2, do, dH, dm, ds):
            o.free()
