"""Sim(3) refinement by reprojection error (slam_sim3_optimize_f64) without a GPU: the host twin of csrc/sim3_opt.hip
(tests/sim3_opt_twin.py: the kernel file's own routines compiled for the host, the summation order and the sequential
Levenberg-Marquardt restated) against the numpy statement on another route (tests/sim3_opt_ref.py: central-difference
Jacobians, numpy sums, np.linalg.solve), against planted similarities, against a sanitised stand-alone build of itself, and
the C entry's argument checks.  tests/test_sim3_opt_gpu.py then holds the device to the twin bit for bit.

Every model tolerance is BOUNDS below: 16 x the larger of numpy's and the twin's own error for that quantity and scene, as
tools/sim3_opt_edges.py measured them into profiles/sim3_opt_edges.log (the figures are quoted beside each bound; the factor
16, four bits, allows for another libm or BLAS).  The truth of an exact scene is the planted similarity, the truth of a
noisy scene the minimiser next to numpy's model (sim3_opt_ref.polished).  The scenes' seeds are fixed so that the numpy
statement alone keeps no planted outlier and at least 90 % of the planted inliers on every one of them."""
import ctypes
import os
import re

import numpy as np
import pytest

import sim3_opt_ref as ref
import sim3_opt_twin as tw

K = ref.EUROC
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUANTITIES = ("scale", "rotation", "translation")
JACOBIAN = 1.751e-10      # profiles/sim3_opt_edges.log: "worst |dJ| / max |J| over 200 pairs: 1.751e-10"

BOUNDS = {
    ("exact_s0.5_o0", "scale"): 16 * 6.661e-16,                # numpy 6.661e-16 twin 0.000e+00
    ("exact_s0.5_o0", "rotation"): 16 * 3.152e-16,             # numpy 3.152e-16 twin 3.147e-16
    ("exact_s0.5_o0", "translation"): 16 * 2.429e-16,          # numpy 2.429e-16 twin 1.923e-16
    ("exact_s0.5_o10000", "scale"): 16 * 6.883e-14,            # numpy 6.883e-14 twin 6.861e-14
    ("exact_s0.5_o10000", "rotation"): 16 * 2.759e-14,         # numpy 2.758e-14 twin 2.759e-14
    ("exact_s0.5_o10000", "translation"): 16 * 7.126e-13,      # numpy 7.126e-13 twin 7.126e-13
    ("exact_s1_o0", "scale"): 16 * 2.220e-16,                  # numpy 1.110e-16 twin 2.220e-16
    ("exact_s1_o0", "rotation"): 16 * 2.531e-16,               # numpy 6.206e-17 twin 2.531e-16
    ("exact_s1_o0", "translation"): 16 * 2.359e-16,            # numpy 4.994e-17 twin 2.359e-16
    ("exact_s1_o10000", "scale"): 16 * 4.508e-14,              # numpy 4.508e-14 twin 4.374e-14
    ("exact_s1_o10000", "rotation"): 16 * 3.931e-14,           # numpy 3.930e-14 twin 3.931e-14
    ("exact_s1_o10000", "translation"): 16 * 4.090e-13,        # numpy 4.088e-13 twin 4.090e-13
    ("exact_s2_o0", "scale"): 16 * 1.332e-15,                  # numpy 0.000e+00 twin 1.332e-15
    ("exact_s2_o0", "rotation"): 16 * 4.839e-16,               # numpy 4.791e-16 twin 4.839e-16
    ("exact_s2_o0", "translation"): 16 * 1.993e-16,            # numpy 1.993e-16 twin 1.044e-16
    ("exact_s2_o10000", "scale"): 16 * 1.488e-14,              # numpy 1.488e-14 twin 7.994e-15
    ("exact_s2_o10000", "rotation"): 16 * 3.835e-14,           # numpy 3.835e-14 twin 3.833e-14
    ("exact_s2_o10000", "translation"): 16 * 3.461e-12,        # numpy 3.461e-12 twin 3.461e-12
    ("noisy_s0.5_out0", "scale"): 16 * 9.057e-13,              # numpy 5.458e-13 twin 9.057e-13
    ("noisy_s0.5_out0", "rotation"): 16 * 4.805e-14,           # numpy 4.805e-14 twin 4.426e-14
    ("noisy_s0.5_out0", "translation"): 16 * 2.010e-13,        # numpy 1.004e-13 twin 2.010e-13
    ("noisy_s0.5_out30", "scale"): 16 * 1.212e-12,             # numpy 4.023e-13 twin 1.212e-12
    ("noisy_s0.5_out30", "rotation"): 16 * 1.007e-13,          # numpy 1.007e-13 twin 2.737e-14
    ("noisy_s0.5_out30", "translation"): 16 * 2.098e-13,       # numpy 1.925e-13 twin 2.098e-13
    ("noisy_s1_out0", "scale"): 16 * 2.072e-10,                # numpy 2.072e-10 twin 7.837e-12
    ("noisy_s1_out0", "rotation"): 16 * 9.149e-12,             # numpy 9.149e-12 twin 8.954e-14
    ("noisy_s1_out0", "translation"): 16 * 4.979e-11,          # numpy 4.979e-11 twin 1.377e-12
    ("noisy_s1_out30", "scale"): 16 * 1.194e-11,               # numpy 4.594e-12 twin 1.194e-11
    ("noisy_s1_out30", "rotation"): 16 * 3.563e-13,            # numpy 1.038e-13 twin 3.563e-13
    ("noisy_s1_out30", "translation"): 16 * 2.201e-12,         # numpy 7.132e-13 twin 2.201e-12
    ("noisy_s2_out0", "scale"): 16 * 3.556e-11,                # numpy 1.121e-11 twin 3.556e-11
    ("noisy_s2_out0", "rotation"): 16 * 5.662e-13,             # numpy 5.662e-13 twin 4.612e-13
    ("noisy_s2_out0", "translation"): 16 * 8.969e-12,          # numpy 7.615e-12 twin 8.969e-12
    ("noisy_s2_out30", "scale"): 16 * 1.324e-11,               # numpy 6.056e-12 twin 1.324e-11
    ("noisy_s2_out30", "rotation"): 16 * 4.101e-13,            # numpy 4.101e-13 twin 1.068e-13
    ("noisy_s2_out30", "translation"): 16 * 4.477e-12,         # numpy 4.477e-12 twin 2.904e-12
    ("noisy_sigma_out30", "scale"): 16 * 2.391e-11,            # numpy 2.092e-11 twin 2.391e-11
    ("noisy_sigma_out30", "rotation"): 16 * 4.214e-13,         # numpy 2.671e-13 twin 4.214e-13
    ("noisy_sigma_out30", "translation"): 16 * 4.301e-12,      # numpy 3.758e-12 twin 4.301e-12
    ("ransac_out30", "scale"): 16 * 1.464e-10,                 # numpy 1.464e-10 twin 1.338e-11
    ("ransac_out30", "rotation"): 16 * 5.095e-12,              # numpy 5.095e-12 twin 2.893e-13
    ("ransac_out30", "translation"): 16 * 3.524e-11,           # numpy 3.524e-11 twin 1.253e-12
    ("ransac_out0", "scale"): 16 * 4.776e-12,                  # numpy 2.828e-12 twin 4.776e-12
    ("ransac_out0", "rotation"): 16 * 1.936e-13,               # numpy 1.936e-13 twin 5.423e-14
    ("ransac_out0", "translation"): 16 * 7.868e-13,            # numpy 7.868e-13 twin 7.667e-13
}


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


def _twin(sc, start, **kw):
    return tw.optimize(sc["X1"], sc["X2"], sc["px1"], sc["px2"], start, K, sc.get("sigma2"), **kw)


@pytest.fixture(scope="module")
def scenes():
    return ref.scene_list()


@pytest.fixture(scope="module")
def results(scenes):
    """name -> (numpy's result, the twin's result): computed once, shared, never changed."""
    return {name: (ref.optimize(sc, start), _twin(sc, start)) for name, (sc, start, _) in scenes.items()}


# ------------------------------------------------------------------------------------------------ the pieces
def test_analytic_jacobian_is_the_central_difference_of_the_twins_residual(scenes):
    worst = 0.0
    for name in ("noisy_s1_out30", "noisy_s0.5_out0", "noisy_sigma_out30"):
        sc, start, _ = scenes[name]
        for i in range(0, 200, 5):
            p = np.concatenate([sc["X1"][i], sc["X2"][i], sc["px1"][i], sc["px2"][i], sc["sigma2"][i]])
            for fix in (False, True):
                J = tw.pair(start, p, K, fix)[3]
                Jn = np.zeros((4, 7))
                for k in range(6 if fix else 7):
                    x = np.zeros(7)
                    x[k] = ref.STEP
                    Jn[:, k] = (tw.pair(tw.retract(start, x), p, K)[0] - tw.pair(tw.retract(start, -x), p, K)[0]) / (2 * ref.STEP)
                assert not fix or (J[:, 6] == 0).all()
                worst = max(worst, float(np.abs(J - Jn).max() / np.abs(J).max()))
    print(f"worst |dJ| / max |J|: {worst:.3e}")
    # a central difference of step h = 1e-6 on residuals of up to 1e3 px carries 1e3 eps / h = 2e-7 px of rounding against
    # entries of max |J| >= fx = 458: 5e-10 relative, and its truncation (h^2 / 6 of the third derivative) is below that
    assert worst <= 16 * JACOBIAN


def test_retraction_is_a_rotation_a_positive_scale_and_numpys_chart(scenes):
    model = scenes["exact_s2_o0"][0]["model"]
    rng = np.random.default_rng(5)
    for size in (1e-3, 0.3, 3.0, 50.0):
        x = rng.normal(size=7) * size
        out = tw.retract(model, x)
        s, R, t = ref.split(out)
        # every entry of R_d R is a sum of three products of entries below 1: three roundings each, 16 x
        assert np.abs(R.T @ R - np.eye(3)).max() <= 16 * 3 * 2.3e-16 and abs(np.linalg.det(R) - 1) <= 16 * 3 * 2.3e-16 and s > 0
        assert np.abs(out - ref.retract(model, x)).max() <= 16 * 2.3e-16 * (1 + np.abs(out).max()) * 8
    assert _bits(tw.retract(model, np.zeros(7)), model)


def test_the_sums_are_numpys_sums_in_another_order(scenes):
    sc, start, _ = scenes["noisy_s1_out30"]
    act = np.random.default_rng(1).random(200) < 0.8
    for delta in (0.0, np.sqrt(10.0)):
        s = tw.linearize(sc["X1"], sc["X2"], sc["px1"], sc["px2"], start, K, delta, sc["sigma2"], act)
        H, b, F = ref.linearize(start, sc, K, act, delta)
        Ht = np.zeros((7, 7))
        Ht[np.triu_indices(7)] = s[:28]
        Ht = Ht + np.triu(Ht, 1).T
        # numpy's Jacobians are central differences (JACOBIAN of max |J|, the test above): H = J^T J agrees to twice that of its
        # largest entry, b = J^T e to that of sqrt(max H) * |e| with |e|^2 the plain cost
        F0 = ref.linearize(start, sc, K, act, 0.0)[2]
        assert np.abs(Ht - H).max() <= 16 * 2 * JACOBIAN * np.abs(H).max()
        assert np.abs(s[28:35] - b).max() <= 16 * JACOBIAN * np.sqrt(np.abs(H).max() * F0)
        assert abs(s[35] - F) <= 16 * 200 * 2.3e-16 * F                 # a sum of 200 positive terms in another order


# ------------------------------------------------------------------------------------------------ twin against numpy
def test_twin_against_numpy_on_every_scene(scenes, results):
    for name, (sc, start, kind) in scenes.items():
        r, (m, mask, chi2, st) = results[name]
        assert np.array_equal(mask, r["mask"]) and st[0] == r["stats"][0] == mask.sum() and st[2] == r["stats"][2], name
        assert not (st[3] & ref.REJECTED) and np.array_equal(np.isnan(chi2[:, 0]), ~r["start_active"])
        truth = sc["model"] if kind == "exact" else ref.polished(sc, r["model"], r["fitted"])
        for who, model in (("numpy", r["model"]), ("twin", m)):
            for q, v in zip(QUANTITIES, ref.model_errors(model, truth)):
                print(f"{name} {q} {who}: {v:.3e} (bound {BOUNDS[(name, q)]:.3e})")
                assert v <= BOUNDS[(name, q)], (name, q, who, v)


def test_conditions_on_the_scenes_hold_on_the_numpy_statement_alone(scenes, results):
    kinds = [kind for _, _, kind in scenes.values()]
    assert kinds.count("noisy") >= 8 and kinds.count("exact") == 6
    for name, (sc, start, kind) in scenes.items():
        r = results[name][0]
        ti = sc["true_inlier"]
        assert not r["mask"][~ti].any(), name                           # no planted outlier survives
        assert r["mask"][ti].mean() >= 0.9, name
        if kind == "noisy":
            delta = np.sqrt(ref.TH2)
            assert ref.cost(r["model"], sc, K, r["start_active"], delta)[0] < ref.cost(start, sc, K, r["start_active"], delta)[0], name
            assert (~ti).sum() == 0 or 40 <= (~ti).sum() <= 80          # "30 %" of 200


def test_exact_scenes_converge_to_the_planted_similarity(scenes, results):
    seen = set()
    for name, (sc, start, kind) in scenes.items():
        if kind != "exact":
            continue
        m, mask, chi2, st = results[name][1]
        seen.add((float(sc["model"][12]), "o10000" in name))
        assert mask.all() and st[0] == 200 and st[2] == 0
        assert max(ref.model_errors(start, sc["model"])) > 1e-3         # the start was not the answer
        for q, v in zip(QUANTITIES, ref.model_errors(m, sc["model"])):
            assert v <= BOUNDS[(name, q)], (name, q, v)
    assert seen == {(s, o) for s in (0.5, 1.0, 2.0) for o in (False, True)}


# ------------------------------------------------------------------------------------------------ the contract
def test_fix_scale_returns_the_scale_bit_for_bit(scenes):
    for name in ("noisy_s2_out30", "exact_s0.5_o0", "ransac_out30"):
        sc, start, _ = scenes[name]
        start = start.copy()
        start[12] = start[12] * (1 + 2.0 ** -30)
        m, mask, chi2, st = _twin(sc, start, fix_scale=True)
        assert m[12].tobytes() == start[12].tobytes() and st[1] > 0 and not _bits(m[:12], start[:12]), name
        r = ref.optimize(sc, start, fix_scale=True)
        assert r["model"][12] == start[12] and np.array_equal(r["mask"], mask)


def _good(n, seed=8):
    sc = ref.make_scene(np.random.default_rng(seed), n, 1.1, 0.5)
    return sc, ref.moved(np.random.default_rng(seed + 1), sc["model"])


def test_a_rejected_candidate_returns_its_input_bit_for_bit():
    sc, start = _good(9)                                                # 9 good pairs, min_pairs 10
    m, mask, chi2, st = _twin(sc, start)
    assert _bits(m, start) and not mask.any() and st[0] == 0 and st[3] & ref.REJECTED and np.isnan(chi2).all()
    assert ref.optimize(sc, start)["stats"][3] & ref.REJECTED
    m, mask, chi2, st = _twin(sc, start, min_pairs=9)                   # the same nine with min_pairs 9: refined
    assert st[0] == 9 and mask.all() and not (st[3] & ref.REJECTED) and not _bits(m, start)
    sc, start = _good(10)                                               # 10 good pairs: accepted ...
    m, mask, chi2, st = _twin(sc, start)
    assert st[0] == 10 and mask.all()
    sc["px2"][4] += [30.0, -40.0]                                       # ... until one is pushed past the gate
    m, mask, chi2, st = _twin(sc, start)
    r = ref.optimize(sc, start)
    assert _bits(m, start) and not mask.any() and st[0] == 0 and st[2] == 1 and st[3] & ref.REJECTED
    assert r["stats"][2] == 1 and r["stats"][3] & ref.REJECTED and np.array_equal(r["model"], start)


def test_invalid_models_and_non_finite_pairs_are_data(scenes):
    sc, start, _ = scenes["noisy_s1_out0"]
    for k, v in ((0, np.nan), (7, np.inf), (12, 0.0), (12, -1.0), (12, np.nan)):
        bad = start.copy()
        bad[k] = v
        m, mask, chi2, st = _twin(sc, bad)
        assert np.array_equal(m, ref.base.IDENTITY) and not mask.any() and st.tolist() == [0, 0, 0, 3] and np.isnan(chi2).all()
        assert ref.optimize(sc, bad)["stats"].tolist() == [0, 0, 0, 3]
    clean = _twin(sc, start)
    d = {k: sc[k].copy() for k in ("X1", "X2", "px1", "px2", "sigma2")}
    d["X1"][3, 1] = np.nan; d["X2"][10, 2] = -d["X2"][10, 2]; d["px1"][20, 0] = np.inf; d["sigma2"][30, 1] = 0.0
    d["sigma2"][40, 0] = np.nan; d["X1"][50, 2] = 0.0; d["px2"][60, 1] = -np.inf; d["sigma2"][70, 0] = -1.0
    dead = [3, 10, 20, 30, 40, 50, 60, 70]
    m, mask, chi2, st = _twin(d, start)
    r = ref.optimize(d, start)
    assert np.isfinite(m).all() and not mask[dead].any() and np.isnan(chi2[dead]).all() and np.isfinite(np.delete(chi2, dead, 0)).all()
    assert np.array_equal(mask, r["mask"]) and st[0] == r["stats"][0] and st[2] == r["stats"][2]
    assert np.array_equal(np.delete(mask, dead), np.delete(clean[1], dead))          # the other pairs are judged as without them
    empty = {k: v[:0] for k, v in d.items()}
    m, mask, chi2, st = _twin(empty, start)
    assert _bits(m, start) and st.tolist() == [0, 0, 0, ref.REJECTED | ref.STALLED] and len(mask) == 0


def test_extreme_finite_data_gives_a_finite_model_and_a_consistent_vote():
    for name, (sc, start) in ref.extreme_cases().items():
        for fix in (False, True):
            m, mask, chi2, st = _twin(sc, start, fix_scale=fix)
            print(name, fix, st)
            assert np.isfinite(m).all() and m[12] > 0 and st[0] == mask.sum(), name
            assert (st[3] & ref.REJECTED and _bits(m, start) and not mask.any()) or (not st[3] & ref.REJECTED and st[0] >= 10), name
            with np.errstate(all="ignore"):
                assert (chi2[mask] <= ref.TH2).all(), name


def test_zero_iterations_only_classify(scenes):
    sc, start, _ = scenes["noisy_s1_out30"]
    m, mask, chi2, st = _twin(sc, start, iterations=(0, 0, 0))
    c, front = ref.chi2(start, sc, K)
    assert _bits(m, start) and st[1] == 0 and np.array_equal(mask, (c <= ref.TH2).all(1) & front) and st[0] == mask.sum()


def test_the_sanitised_program_agrees_with_the_library_bit_for_bit(scenes):
    for name, kw in (("noisy_sigma_out30", {}), ("ransac_out30", dict(fix_scale=True)), ("exact_s0.5_o10000", dict(iterations=(3, 4, 2)))):
        sc, start, _ = scenes[name]
        a = _twin(sc, start, **kw)
        b = tw.san_optimize(sc["X1"], sc["X2"], sc["px1"], sc["px2"], start, K, sc["sigma2"], **kw)
        assert _bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and _bits(a[2], b[2]) and a[3].tolist() == b[3].tolist(), name
    sc, start = _good(9)
    sc["X1"][2, 0] = np.nan
    a, b = _twin(sc, start), tw.san_optimize(sc["X1"], sc["X2"], sc["px1"], sc["px2"], start, K)
    assert _bits(a[0], b[0]) and _bits(a[2], b[2]) and a[3].tolist() == b[3].tolist()
    e = np.zeros((0, 3))
    a, b = tw.optimize(e, e, e[:, :2], e[:, :2], start, K), tw.san_optimize(e, e, e[:, :2], e[:, :2], start, K)
    assert _bits(a[0], b[0]) and a[3].tolist() == b[3].tolist()


# ------------------------------------------------------------------------------------------------ ABI and arguments
def test_abi_table_matches_the_header_and_the_stage_is_stated(built):
    from slamhip import _lib

    header = " ".join(open(os.path.join(ROOT, "include", "slamhip.h")).read().split())
    decl = re.search(r"SLAM_API int slam_sim3_optimize_f64\((.*?)\);", header).group(1)
    restype, argtypes = _lib.SIGNATURES["slam_sim3_optimize_f64"]
    kinds = []
    for a in decl.split(","):
        a = a.strip()
        kinds.append(ctypes.c_void_p if "*" in a else {"int64_t": ctypes.c_int64, "double": ctypes.c_double, "int": ctypes.c_int}[a.split()[0]])
    assert restype is ctypes.c_int and argtypes == kinds and len(kinds) == 24
    assert getattr(_lib.load(), "slam_sim3_optimize_f64").argtypes == argtypes
    assert "#define SLAM_SIM3_OPT_STAGE 512" in header
    src = open(os.path.join(ROOT, "slam-experiments_amd", "csrc", "sim3_opt.hip")).read()
    assert "#define SO_STAGE 512" in src and "sim3_opt.hip" in open(os.path.join(ROOT, "slam-experiments_amd", "csrc", "Makefile")).read()


def test_argument_errors_are_refused_without_a_device(built):
    """SLAM_ERR_INVALID comes back before any device call, so these run where there is no GPU; the handle is never dereferenced
    (a bad argument is found first)."""
    from slamhip import _lib

    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)

    def call(**kw):
        a = dict(ctx=p, B=1, off=p, X1=p, X2=p, px1=p, px2=p, M=4, sg=None, mi=p, fx=458.0, fy=457.0, cx=367.0, cy=248.0, th2=10.0, it0=5,
                 it_bad=10, it_clean=5, min_pairs=10, fix=0, mo=p, inl=p, chi=p, st=p)
        a.update(kw)
        return lib.slam_sim3_optimize_f64(*a.values())

    for kw in (dict(ctx=None), dict(B=-1), dict(B=65536), dict(M=-1), dict(M=(1 << 28) + 1), dict(th2=0.0), dict(th2=-1.0), dict(th2=np.inf),
               dict(th2=np.nan), dict(it0=-1), dict(it_bad=-1), dict(it_clean=-1), dict(it_bad=1001), dict(min_pairs=0), dict(min_pairs=-3),
               dict(off=None), dict(X1=None), dict(X2=None), dict(px1=None), dict(px2=None), dict(mi=None), dict(mo=None), dict(inl=None),
               dict(chi=None), dict(st=None), dict(fx=0.0), dict(fy=np.nan), dict(cx=np.inf)):
        assert call(**kw) == _lib.SLAM_ERR_INVALID, kw
        assert lib.slam_last_error()


def test_python_layer_checks_and_the_inverse_form(built):
    import slamhip

    sc, start = _good(12)
    for kw in (dict(th2=0.0), dict(iterations=(5, 10)), dict(iterations=(5, -1, 5)), dict(min_pairs=0)):
        with pytest.raises(ValueError):
            slamhip.optimize_sim3_offsets(sc["X1"], sc["X2"], sc["px1"], sc["px2"], [0, 12], start, K, **kw)
    with pytest.raises(ValueError):
        slamhip.optimize_sim3_offsets(sc["X1"], sc["X2"], sc["px1"][:5], sc["px2"], [0, 12], start, K)
    with pytest.raises(ValueError):
        slamhip.optimize_sim3_offsets(sc["X1"], sc["X2"], sc["px1"], sc["px2"], [0, 12], np.zeros((2, 13)), K)
    out = slamhip.optimize_sim3_offsets(sc["X1"][:0], sc["X2"][:0], sc["px1"][:0], sc["px2"][:0], [0], np.zeros((0, 13)), K)
    assert out[0].shape == (0,) and out[4].shape == (0, 4)
    s, R, t = ref.split(sc["model"])
    S12 = slamhip.sim3_to_s12(sc["model"])
    X2 = s * (sc["X1"] @ R.T) + t
    assert S12.shape == (3, 4) and np.abs(X2 @ S12[:, :3].T + S12[:, 3] - sc["X1"]).max() <= 16 * 2.3e-16 * 8 * np.abs(X2).max()
    assert np.array_equal(slamhip.sim3_to_s12((s, R, t)), S12) and slamhip.sim3_to_s12(np.stack([sc["model"]] * 3)).shape == (3, 3, 4)
    with pytest.raises(ValueError):
        slamhip.sim3_to_s12(np.zeros(13))
    from backend import Backend
    assert callable(Backend.compute_sim3)
