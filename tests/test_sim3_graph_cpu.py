"""CPU suite of the Sim(3) pose-graph optimisation: the numpy reference of tests/sim3_graph_ref.py checks itself against an
80-digit truth and against the SE(3) reference, the yardsticks the GPU tests of tests/test_sim3_graph_gpu.py import are
measured here (constants below, held by honest(): each bounds its measurement and is padded by at most 4x), the host twin of
the kernel file's per-edge routines is held to the truth, and the product code that needs no GPU is exercised."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_sim3_graph_truth as MT  # noqa: E402
import pose_graph_ref as P  # noqa: E402
import sim3_graph_ref as R  # noqa: E402
import sim3_graph_twin as TW  # noqa: E402
from pose_graph_truth import BAND_CUTS, band_of  # noqa: E402
from test_pose_graph_cpu import LIN_MARGIN, honest, rel  # noqa: E402

# ---- yardsticks ------------------------------------------------------------------------------------------------------------
# (a) the numpy reference (closed forms, f64) against the 80-digit truth of tests/golden/sim3_graph_truth.npz, per band of the
#     residual's rotation angle [0, 1e-3) [1e-3, 0.05) [0.05, 0.2) [0.2, 0.5) [0.5, 2.5) [2.5, 3.1]: cost, grad (both ends),
#     Hdiag (both ends) and W per edge, each relative to that edge's own largest magnitude, largest over Huber off and on.
#     "general": the four families with translation information; "rot_scale_only" stands alone, as rot_only does in
#     tests/test_pose_graph_edges_cpu.py.  Measured by test_yardstick_truth (python tests/test_sim3_graph_cpu.py prints them).
YARD_TRUTH = {
    "general": {
        "cost": (2.5e-11, 2.7e-12, 7.8e-13, 9.2e-12, 7.6e-13, 1.5e-12),
        "grad": (5.5e-10, 9.2e-11, 1.1e-12, 1.7e-11, 2.1e-10, 9.4e-13),
        "Hdiag": (4.4e-12, 1.1e-13, 4.2e-14, 2.5e-12, 3.7e-13, 4.8e-14),
        "W": (9.4e-12, 1.5e-12, 7.6e-14, 1.1e-11, 3.0e-12, 2.7e-13),
    },
    "rot_scale_only": {
        "cost": (2.4e-15, 5.9e-16, 7.1e-16, 1.1e-15, 8.4e-16, 6.4e-16),
        "grad": (4.5e-15, 8.3e-15, 6.2e-16, 9.4e-16, 7.3e-16, 2.1e-14),
        "Hdiag": (3.5e-15, 1.9e-15, 4.9e-15, 5.8e-15, 1.5e-15, 1.2e-14),
        "W": (1.7e-15, 9.8e-16, 4.2e-15, 5.8e-15, 9.1e-16, 1.2e-14),
    },
}
# Measured values behind the constants (python tests/test_sim3_graph_cpu.py prints them; each constant is 1.5x its measurement,
# rounded to two digits, and honest() holds it between 1x and 4x):
#   YARD_TRUTH general cost: 1.7e-11 1.8e-12 5.2e-13 6.1e-12 5.1e-13 1.0e-12
#   YARD_TRUTH general grad: 3.7e-10 6.1e-11 7.1e-13 1.2e-11 1.4e-10 6.2e-13
#   YARD_TRUTH general Hdiag: 2.9e-12 7.4e-14 2.8e-14 1.7e-12 2.4e-13 3.2e-14
#   YARD_TRUTH general W: 6.3e-12 1.0e-12 5.0e-14 7.1e-12 2.0e-12 1.8e-13
#   YARD_TRUTH rot_scale_only cost: 1.6e-15 3.9e-16 4.7e-16 7.2e-16 5.6e-16 4.3e-16
#   YARD_TRUTH rot_scale_only grad: 3.0e-15 5.5e-15 4.1e-16 6.3e-16 4.9e-16 1.4e-14
#   YARD_TRUTH rot_scale_only Hdiag: 2.4e-15 1.3e-15 3.3e-15 3.8e-15 1.0e-15 8.1e-15
#   YARD_TRUTH rot_scale_only W: 1.1e-15 6.5e-16 2.8e-15 3.8e-15 6.1e-16 8.1e-15
#   YARD_LIN: cost 5.1e-16, grad 7.9e-15, Hdiag 5.6e-15, W 2.2e-14;  YARD_HMUL: 4.6e-15
#   YARD_SOLVE drift_loop: chi2 4.8e-15, rotation 1.8e-13, translation 1.6e-12, log_scale 2.6e-12
#   YARD_SOLVE hub: chi2 3.4e-11, rotation 1.5e-09, translation 6.5e-10, log_scale 2.9e-10
#   YARD_SOLVE sphere_s1: chi2 5.3e-08, rotation 4.7e-08, translation 1.2e-08, log_scale 7.3e-08
ROUNDING = 2.0 ** -53        # no f64 result is held tighter than its own rounding
TRUTH_MARGIN = LIN_MARGIN    # 16x: the margin of tests/test_pose_graph_edges_cpu.py
# (b) linearisation on the scenes: the reference's closed-form path against its series path, Huber off and on
YARD_LIN = {"cost": 7.7e-16, "grad": 1.2e-14, "Hdiag": 8.4e-15, "W": 3.3e-14}
# scipy's CSR product against a dense numpy product of the same matrix (relative to the largest entry of the result)
YARD_HMUL = 6.9e-15
# (c) solve, per scene: reference-PCG LM against reference-direct LM (relative chi2, radians, fraction of the extent, |log s|)
#     after SOLVE_ITERATIONS iterations, a count inside the descent (test_solve_iterations_end_in_the_descent holds each to a
#     chi2 that still falls by more than 1e-6 of itself).  drift_loop is at its optimum after 8 iterations; from there on a
#     trial is accepted or turned down on the sign of a chi2 difference of rounding size, two correct implementations take
#     different branches (the reference itself: 13 iterations and 29 trials), and a gap between two such runs measures that
#     coin, not the arithmetic: 6 is the last count that falls by 1e-6.  sphere_s1 (2500 poses) is still falling at 15, but
#     from its fourth iteration on the reference PCG runs into PCG_MAX_ITER = 500 and the gap would measure the cap: 3 is the
#     last count at which every solve met PCG_TOL (and its direct solves stay at seconds).  hub: 5, for its slow direct solve.
SOLVE_ITERATIONS = {"drift_loop": 6, "hub": 5, "sphere_s1": 3}
YARD_SOLVE = {
    "drift_loop": {"chi2": 7.3e-15, "rotation": 2.7e-13, "translation": 2.4e-12, "log_scale": 4.0e-12},
    "hub": {"chi2": 5.1e-11, "rotation": 2.2e-09, "translation": 9.7e-10, "log_scale": 4.4e-10},
    "sphere_s1": {"chi2": 7.9e-08, "rotation": 7.0e-08, "translation": 1.8e-08, "log_scale": 1.1e-07},
}
# (d) mutation check: factors by which a reference with the sign of Ad's -t column flipped / without J_j's Jl^-1 (0; t_D)
#     column misses the truth's W or Hdiag, over the largest general yardstick of W (measured 1.9e12 and 1.9e11; asserted >= 1e6)
MUTATION_FACTOR = 1e6
# (e) reduction to SE(3): fix_scale, every s = 1, Omega = diag(Omega_6, w_sigma): the 6x6 corner of every block against
#     pose_graph_ref.linearize, in ulps of the largest entry of the quantity (observed 0: the same operations)
REDUCTION_ULPS = 4
GROUPS = {"general": ("diag", "spd1", "spd1e4", "spd1e8"), "rot_scale_only": ("rot_scale_only",)}
QUANTITIES = ("cost", "grad", "Hdiag", "W")


@functools.lru_cache(maxsize=None)
def fixture():
    return MT.load_fixture()


@functools.lru_cache(maxsize=None)
def scene(name):
    return R.SMALL_SCENES[name]()


@functools.lru_cache(maxsize=None)
def solved(name, solver):
    s = scene(name)
    return R.optimize(s.init, s.edges, s.meas, s.info, s.fixed, iterations=SOLVE_ITERATIONS[name], solver=solver)


def bands(fx):
    return np.array([band_of(a) for a in np.linalg.norm(fx["r"][:, :3], axis=1)])


def truth_of(fx, fam, hub):
    k = f"_{fam}{hub}"
    return dict(cost=fx["cost" + k], grad=np.concatenate([fx["bi" + k], fx["bj" + k]], 1), Hdiag=np.stack([fx["Hii" + k], fx["Hjj" + k]], 1),
                W=fx["W" + k])


def blocks_from_jacobians(r, Ji, Jj, Om, delta):
    chi2 = np.einsum("ea,eab,eb->e", r, Om, r)
    rho, w = P.robust(chi2, delta)
    wI = w[:, None, None] * Om
    Or = np.einsum("eab,eb->ea", wI, r)
    T_ = lambda A: np.swapaxes(A, 1, 2)
    return dict(cost=rho, grad=np.concatenate([np.einsum("eba,eb->ea", Ji, Or), np.einsum("eba,eb->ea", Jj, Or)], 1),
                Hdiag=np.stack([T_(Ji) @ wI @ Ji, T_(Jj) @ wI @ Jj], 1), W=T_(Ji) @ wI @ Jj)


def reference_edges(fx, fam, delta, mutate=None):
    N = len(fx["r"])
    sims = np.concatenate([fx["Si"], fx["Sj"]])
    edges = np.stack([np.arange(N), N + np.arange(N)], 1)
    r, Ji, Jj = R.jacobians(sims, edges, fx["Z"])
    if mutate:
        _, A, D = R.residuals(sims, edges, fx["Z"])
        Ad = R.adjoint(A)
        if mutate == "ad_t_sign":
            Ad[:, 3:6, 6] = -Ad[:, 3:6, 6]
        if mutate == "drop_scale_column":
            Jj[:, :6, 6] = 0.0
        Ji = -Jj @ Ad
    return blocks_from_jacobians(r, Ji, Jj, fx["info_" + fam], delta)


def twin_edges(fx, fam, delta, san=False):
    o = (TW.san_edges if san else TW.edges)(fx["Si"], fx["Sj"], fx["Z"], fx["info_" + fam], delta)
    Hi, bi = TW.full_blocks(o["Di"])
    Hj, bj = TW.full_blocks(o["Dj"])
    assert not o["why"].any()
    return dict(cost=o["rho"], grad=np.concatenate([bi, bj], 1), Hdiag=np.stack([Hi, Hj], 1), W=o["W"])


def edge_errors(got, truth):
    """per edge, each quantity's largest difference relative to the edge's own largest magnitude of that quantity"""
    out = {}
    for q in QUANTITIES:
        g, t = got[q].reshape(len(truth[q]), -1), truth[q].reshape(len(truth[q]), -1)
        out[q] = np.abs(g - t).max(1) / np.maximum(np.abs(t).max(1), 1e-300)
    return out


def band_errors(fx, edges_fn):
    """{group: {quantity: [6]}}: the largest per-edge error of edges_fn(fx, family, delta) per band, over families and Huber"""
    b = bands(fx)
    out = {g: {q: np.zeros(len(BAND_CUTS) + 1) for q in QUANTITIES} for g in GROUPS}
    for g, fams in GROUPS.items():
        for fam in fams:
            for hub, delta in (("", 0.0), ("_huber", float(fx["delta_" + fam]))):
                err = edge_errors(edges_fn(fx, fam, delta), truth_of(fx, fam, hub))
                for q in QUANTITIES:
                    for k in range(len(BAND_CUTS) + 1):
                        out[g][q][k] = max(out[g][q][k], err[q][b == k].max())
    return out


def truth_bound(group, q, k):
    return TRUTH_MARGIN * max(YARD_TRUTH[group][q][k], ROUNDING)


# ---------------------------------------------------------------- the truth checks itself -----------------------------------------
def test_fixture_holds_the_whole_sweep():
    fx = fixture()
    for key, val in MT.sweep_inputs().items():
        assert np.array_equal(fx[key], val), key                       # the inputs are a function of the committed seed
    ang = np.linalg.norm(fx["r"][:, :3], axis=1)
    assert len(ang) == len(MT.ANGLES) * len(MT.TRANSLATIONS) * MT.N_AXES
    assert set(bands(fx)) == set(range(len(BAND_CUTS) + 1))
    for lo, hi in ((0.5e-4, 1e-4), (1e-4, 2e-4), (0.15, 0.2), (0.2, 0.25)):      # both sides of both switches of the kernel
        assert ((ang > lo) & (ang < hi)).any(), (lo, hi)
    assert ang.min() <= 1e-10 and ang.max() >= 3.09
    sD = fx["Sj"][:, 12] / fx["Si"][:, 12] / fx["Z"][:, 12]
    assert (fx["r"][:, 6] == 0).sum() >= 10 and np.all(sD[fx["r"][:, 6] == 0] == 1.0)         # s_D = 1 exactly
    assert np.exp(fx["r"][:, 6]).min() < np.exp(-2.9) and np.exp(fx["r"][:, 6]).max() > np.exp(2.9)
    tm = np.linalg.norm(fx["r"][:, 3:6], axis=1)
    assert all(np.isclose(tm, t, rtol=1e-12).sum() == len(ang) // 3 for t in MT.TRANSLATIONS)
    for fam, cond in (("spd1", 1.0), ("spd1e4", 1e4), ("spd1e8", 1e8)):
        c = np.linalg.cond(fx["info_" + fam])
        assert np.all(c > 0.5 * cond) and np.all(c < 2 * cond)
    assert np.all(fx["info_rot_scale_only"][:, 3:6, :] == 0) and np.all(fx["info_rot_scale_only"][:, :, 3:6] == 0)
    for fam in MT.FAMILIES:                                            # the Huber delta splits the samples
        over = fx["w_" + fam + "_huber"] < 1.0
        assert 0.2 < over.mean() < 0.8, (fam, over.mean())
    assert os.path.getsize(MT.FIXTURE) < (1 << 20)


def test_fixture_equals_regenerated_truth():
    pytest.importorskip("mpmath")
    fx = fixture()
    idx = np.arange(0, len(fx["r"]), 17)                               # five samples across the angles
    again = MT.build_fixture(idx)
    assert sorted(again) == sorted(fx)
    for key, val in again.items():
        want = fx[key] if fx[key].ndim == 0 else fx[key][idx]
        assert np.array_equal(val, want), key


def test_truth_residual_is_the_residual_of_the_rounded_inputs():
    """the case is built backwards; the f64 inputs' own residual is the chosen r up to the rounding of S_j"""
    fx = fixture()
    N = len(fx["r"])
    r, _, D = R.residuals(np.concatenate([fx["Si"], fx["Sj"]]), np.stack([np.arange(N), N + np.arange(N)], 1), fx["Z"])
    size = 1 + np.abs(fx["Sj"][:, :12]).max(1) + np.abs(fx["r"]).max(1)
    assert np.all(np.abs(r - fx["r"]).max(1) <= 1e-13 * size * (1 + np.abs(fx["r"][:, 3:6]).max(1)))


# ---------------------------------------------------------------- yardsticks and the twin ---------------------------------------
def test_yardstick_truth():
    got = band_errors(fixture(), reference_edges)
    print({g: {q: tuple(float(f"{v:.1e}") for v in got[g][q]) for q in QUANTITIES} for g in GROUPS})
    for g in GROUPS:
        for q in QUANTITIES:
            for k in range(len(BAND_CUTS) + 1):
                if got[g][q][k] > ROUNDING / 4:
                    honest(got[g][q][k], YARD_TRUTH[g][q][k])
                else:
                    assert YARD_TRUTH[g][q][k] <= ROUNDING


def test_twin_against_truth():
    """the device's per-edge source, compiled for the host, within 16x the reference's own distance to the truth per band"""
    got = band_errors(fixture(), twin_edges)
    print({g: {q: tuple(float(f"{v:.1e}") for v in got[g][q]) for q in QUANTITIES} for g in GROUPS})
    for g in GROUPS:
        for q in QUANTITIES:
            for k in range(len(BAND_CUTS) + 1):
                assert got[g][q][k] <= truth_bound(g, q, k), (g, q, k, got[g][q][k])


def test_sanitized_twin_gives_the_library_twins_bits():
    """the stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer: the truth's edges (Huber off and on,
    fix_scale, the cost-only form), the retraction and the 7x7 inverse; a report would end it with a non-zero status"""
    fx = fixture()
    for fam in ("spd1e8", "rot_scale_only"):
        for delta, fix in ((0.0, False), (float(fx["delta_" + fam]), True)):
            a = TW.edges(fx["Si"], fx["Sj"], fx["Z"], fx["info_" + fam], delta, fix)
            b = TW.san_edges(fx["Si"], fx["Sj"], fx["Z"], fx["info_" + fam], delta, fix)
            assert all(np.array_equal(a[k], b[k]) for k in a)
    c = TW.san_edges(fx["Si"], fx["Sj"], fx["Z"], fx["info_diag"], 0.0, False, full=False)
    assert np.array_equal(c["rho"], TW.edges(fx["Si"], fx["Sj"], fx["Z"], fx["info_diag"])["rho"])      # cost-only == full
    bad = fx["Si"][:4].copy()
    bad[:, 12] = (0.0, -1.0, np.inf, np.nan)
    d = TW.san_edges(bad, fx["Sj"][:4], fx["Z"][:4], fx["info_diag"][:4])
    assert np.all(d["why"] == 32) and not d["W"].any() and not d["Di"].any() and not d["rho"].any()
    rng = np.random.default_rng(3)
    dx = np.concatenate([rng.normal(0, 1, (8, 7)) * np.array([1e-6, 1e-3, 0.3, 1, 1, 1, 1, 1])[:, None], np.zeros((1, 7))])
    assert np.array_equal(TW.san_update(dx, fx["Si"][:9]), TW.update(dx, fx["Si"][:9]))
    A = rng.normal(size=(5, 7, 7))
    A = A @ np.swapaxes(A, 1, 2) + np.eye(7)
    A[4, 6, 6] = -1.0                                                   # not SPD: the identity and the flag
    inv, ok = TW.san_inverse7(A)
    assert np.array_equal(inv, TW.inverse7(A)[0]) and ok.tolist() == [True] * 4 + [False] and np.array_equal(inv[4], np.eye(7))
    assert np.abs(inv[:4] @ A[:4] - np.eye(7)).max() < 1e-12


def test_twin_retraction_and_fix_scale():
    fx = fixture()
    rng = np.random.default_rng(5)
    dx = rng.normal(0, 1, (len(fx["Si"]), 7)) * rng.choice([1e-8, 0.9e-4, 1.1e-4, 0.1, 1.0], (len(fx["Si"]), 1))
    got, want = TW.update(dx, fx["Si"]), R.mul(R.phi(dx), fx["Si"])
    assert np.abs(got - want).max(1).max() <= 1e-13 * np.abs(want).max()
    dx[:, 6] = 0.0
    assert np.array_equal(TW.update(dx, fx["Si"])[:, 12], fx["Si"][:, 12])           # d_sigma = 0: every s bit for bit
    o = TW.edges(fx["Si"], fx["Sj"], fx["Z"], fx["info_spd1e4"], 0.0, fix_scale=True)
    Hi, bi = TW.full_blocks(o["Di"])
    Hj, bj = TW.full_blocks(o["Dj"])
    for M in (Hi, Hj, o["W"]):
        assert not M[:, 6, :].any() and not M[:, :, 6].any()
    assert not bi[:, 6].any() and not bj[:, 6].any()


def test_mutations_of_the_reference_miss_the_truth():
    fx = fixture()
    base = max(YARD_TRUTH["general"]["W"])
    for mutate in ("ad_t_sign", "drop_scale_column"):
        got = band_errors(fx, lambda f, fam, d: reference_edges(f, fam, d, mutate))
        worst = max(got["general"]["W"].max(), got["general"]["Hdiag"].max())
        print(mutate, worst, worst / base)
        assert worst >= MUTATION_FACTOR * base, (mutate, worst)


def test_jacobian_formulas_against_central_differences():
    rng = np.random.default_rng(0)
    sims = R.phi(np.concatenate([rng.normal(0, 0.8, (40, 3)), rng.normal(0, 2, (40, 3)), rng.normal(0, 0.8, (40, 1))], 1))
    edges = np.stack([np.arange(20), 20 + np.arange(20)], 1)
    Z = R.phi(np.concatenate([rng.normal(0, 0.8, (20, 3)), rng.normal(0, 2, (20, 3)), rng.normal(0, 0.8, (20, 1))], 1))
    _, Ji, Jj = R.jacobians(sims, edges, Z)
    _, Ni, Nj = R.jacobians(sims, edges, Z, numeric=True)
    assert rel(Ni, Ji) < 1e-7 and rel(Nj, Jj) < 1e-7          # h^2 truncation + eps / h rounding of a central difference
    a = R.linearize(sims, edges, Z, np.tile(np.eye(7), (20, 1, 1)))
    b = R.linearize(sims, edges, Z, np.tile(np.eye(7), (20, 1, 1)), numeric=True)
    assert all(rel(x, y) < 1e-6 for x, y in zip(a[1:], b[1:]))


# ---------------------------------------------------------------- scenes ------------------------------------------------------------
def test_drift_loop_is_closed_by_seven_dof_and_not_by_six():
    s = R.drift_loop()
    assert (s.V, s.E) == (60, 66) and s.fixed.sum() == 1 and s.fixed[0] == 1
    assert abs(np.log(R.parts(s.truth)[0][-1]) - 0.4 * 59 / 60) < 1e-15 and np.all(R.parts(s.init)[0] == 1.0)
    out, st = R.optimize(s.init, s.edges, s.meas, s.info, s.fixed)
    print(st, R.ate(s.init, s.gt), R.ate(out, s.gt))
    assert st["iterations"] <= 15 and st["chi2_final"] < 1e-20 * st["chi2_initial"]
    assert np.abs(R.parts(out)[0] - R.parts(s.truth)[0]).max() < 1e-12
    assert R.ate(out, s.gt) < 1e-12 * R.ate(s.init, s.gt) + 1e-13
    frozen, sf = R.optimize(s.init, s.edges, s.meas, s.info, s.fixed, fix_scale=True)
    print(sf, R.ate(frozen, s.gt))
    assert sf["chi2_final"] > 1e-3 * sf["chi2_initial"] and np.array_equal(R.parts(frozen)[0], R.parts(s.init)[0])


def test_scene_sizes():
    s = scene("hub")
    assert np.bincount(s.edges.ravel())[0] == 1000 and s.fixed[1] == 1 and s.fixed.sum() == 1 and np.ptp(s.init[:, 12]) > 0.1
    s = scene("sphere_s1")
    assert (s.V, s.fixed.sum(), s.fixed[0]) == (2500, 1, 1) and 9500 < s.E < 10500                     # the SE(3) suite's own sphere
    assert np.all(s.init[:, 12] == 1) and np.all(s.meas[:, 12] == 1) and np.array_equal(s.init[:, :12].reshape(-1, 3, 4), P.sphere().init)
    s = scene("drift_loop")
    assert s.V == 60 and R.cost(s.truth, s.edges, s.meas, s.info) > 10          # the noisy one


@pytest.mark.parametrize("name", sorted(R.SMALL_SCENES))
def test_reference_lm_lowers_chi2(name):
    s = scene(name)
    for solver in ("direct", "pcg"):
        out, st = solved(name, solver)
        assert st["chi2_final"] < 0.2 * st["chi2_initial"] and st["trials"] >= st["iterations"] >= 1, (solver, st)
        r, _, _ = R.residuals(out, s.edges, s.meas)
        assert np.linalg.norm(r[:, :3], axis=1).max() < 3.1


@pytest.mark.parametrize("name", sorted(R.SMALL_SCENES))
def test_solve_iterations_end_in_the_descent(name):
    s = scene(name)
    k = SOLVE_ITERATIONS[name]
    _, last = solved(name, "direct")
    _, before = R.optimize(s.init, s.edges, s.meas, s.info, s.fixed, iterations=k - 1)
    drop = (before["chi2_final"] - last["chi2_final"]) / last["chi2_final"]
    print(name, k, drop)
    assert last["iterations"] == last["trials"] == k and drop > 1e-6
    _, pc = solved(name, "pcg")
    assert pc["iterations"] == pc["trials"] == k and pc["cg_iterations"] < k * R.PCG_MAX_ITER        # the solves together stay well under the cap


def measure_lin():
    worst = dict.fromkeys(YARD_LIN, 0.0)
    for name in R.SMALL_SCENES:
        s = scene(name)
        for huber in (0.0, 3.0):
            a = R.linearize(s.init, s.edges, s.meas, s.info, huber)
            b = R.linearize(s.init, s.edges, s.meas, s.info, huber, series=True)
            for key, x, y in zip(("cost", "grad", "Hdiag", "W"), a, b):
                worst[key] = max(worst[key], abs(x - y) / abs(y) if key == "cost" else rel(x, y))
    return worst


def test_yardstick_linearisation():
    worst = measure_lin()
    print(worst)
    for key in YARD_LIN:
        honest(worst[key], YARD_LIN[key])


def measure_hmul():
    worst = 0.0
    rng = np.random.default_rng(2)
    for name in ("drift_loop", "hub"):                 # the dense matrix of sphere_s1 would take 2.4 GB
        s = scene(name)
        _, _, Hd, W = R.linearize(s.init, s.edges, s.meas, s.info)
        H = R.assemble(s.V, s.edges, Hd, W)
        x = rng.normal(size=(s.V, 7))
        lam = 1e-3 * np.abs(Hd).max()
        f = R.free_index(s.fixed)
        dense = np.zeros(7 * s.V)
        dense[f] = (H.toarray()[np.ix_(f, f)] + lam * np.eye(len(f))) @ x.ravel()[f]
        worst = max(worst, rel(R.hmul(H, s.fixed, lam, x).ravel(), dense))
    return worst


def test_yardstick_hmul():
    worst = measure_hmul()
    print(worst)
    honest(worst, YARD_HMUL)


def measure_solve(name):
    s = scene(name)
    (a, sa), (b, sb) = solved(name, "pcg"), solved(name, "direct")
    ang, dist, ls = R.sim_gap(a, b)
    return {"chi2": abs(sa["chi2_final"] - sb["chi2_final"]) / sb["chi2_final"], "rotation": ang, "translation": dist / P.extent(s.gt),
            "log_scale": ls}


@pytest.mark.parametrize("name", sorted(R.SMALL_SCENES))
def test_yardstick_solve(name):
    got = measure_solve(name)
    print(name, got)
    for key, v in got.items():
        honest(v, YARD_SOLVE[name][key])


def test_reduction_to_the_se3_reference():
    """fix_scale, every s = 1 and Omega = diag(Omega_6, w_sigma): the 6x6 corner of every block is pose_graph_ref.linearize"""
    for base, huber in ((P.loop_closure(n=96, closures=10), 0.0), (P.hub(140), 3.0)):
        V, E = base.V, base.E
        info = np.zeros((E, 7, 7))
        info[:, :6, :6] = base.info
        info[:, 6, 6] = 400.0
        c7, b7, H7, W7 = R.linearize(R.pack(np.ones(V), base.init), base.edges, R.pack(np.ones(E), base.meas), info, huber, fix_scale=True)
        c6, b6, H6, W6 = P.linearize(base.init, base.edges, base.meas, base.info, huber)
        ulp = lambda x, y: float(np.abs(x - y).max() / np.spacing(np.abs(y).max()))
        got = (abs(c7 - c6) / np.spacing(c6), ulp(b7[:, :6], b6), ulp(H7[:, :6, :6], H6), ulp(W7[:, :6, :6], W6))
        print(base.name, got)
        assert max(got) <= REDUCTION_ULPS
        assert not b7[:, 6].any() and not H7[:, 6].any() and not H7[:, :, 6].any() and not W7[:, 6].any() and not W7[:, :, 6].any()


# ---------------------------------------------------------------- product code that needs no GPU -------------------------------------
def test_plan_and_workspace_need_no_device(built):
    from slamhip import sim3_graph as G

    p = G.plan(512 * 36 + 1, 100)
    assert p["vertices_per_block"] == 36 and p["product_blocks"] == 512 and p["hub_blocks"] == 16 and p["hub_degree"] == 128
    assert p["edge_blocks"] == 2 and p["cg_check"] == 32 and p["launches_per_cg_iteration"] == 3 and p["slot_row_doubles"] == 7
    assert G.plan(36, 1)["product_blocks"] == 1 and G.plan(37, 1)["product_blocks"] == 2
    assert G.plan(1000, 3000)["workspace_bytes"] > 2 * 3000 * (49 + 35) * 8
    assert G.status_names(32 | 2) == ["angle", "scale"]


def test_edge_builders_and_readers(built):
    import slamhip
    from slamhip import sim3_graph as G

    rng = np.random.default_rng(7)
    B = 6
    mod = R.phi(np.concatenate([rng.normal(0, 0.5, (B, 3)), rng.normal(0, 2, (B, 3)), rng.normal(0, 0.6, (B, 1))], 1))
    s, Rm, t = G.split(mod)
    s[4] = -1.0
    pairs = np.array([[0, 1], [1, 2], [2, 2], [3, 0], [4, 1], [5, 3]])
    counts = np.array([40, 19, 50, 60, 70, 20])
    e, Z, info = slamhip.sim3_edges_from_sim3(pairs, (s, Rm, t), counts, min_inliers=20, rotation_sigma=0.01, translation_sigma=0.1,
                                              scale_sigma=0.05)
    assert e.tolist() == [[0, 1], [3, 0], [5, 3]] and e.dtype == np.int32                # too few inliers, i == j, s < 0 dropped
    assert np.array_equal(Z, mod[[0, 3, 5]]) and abs(np.log(Z[:, 12])).max() > 0.05          # kept at ANY scale
    assert np.allclose(info[1], 3.0 * np.diag([1e4] * 3 + [100.0] * 3 + [400.0]))
    _, _, _, scales = slamhip.loop_edges_from_sim3(pairs, (s, Rm, t), counts)                # unchanged behaviour beside it
    assert len(scales) == B
    base = P.loop_closure(n=20, closures=2)
    S, e2, Z2, I2 = slamhip.lift_se3_graph(base.init, base.edges, base.meas, base.info, scale_sigma=0.1)
    assert S.shape == (20, 13) and np.all(S[:, 12] == 1) and np.all(Z2[:, 12] == 1) and np.array_equal(S[:, :12].reshape(-1, 3, 4), base.init)
    assert np.array_equal(I2[:, :6, :6], base.info) and np.allclose(I2[:, 6, 6], 100.0) and not I2[:, 6, :6].any() and not I2[:, :6, 6].any()
    assert np.array_equal(slamhip.sims_to_poses(mod), R.to_poses(mod))
    three = [mod[0], mod[1], mod[2]]                                     # a list of three vertices is not the tuple (s, R, t)
    assert not G.is_srt(three) and G.is_srt((s[:3], Rm[:3], t[:3])) and np.array_equal(G._sims13(three), mod[:3])
    with pytest.raises(ValueError):
        slamhip.sim3_edges_from_sim3(pairs, (s, Rm, t), counts[:3])
    with pytest.raises(ValueError):
        slamhip.lift_se3_graph(base.init, base.edges, base.meas, base.info, scale_sigma=0.0)
    with pytest.raises(ValueError):
        slamhip.optimize_sim3_graph(S, e2, Z2, I2[:, :6, :6], np.eye(20)[0])
    with pytest.raises(ValueError):
        slamhip.optimize_sim3_graph(S, e2, Z2, I2, np.zeros(20))


def test_correct_points_keeps_camera_coordinates_up_to_the_scale_change(built):
    import slamhip

    s = R.drift_loop()
    after, _ = R.optimize(s.init, s.edges, s.meas, s.info, s.fixed)
    rng = np.random.default_rng(9)
    X = rng.normal(0, 3, (200, 3))
    k = rng.integers(0, s.V, 200)
    Y = slamhip.correct_points(X, k, s.init, after)
    sb, Rb, tb = R.parts(s.init[k])
    sa, Ra, ta = R.parts(after[k])
    cam_b = sb[:, None] * np.einsum("nij,nj->ni", Rb, X) + tb
    cam_a = sa[:, None] * np.einsum("nij,nj->ni", Ra, Y) + ta
    assert np.abs(cam_a - cam_b).max() < 1e-12 * np.abs(cam_b).max()
    # in METRIC camera coordinates (those of sims_to_poses) the point moves by the keyframe's scale change alone
    Tb, Ta = R.to_poses(s.init[k]), R.to_poses(after[k])
    mb = np.einsum("nij,nj->ni", Tb[:, :, :3], X) + Tb[:, :, 3]
    ma = np.einsum("nij,nj->ni", Ta[:, :, :3], Y) + Ta[:, :, 3]
    assert np.abs(ma * (sa / sb)[:, None] - mb).max() < 1e-12 * np.abs(mb).max()
    assert np.allclose(slamhip.correct_points(X, k, after, after), X, rtol=1e-12, atol=1e-12)          # no correction: no motion
    with pytest.raises(ValueError):
        slamhip.correct_points(X, k + s.V, s.init, after)


if __name__ == "__main__":
    np.set_printoptions(precision=1)
    got = band_errors(fixture(), reference_edges)
    for g in GROUPS:
        for q in QUANTITIES:
            print(g, q, tuple(float(f"{v:.1e}") for v in got[g][q]))
    print("lin", measure_lin())
    print("hmul", measure_hmul())
    for name in sorted(R.SMALL_SCENES):
        print(name, measure_solve(name))
