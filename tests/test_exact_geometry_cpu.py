"""CPU: the f64 oracle against exact rational arithmetic (tests/exact_geometry.py) on the named geometry set.

Tolerance rule (exact_geometry.C): |oracle - exact| <= C 2^-53 bound, per element, where the bound is the same expression
evaluated on absolute values; an element with a zero bound must match exactly."""
import numpy as np
import pytest

import exact_geometry as eg
from oracle import oracle

SCHUR_CASES = tuple(c for c in eg.CASES if c != "tiny_z")
# tiny_z has no Schur test: |Z| <= 1e-6 makes Hll ~ 1e48, of rank 2 for a point seen once, so Hll + lambda I is singular
# in f64 for every lambda the LM takes (ba_schur_np's inverse raises); there is no f64 result to hold to a bound.


def _zero_eps(c, o):
    """The frontend.py:286-291 expression with the 1e-18 dropped, evaluated exactly."""
    P = [eg.B(eg.F(v)) for v in c.poses12[c.obs_pose[o]]]
    X = [eg.B(eg.F(v)) for v in c.points[c.obs_point[o]]]
    p = [P[4 * i] * X[0] + P[4 * i + 1] * X[1] + P[4 * i + 2] * X[2] + P[4 * i + 3] for i in range(3)]
    return eg.closed_form_jacobians(P, p, [eg.B(eg.F(v)) for v in c.cam], eg.B(0))


@pytest.mark.parametrize("name", eg.CASES)
def test_closed_form_is_the_derivative(name):
    """frontend.py:288-291's pose Jacobian is exactly the derivative of e(exp([w, v]) T) at 0 (rotation first), and -A R
    exactly the derivative with respect to the world point, once the 1e-18 is dropped: Fraction equality, every row."""
    c = eg.case(name)
    for o in range(c.O):
        Jp, Jq = _zero_eps(c, o)
        Dp, Dq = eg.dual_jacobians([eg.F(v) for v in c.poses12[c.obs_pose[o]]], [eg.F(v) for v in c.points[c.obs_point[o]]],
                                   [eg.F(v) for v in c.meas[o]], [eg.F(v) for v in c.cam])
        assert [[x.v for x in r] for r in Jp] == Dp, (name, o)
        assert [[x.v for x in r] for r in Jq] == Dq, (name, o)


def test_the_geometry_set_stresses_what_it_names():
    """The cases are what their names say (so a generator change cannot quietly make them benign)."""
    def cam_z(name):
        return np.array([float(q.p[2].v) for q in eg.exact_lins(name)])

    def ratio(name):
        return np.array([float(abs(q.p[0].v / q.p[2].v)) for q in eg.exact_lins(name)])

    assert ratio("wide").max() > 5
    assert cam_z("far").min() > 500 and cam_z("far").max() > 5e4
    assert cam_z("near").max() < 0.02 and cam_z("near").min() > 5e-4
    assert (cam_z("behind") < 0).all()
    z = np.abs(cam_z("tiny_z"))
    assert z.max() <= 1e-6 and z.min() >= 1e-12 and (cam_z("tiny_z") < 0).any()
    q = eg.exact_lins("cancel")
    assert min(float(x.p[2].m / abs(x.p[2].v)) for x in q) > 1e3       # |R||X| + |t| >> |p|
    rot = eg.case("rotations").poses12.reshape(-1, 3, 4)[:, :, :3]
    assert np.array_equal(rot[0], np.eye(3)) and all(set(np.abs(r).ravel()) == {0.0, 1.0} for r in rot[1:4])
    from scipy.spatial.transform import Rotation

    assert (np.pi - Rotation.from_matrix(rot[4:]).magnitude() <= 1.01e-6).all()
    c = eg.case("huber_edge")
    n2 = [q.c2.v for q in eg.exact_lins("huber_edge")]
    d2 = eg.F(c.delta) ** 2
    assert sum(x == d2 for x in n2) >= 10 and sum(x < d2 for x in n2) >= 10 and sum(x > d2 for x in n2) >= 10


@pytest.mark.parametrize("name", eg.CASES)
def test_reproj_oracle_is_exact(name):
    c = eg.case(name)
    lins = eg.exact_lins(name)
    e, Jp, Jq = oracle.reproj_rj_c(c.poses12, c.points, c.obs_pose, c.obs_point, c.meas, *c.cam)
    eg.assert_exact(e, [q.e for q in lins], f"{name} e")
    eg.assert_exact(Jp, [q.Jp for q in lins], f"{name} Jpose")
    eg.assert_exact(Jq, [q.Jq for q in lins], f"{name} Jpoint")
    assert (Jp[:, 0, 4] == 0).all() and (Jp[:, 1, 3] == 0).all()


@pytest.mark.parametrize("name", eg.CASES)
def test_pose_normal_equations_oracle_is_exact(name):
    """oracle_pose_normal_eq_f64 on the observations of pose 0: no kernel, the case's splitting delta; all rows and a
    mixed active mask."""
    c = eg.case(name)
    sel = np.flatnonzero(c.obs_pose == 0)
    lins = [eg.exact_lins(name)[o] for o in sel]
    pts, meas = c.points[c.obs_point[sel]], c.meas[sel]
    mixed = (np.arange(len(sel)) % 3 != 1).astype(np.uint8)
    for delta in (0.0, c.delta):
        for act in (np.ones(len(sel), np.uint8), mixed):
            H, b, chi2 = oracle.pose_normal_eq_c(c.poses12[0], pts, meas, act, *c.cam, delta)
            rH, rb, rchi2 = eg.pose_normal_eq(lins, act, delta)
            eg.assert_exact(H, rH, f"{name} H delta={delta}")
            eg.assert_exact(b, rb, f"{name} b delta={delta}")
            eg.assert_exact(chi2, rchi2, f"{name} chi2")


@pytest.mark.parametrize("name", eg.CASES)
def test_huber_cost_oracle_is_exact(name):
    """oracle._huber_rho on the exact chi2 rounded to doubles, against the exact robust cost."""
    c = eg.case(name)
    lins = eg.exact_lins(name)
    chi2 = eg.values([q.c2 for q in lins])
    for delta in (0.0, c.delta):
        ref = eg.bsum(eg.huber(eg.B(eg.F(x)), delta)[1] for x in chi2)
        eg.assert_exact(oracle._huber_rho(chi2, delta), ref, f"{name} rho delta={delta}")


def test_huber_edge_weights():
    """At the Huber edge the weight is exactly 1 on both sides of the comparison (the function is continuous), one
    measurement ulp outside it is delta / sqrt(c2) < 1, one ulp inside it is 1."""
    c = eg.case("huber_edge")
    d2 = eg.F(c.delta) ** 2
    for q in eg.exact_lins("huber_edge"):
        w, rho = eg.huber(q.c2, c.delta)
        assert (w.v == 1) == (q.c2.v <= d2)
        if q.c2.v == d2:
            assert rho.v == d2 and w.v == 1


@pytest.mark.parametrize("name", SCHUR_CASES)
def test_schur_oracle_is_exact(name):
    """oracle.ba_schur_np / ba_backsub_np on well-conditioned windows of at most four poses (a point seen by every pose,
    a pose with no observation, points nobody observes; exact_geometry.schur_configs): every output within the bound, and
    the bound tight enough that a wrong reduction fails it."""
    c = eg.case(name)
    rng = np.random.default_rng(3)
    for ks, sel, delta, lam in eg.schur_configs(name):
        P, op, ol, meas = eg.window_problem(c, ks, sel)
        ref = eg.schur([eg.exact_lins(name)[o] for o in sel], op, ol, len(P), c.L, delta, lam)
        red = oracle.ba_schur_np(P, c.points, op, ol, meas, *c.cam, delta, lam)
        for key in ("S", "rhs", "bp", "bl", "E"):
            eg.assert_exact(red[key], ref[key], f"{name} {key}")
        eg.assert_exact(red["cost"], eg.bsum(ref["cost"]), f"{name} cost")
        dp = rng.normal(0, 1e-3, (len(P), 6))
        dl, dl_ref = oracle.ba_backsub_np(red, op, ol, dp), eg.backsub(ref, op, ol, dp)
        eg.assert_exact(dl, dl_ref, f"{name} dl")
        eg.assert_schur_is_tight(red["S"], red["rhs"], red["bp"], dl, ref, dl_ref, name)


@pytest.mark.parametrize("name", SCHUR_CASES)
def test_schur_oracle_at_extreme_damping(name):
    """The same with the point seen once kept and lambda = 1e-8 or 1e3: every output within the bound, which for S, rhs
    and dl is as wide as the ill-conditioned E makes it; bp, bl and the cost do not go through E and stay tight."""
    c = eg.case(name)
    for ks, sel, delta, lam in eg.schur_configs(name, extreme=True):
        P, op, ol, meas = eg.window_problem(c, ks, sel)
        ref = eg.schur([eg.exact_lins(name)[o] for o in sel], op, ol, len(P), c.L, delta, lam)
        red = oracle.ba_schur_np(P, c.points, op, ol, meas, *c.cam, delta, lam)
        for key in ("S", "rhs", "bp", "bl", "E"):
            eg.assert_exact(red[key], ref[key], f"{name} {key}")
        eg.assert_exact(red["cost"], eg.bsum(ref["cost"]), f"{name} cost")
        dp = np.random.default_rng(3).normal(0, 1e-3, (len(P), 6))
        eg.assert_exact(oracle.ba_backsub_np(red, op, ol, dp), eg.backsub(ref, op, ol, dp), f"{name} dl")
