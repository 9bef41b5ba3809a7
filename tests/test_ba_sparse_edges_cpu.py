"""CPU: the premises of tests/test_ba_sparse_edges_gpu.py, asserted on tests/ba_sparse_cases.py and tests/ba_sparse_ref.py
alone - every case has the property it exists for: list lengths, edge pair counts, where the largest diagonal lies, that
every term is exact in f64 (the numpy f64 restatement of ba_linearise equals the Fraction statement byte for byte, summed in
any order), that every magnitude stays below 2^53, that the integer path equals Fractions from end to end, the launch plan
of the candidate, and that the numpy reference is finite on the long-list layout at the dampings used."""
import os
import sys
from fractions import Fraction as F

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_sparse_cases as C  # noqa: E402
import ba_sparse_ref as R  # noqa: E402


def _rt(T):
    return T[:, :3, :4].reshape(len(T), 12)


@pytest.mark.parametrize("variant", ["e7", "e8"])
def test_long_layout_has_the_stated_lists_and_edges(built, variant):
    """Case 1: observation counts per pose, pair counts per edge, tracks of length 1, unobserved points, E mod 4 - on the
    brute-force covisibility and on the product's own tables."""
    from slamhip import covisibility
    from slamhip.ba import observation_lists

    lay = C.long_layout(variant)
    K, L = lay["K"], len(lay["tracks"])
    op, ol = C.observations(lay["tracks"], 3)
    fixed = np.zeros(K, bool)
    fixed[0] = True
    n = np.bincount(op, minlength=K)
    assert {k: int(v) for k, v in enumerate(n)} == lay["obs"]
    assert {255, 256, 257, 512, 513, 1, 1025} <= set(n[1:].tolist()) and n[0] == n.max() > 1025
    cov = R.brute_covisibility(op, ol, K, fixed)
    assert {k: len(v) for k, v in cov.items()} == lay["edges"]
    assert {63, 64, 65, 128, 129} <= set(lay["edges"].values())
    assert (len(cov) % 4 == 0) == (variant == "e8")
    lengths = np.bincount(ol, minlength=L)
    assert (lengths == 1).sum() >= 400 and (lengths == 0).sum() == 2 and lengths.max() == 3
    edges, weights, pair_ptr, pa, pb = covisibility(op, ol, K, fixed, L)
    assert [tuple(e) for e in edges.tolist()] == sorted(cov) and weights.tolist() == [len(cov[k]) for k in sorted(cov)]
    pt_ptr, pt_obs, ps_ptr, ps_obs = observation_lists(op, ol, K, L)
    assert np.diff(ps_ptr).tolist() == n.tolist() and np.diff(pt_ptr).tolist() == lengths.tolist()


@pytest.mark.parametrize("lam", [1e-6, 2.5, 1e9])
def test_numpy_reference_is_finite_on_the_long_layout(built, lam):
    """Case 1 on the random scene: ba_sparse_ref's blocks and bounds are finite at the three dampings, its edges the stated ones."""
    lay = C.long_layout()
    w = C.random_window(lay)
    fixed = np.zeros(lay["K"], bool)
    fixed[0] = True
    lin = R.linearize(_rt(w["T0"]), w["X0"], w["op"], w["ol"], w["meas"], R.INTR, 1.0)
    red = R.reduce(lin, w["op"], w["ol"], fixed, lam)
    for name in ("Hdiag", "W", "b", "E"):
        assert np.isfinite(red[name]).all(), name
    assert all(np.isfinite(v).all() for v in red["bound"].values())
    assert {tuple(e): int(n) for e, n in zip(red["edges"].tolist(), red["weights"])} == lay["edges"]
    assert abs(lin["cost_pose"].sum() - lin["cost"]) <= 1e-12 * lin["cost"]
    print(f"\nlong layout, lambda = {lam}: largest bound / |W| {float((red['bound']['W'] / np.abs(red['W']).max()).max()):.3g}")


@pytest.mark.parametrize("i", range(6))
def test_grid_scenes_are_exact_in_f64(built, i):
    """Case 2's premise.  Camera coordinates on the grid; every residual norm one of 0, 5, 10, 20 (weights 1, 1/2, 1/4, the
    norm 5 = delta at weight 1); every term of every sum an f64 number, equal to its Fraction; the f64 sums - np.add.at in
    observation order, and in the reverse order - equal the exact ones byte for byte; all below 2^53; the total cost an
    integer."""
    sc, delta = C.grid_scenes()[i]
    ex = C.linearize_exact(sc, delta)
    pc = sc["pc"]
    assert (np.abs(pc[:, :2]) <= 4).all() and np.isin(pc[:, 2], [1, 2, 4, 8]).all()
    t = ex["terms"]
    assert t["den"]["e"] == t["den"]["jp"] == t["den"]["jq"] == 1 and t["den"]["w"] in (1, 4) and t["den"]["rho"] == 1
    assert np.array_equal(t["e"], sc["res"])
    if delta == 5.0:
        norms = np.sqrt((sc["res"] ** 2).sum(1))
        assert set(norms.tolist()) == {0.0, 5.0, 10.0, 20.0} and set(t["w"].tolist()) == {4, 2, 1}
        assert (t["w"][norms == 5.0] == 4).all() and (t["rho"][norms == 5.0] == 25).all()      # the strict gate
        assert (t["rho"][norms == 20.0] == 175).all() and (t["rho"][norms == 10.0] == 75).all()
    if delta == C.SQRT2:
        assert float(np.sqrt(2.0)) == delta and F(delta) ** 2 > 2                 # en == delta in f64, en^2 < delta^2 exactly
        assert set(t["rho"].tolist()) == {0, 2} and (t["w"] == 1).all()
    assert ex["total"].denominator == 1
    f = C.linearise_f64(sc, delta)
    K, L, op, ol = sc["K"], sc["L"], sc["op"], sc["ol"]
    assert C.same_bits(f["Hpl"].reshape(-1, 18), ex["Hpl"])
    for order in (np.arange(len(op)), np.arange(len(op))[::-1]):
        Hpp, bp, Hll, bl, cost = np.zeros((K, 6, 6)), np.zeros((K, 6)), np.zeros((L, 3, 3)), np.zeros((L, 3)), np.zeros(K)
        np.add.at(Hpp, op[order], f["Hpp"][order])
        np.add.at(bp, op[order], f["bp"][order])
        np.add.at(Hll, ol[order], f["Hll"][order])
        np.add.at(bl, ol[order], f["bl"][order])
        np.add.at(cost, op[order], f["rho"][order])
        assert C.same_bits(C.packed(Hpp, C.TRI), ex["Hpp"]) and C.same_bits(bp, ex["bp"]) and C.same_bits(cost, ex["cost"])
        assert C.same_bits(C.packed(Hll, C.TRI3), ex["Hll"]) and C.same_bits(bl, ex["bl"])
    assert max(np.abs(ex[n]).max() for n in ("Hpp", "bp", "Hll", "bl", "Hpl", "cost")) < 2.0 ** 53
    print(f"\n{sc['name']}, delta = {delta}: largest entry {max(np.abs(ex[n]).max() for n in ('Hpp', 'bp', 'Hll', 'bl', 'Hpl')):.3g}, cost {ex['total']}")


def test_integer_sums_equal_fraction_sums(built):
    """The common-denominator integer path of linearize_exact against Fractions from end to end, for the poses with 1, 255
    and 1025 observations and three points."""
    sc = C.grid_scene(C.long_layout(), 21)
    ex = C.linearize_exact(sc, 5.0)
    for k in (7, 2, 1):
        obs = np.flatnonzero(sc["op"] == k)
        for n, (a, c) in enumerate(C.TRI):
            s = sum((ex["lin"][o][3] * (ex["lin"][o][1][0][a] * ex["lin"][o][1][0][c] + ex["lin"][o][1][1][a] * ex["lin"][o][1][1][c]) for o in obs), F(0))
            assert F(float(ex["Hpp"][k, n])) == s
        assert F(float(ex["cost"][k])) == sum((ex["lin"][o][4] for o in obs), F(0))
        for a in range(6):
            s = sum((ex["lin"][o][3] * (ex["lin"][o][1][0][a] * ex["lin"][o][0][0] + ex["lin"][o][1][1][a] * ex["lin"][o][0][1]) for o in obs), F(0))
            assert F(float(ex["bp"][k, a])) == s
    for l in (0, 1, 2):
        obs = np.flatnonzero(sc["ol"] == l)
        for n, (a, c) in enumerate(C.TRI3):
            s = sum((ex["lin"][o][3] * (ex["lin"][o][2][0][a] * ex["lin"][o][2][0][c] + ex["lin"][o][2][1][a] * ex["lin"][o][2][1][c]) for o in obs), F(0))
            assert F(float(ex["Hll"][l, n])) == s


def test_largest_diagonal_lies_where_the_case_says(built):
    """Long layout: the FIXED pose holds the largest diagonal entry of all, so the answer (over free poses and points) is
    smaller and a missing skip shows.  K = 300: the winner is pose 299 / point 299, strictly, past the first 256."""
    for sc, delta in C.grid_scenes()[:3]:
        ex = C.linearize_exact(sc, delta)
        assert ex["dmax_pose"][0] > ex["dmax"] == ex["dmax_pose"][1:].max() > ex["dmax_point"].max()
    ex = C.linearize_exact(*C.grid_scenes()[4])
    assert ex["dmax"] == ex["dmax_pose"][299] > max(np.delete(ex["dmax_pose"], [0, 299]).max(), ex["dmax_point"].max())
    ex = C.linearize_exact(*C.grid_scenes()[5])
    assert ex["dmax"] == ex["dmax_point"][299] > max(ex["dmax_pose"][1:].max(), ex["dmax_point"][:299].max())


@pytest.mark.parametrize("lam", [0, 1])
def test_integer_blocks_reduce_exactly(built, lam):
    """Cases 4 and 6's premise: Hll + lambda I is one of UNIMODULAR, every determinant 1, 2, 4 or 8, the inverse times 8 an
    integer matrix and truly the inverse; the integer path equals Fractions from end to end for an edge of 129 pairs and
    one of 1, and dl for a hub point (41 observations), a track of 1 and an unobserved point."""
    for lay, seed in ((C.long_layout(), 31), (C.hub_layout(), 32)):
        K, L = lay["K"], len(lay["tracks"])
        op, ol = C.observations(lay["tracks"], seed)
        fixed = np.zeros(K, bool)
        fixed[0] = True
        blk = C.integer_blocks(K, L, op, ol, lam, seed)
        adj, det = C.adjugate(blk["M"])
        assert set(det.tolist()) <= {1, 2, 4, 8} and len(set(det.tolist())) >= 3
        assert np.array_equal(np.einsum("lab,lbc->lac", blk["M"], adj), det[:, None, None] * np.eye(3, dtype=np.int64)[None])
        assert np.array_equal(blk["Hll"] + lam * np.eye(3, dtype=np.int64), blk["M"]) and (blk["dp"] != 0).all()
        assert np.array_equal(blk["Hpp"], blk["Hpp"].transpose(0, 2, 1))
        cov = R.brute_covisibility(op, ol, K, fixed)
        ex = C.reduce_exact(blk, cov)
        assert np.array_equal(ex["E"][~blk["seen"]], np.zeros(((~blk["seen"]).sum(), 9))) and (~blk["seen"]).sum() >= 2
        assert np.array_equal(ex["dl"][~blk["seen"]], np.zeros(((~blk["seen"]).sum(), 3)))
        sizes = sorted({len(v) for v in cov.values()})
        for i, k in enumerate(ex["keys"]):
            if len(cov[k]) in (sizes[0], sizes[-1]) and i < 400:
                Wf = C.edge_fraction(blk, cov[k])
                assert all(F(float(ex["W"][i, r * 6 + s])) == Wf[r][s] for r in range(6) for s in range(6))
                break
        lengths = np.bincount(ol, minlength=L)
        for l in (int(lengths.argmax()), int(np.flatnonzero(lengths == 1)[0]), int(np.flatnonzero(lengths == 0)[0])):
            assert [F(float(v)) for v in ex["dl"][l]] == C.point_step_fraction(blk, l)
        if lay["K"] == 41:
            assert lengths.max() == 41 and len(cov) == 780
    # against the numpy statement: the exact values lie within its own bound
    lay = C.long_layout()
    op, ol = C.observations(lay["tracks"], 31)
    blk = C.integer_blocks(lay["K"], len(lay["tracks"]), op, ol, lam, 31)
    fixed = np.arange(lay["K"]) == 0
    ex = C.reduce_exact(blk, R.brute_covisibility(op, ol, lay["K"], fixed))
    lin = dict(Hpp=blk["Hpp"].astype(float), bp=blk["bp"].astype(float), Hll=blk["Hll"].astype(float), bl=blk["bl"].astype(float),
               Hpl=blk["Hpl"].astype(float), K=blk["K"], L=blk["L"])
    red = R.reduce(lin, op, ol, fixed, float(lam))
    assert np.abs(red["W"].reshape(-1, 36) - ex["W"]).max() <= 1e-9 and np.abs(red["Hdiag"].reshape(-1, 36) - ex["Hdiag"]).max() <= 1e-9
    assert np.abs(red["b"] - ex["b"]).max() <= 1e-9
    assert np.abs(R.backsub(lin, red, op, ol, blk["dp"].astype(float))[blk["seen"]] - ex["dl"][blk["seen"]]).max() <= 1e-9


def test_candidate_cases_and_launch_plan(built):
    """Case 7's premise: K + L past 1024 * 256 needs the grid-stride loop (the plan reports the cap of 1024 workgroups),
    the other shapes sit at 255, 256, 257 and exactly 262144 items; fixed poses carry non-zero dp and bp; the denominator
    is an integer well below 2^53; the rotating poses turn by 0.5 to 1.5 rad."""
    from slamhip import ba_sparse

    totals = []
    for K, L in C.CANDIDATE_SHAPES:
        c = C.candidate_case(K, L)
        p = ba_sparse.plan(K, L, 0, 0, 0)
        totals.append(K + L)
        assert p["candidate_blocks"] == min(1024, (K + L + 255) // 256) and p["threads"] == 256
        assert c["fixed"][0] and c["fixed"].sum() >= 2 and (c["dp"][c["fixed"]] != 0).all() and (c["bp"][c["fixed"]] != 0).all()
        th = np.linalg.norm(c["dp"][c["rot"], :3], axis=1)
        assert len(c["rot"]) >= 2 and (th >= 0.5).all() and (th <= 1.5).all() and not c["fixed"][c["rot"]].any()
        Tn, Xn, den, plain = C.candidate_exact(c)
        assert abs(den) < 2 ** 40 and den != 0 and (c["dp"][~c["fixed"] & plain, :3] == 0).all()
        fixed_terms = int((c["dp"][c["fixed"]] * (2 * c["dp"][c["fixed"]] - c["bp"][c["fixed"]])).sum())
        assert fixed_terms != 0                                               # a kernel that adds them shows
    assert totals == [262144 + 593, 262144, 255, 256, 257]
    assert ba_sparse.plan(300, 262144 + 293, 0, 0, 0)["candidate_blocks"] == 1024 and 300 + 262144 + 293 > 1024 * 256


def test_embedding_keeps_every_list_in_order(built):
    """Case 9's premise: in the larger problem every original pose list, point list and edge pair list is the original one
    under the (increasing) maps, and the extra poses and points see only each other."""
    from slamhip import covisibility
    from slamhip.ba import observation_lists

    lay = C.long_layout()
    w = C.random_window(lay)
    big, pm, lm, om = C.embed(w)
    K, L, K2, L2 = lay["K"], len(lay["tracks"]), len(big["T0"]), len(big["X0"])
    assert (K2, L2) == (K + 40, L + 500) and (np.diff(pm) > 0).all() and (np.diff(lm) > 0).all() and (np.diff(om) > 0).all()
    inside = np.zeros(len(big["op"]), bool)
    inside[om] = True
    assert not np.isin(big["op"][~inside], pm).any() and not np.isin(big["ol"][~inside], lm).any()
    a, b = observation_lists(w["op"], w["ol"], K, L), observation_lists(big["op"], big["ol"], K2, L2)
    for k in range(K):
        assert np.array_equal(om[a[3][a[2][k]:a[2][k + 1]]], b[3][b[2][pm[k]]:b[2][pm[k] + 1]])
    for l in range(L):
        assert np.array_equal(om[a[1][a[0][l]:a[0][l + 1]]], b[1][b[0][lm[l]]:b[0][lm[l] + 1]])
    f1, f2 = np.arange(K) == 0, np.arange(K2) == 0
    e1, _, p1, a1, b1 = covisibility(w["op"], w["ol"], K, f1, L)
    e2, _, p2, a2, b2 = covisibility(big["op"], big["ol"], K2, f2, L2)
    where = {tuple(e): i for i, e in enumerate(e2.tolist())}
    for i, (k1, k2) in enumerate(e1.tolist()):
        j = where[(int(pm[k1]), int(pm[k2]))]
        assert np.array_equal(om[a1[p1[i]:p1[i + 1]]], a2[p2[j]:p2[j + 1]]) and np.array_equal(om[b1[p1[i]:p1[i + 1]]], b2[p2[j]:p2[j + 1]])
    assert len(e2) > len(e1)
