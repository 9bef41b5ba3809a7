"""CPU: the host side of the sparse bundle adjustment - slamhip.covisibility against a brute-force set construction, its
refusals, slam_bas_workspace / slam_bas_plan without a device - and the numpy statement the GPU tests compare against
(tests/ba_sparse_ref.py: block-Jacobi PCG at tolerance 1e-10 in place of the dense solve) held to oracle.ba_lm_c with the
bars of tests/test_ba_limits_gpu.py::_holds: the same accepted steps, cost 1e-9 relative, poses 1e-8, points 1e-7."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_sparse_ref as R  # noqa: E402
from oracle import oracle  # noqa: E402


def _mask(K, fixed):
    m = np.zeros(K, bool)
    m[list(fixed)] = True
    return m


def _check_against_brute(op, ol, K, fixed):
    from slamhip import covisibility

    op, ol = np.asarray(op, np.int32), np.asarray(ol, np.int32)
    edges, weights, ptr, pa, pb = covisibility(op, ol, K, _mask(K, fixed))
    cov = R.brute_covisibility(op, ol, K, _mask(K, fixed))
    keys = sorted(cov)
    assert edges.dtype == np.int32 and edges.shape == (len(keys), 2)
    assert [tuple(e) for e in edges.tolist()] == keys                    # k1 < k2, ascending by (k1, k2)
    assert all(k1 < k2 for k1, k2 in keys)
    assert weights.tolist() == [len(cov[k]) for k in keys]
    assert ptr.tolist() == np.r_[0, np.cumsum([len(cov[k]) for k in keys])].astype(int).tolist()
    assert pa.tolist() == [t[1] for k in keys for t in cov[k]]           # ascending in l inside an edge
    assert pb.tolist() == [t[2] for k in keys for t in cov[k]]
    for e, (k1, k2) in enumerate(keys):
        sl = slice(ptr[e], ptr[e + 1])
        assert (op[pa[sl]] == k1).all() and (op[pb[sl]] == k2).all() and (ol[pa[sl]] == ol[pb[sl]]).all()
        assert (np.diff(ol[pa[sl]]) > 0).all()
    return edges, weights


def test_covisibility_matches_brute_force_on_a_shuffled_chain(built):
    w = R.sliding(np.random.default_rng(1), 20, 600, fixed=(0, 1))
    edges, weights = _check_against_brute(w["op"], w["ol"], 20, w["fixed"])
    assert len(edges) > 20 and weights.max() > 1


def test_covisibility_tracks_of_length_one_make_no_pair(built):
    edges, _ = _check_against_brute([1, 2, 3, 4], [0, 1, 2, 3], 5, (0,))
    assert len(edges) == 0


def test_covisibility_point_seen_by_all_poses(built):
    K = 9
    edges, weights = _check_against_brute(np.arange(K), np.zeros(K, int), K, (0,))
    assert len(edges) == (K - 1) * (K - 2) // 2 and (weights == 1).all()


def test_covisibility_point_seen_only_by_fixed_poses(built):
    edges, weights = _check_against_brute([0, 3, 1, 2, 0, 3], [0, 0, 1, 1, 2, 2], 4, (0, 3))
    assert edges.tolist() == [[1, 2]] and weights.tolist() == [1]


def test_covisibility_fixed_poses_in_the_middle_of_the_range(built):
    rng = np.random.default_rng(7)
    K, L = 12, 40
    pick = np.sort(rng.choice(K * L, 200, replace=False))
    edges, _ = _check_against_brute(pick // L, pick % L, K, (4, 5, 9))
    assert not np.isin(edges, [4, 5, 9]).any() and len(edges) > 10


def test_covisibility_empty_observation_list(built):
    from slamhip import covisibility

    edges, weights, ptr, pa, pb = covisibility(np.zeros(0, np.int32), np.zeros(0, np.int32), 3, [True, False, False])
    assert edges.shape == (0, 2) and len(weights) == 0 and ptr.tolist() == [0] and len(pa) == 0 and len(pb) == 0


def test_covisibility_refusals(built, monkeypatch):
    from slamhip import ba_sparse, covisibility

    fixed = [True, False, False]
    for op, ol in (([0, 3], [0, 0]), ([0, -1], [0, 0]), ([0, 1], [0, -1])):
        with pytest.raises(ValueError, match="out of range"):
            covisibility(op, ol, 3, fixed)
    with pytest.raises(ValueError, match="out of range"):
        covisibility([0, 1], [0, 5], 3, fixed, L=5)
    with pytest.raises(ValueError, match="more than once"):
        covisibility([1, 2, 1], [4, 4, 4], 3, fixed)
    with pytest.raises(ValueError, match="fixed"):
        covisibility([1, 2], [0, 0], 3, [False, False, False])
    with pytest.raises(ValueError):
        covisibility([1, 2], [0, 0], 3, [True, False])                   # a mask of the wrong length
    with pytest.raises(ValueError):
        covisibility([1.0, 2.0], [0, 0], 3, fixed)                       # indices that are not integers
    K = 8
    op, ol = np.arange(1, K), np.zeros(K - 1, int)                       # 7 free poses on one point: 21 pairs, 21 edges
    monkeypatch.setattr(ba_sparse, "MAX_PAIRS", 20)
    with pytest.raises(ValueError, match="pairs"):
        covisibility(op, ol, K, _mask(K, (0,)))
    monkeypatch.setattr(ba_sparse, "MAX_PAIRS", 1 << 30)
    monkeypatch.setattr(ba_sparse, "MAX_EDGES", 20)
    with pytest.raises(ValueError, match="edges"):
        covisibility(op, ol, K, _mask(K, (0,)))
    monkeypatch.undo()
    assert ba_sparse.MAX_PAIRS == 1 << 30 and ba_sparse.MAX_EDGES == 1 << 25       # the limits of slamhip.h


def test_workspace_and_plan_need_no_device(built):
    from slamhip import ba_sparse
    from slamhip._lib import SlamHipError

    p = ba_sparse.plan(200, 50000, 10 ** 6, 5000, 3 * 10 ** 6)
    assert p["obs_blocks"] == (10 ** 6 + 255) // 256 and p["point_blocks"] == (50000 + 255) // 256 and p["pose_blocks"] == 200
    assert p["edge_blocks"] == 1250 and p["candidate_blocks"] == (50200 + 255) // 256 and p["threads"] == 256 and p["lanes_per_edge"] == 64
    # the blocks that grow with the problem: Hpl per observation, 33 doubles and a pointer slot per point, 36 doubles per edge
    small, big = ba_sparse.workspace_bytes(10, 10, 0, 0, 0), p["workspace_bytes"]
    assert big >= 10 ** 6 * (144 + 32) + 50000 * 8 * 30 + 5000 * 288 + 3 * 10 ** 6 * 8 and 0 < small < 1 << 16
    assert ba_sparse.plan(2 ** 24, 1, 0, 0, 0)["candidate_blocks"] == 1024          # the partial sums are capped
    for bad in ((0, 1, 0, 0, 0), (2 ** 24 + 1, 1, 0, 0, 0), (1, 0, 0, 0, 0), (1, 1, 2 ** 28 + 1, 0, 0), (4, 4, 8, 2 ** 25 + 1, 2 ** 26),
                (4, 4, 8, 3, 2), (4, 4, 8, 3, 2 ** 30 + 1)):
        with pytest.raises(SlamHipError):
            ba_sparse.workspace_bytes(*bad)
        with pytest.raises(SlamHipError):
            ba_sparse.plan(*bad)


def test_numpy_reduced_system_equals_the_oracles_dense_one(built):
    """tests/ba_sparse_ref.py's blocks put together are oracle.ba_schur_np's S and rhs (scattered fixed poses, Huber)."""
    w = R.sliding(np.random.default_rng(3), 14, 500, fixed=(0, 6, 7))
    K, lam, delta = 14, 3.0, 1.0
    fixed = _mask(K, w["fixed"])
    T12 = w["T0"][:, :3, :4].reshape(K, 12)
    lin = R.linearize(T12, w["X0"], w["op"], w["ol"], w["meas"], R.INTR, delta)
    red = R.reduce(lin, w["op"], w["ol"], fixed, lam)
    ref = oracle.ba_schur_np(T12, w["X0"], w["op"], w["ol"], w["meas"], *R.INTR, delta, lam)
    S = R.dense_system(red, lam)
    free = np.flatnonzero(~fixed)
    scale = np.abs(ref["S"]).max()
    assert np.abs(S[np.ix_(free, free)] - ref["S"][np.ix_(free, free)]).max() <= 1e-12 * scale
    assert np.abs(-red["b"][free] - ref["rhs"][free]).max() <= 1e-12 * np.abs(ref["rhs"]).max()
    assert abs(lin["cost"] - ref["cost"]) <= 1e-12 * ref["cost"]
    x = np.random.default_rng(4).normal(size=(K, 6))
    y = np.einsum("ijab,jb->ia", S[np.ix_(free, free)], x[free])
    assert np.abs(R.hmul(red, fixed, lam, x)[free] - y).max() <= 1e-12 * np.abs(y).max()


@pytest.mark.parametrize("K,O,delta", [(12, 1168, 0.0), (24, 2900, 1.0), (40, 5999, 0.0)])
def test_numpy_statement_follows_the_oracle(built, K, O, delta):
    """Sliding windows (tracks of 2 to 6), 6 iterations: block-Jacobi PCG at 1e-10 against oracle.ba_lm_c's direct solve."""
    w = R.sliding(np.random.default_rng(1000 + K), K, O, fixed=(0, 1))
    Tr, Xr, c0, c1, acc, _ = oracle.ba_lm_c(w["T0"][:, :3, :4].reshape(K, 12), w["X0"], w["op"], w["ol"], w["meas"], *R.INTR, 6, w["fixed"], delta)
    T, X, g0, g1, gacc, st = R.lm(w["T0"], w["X0"], w["op"], w["ol"], w["meas"], R.INTR, 6, w["fixed"], delta, 1e-10, 500)
    assert gacc == acc and acc >= 3 and st["unconverged"] == 0
    assert abs(g0 - c0) <= 1e-9 * c0 and abs(g1 - c1) <= 1e-9 * max(c1, 1.0)
    assert np.abs(T - Tr).max() <= 1e-8, np.abs(T - Tr).max()
    assert np.abs(X - Xr).max() <= 1e-7, np.abs(X - Xr).max()
    for k in w["fixed"]:
        assert np.array_equal(T[k], w["T0"][k])
