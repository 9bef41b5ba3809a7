"""Absolute pose at its edges, on the host twin of csrc/pnp.hip and once more through the same code under the address and
undefined-behaviour sanitizers: candidates of 0 .. 4 correspondences, identical / collinear / coplanar points, a point at
the camera centre, points behind the camera, NaN / inf / 1e150 coordinates, integer pixels, fx / fy = 1e3, H = 1.  Every
output is finite and follows the header's stated answer (tests/pnp_ref.py: check_candidate)."""
import numpy as np
import pytest

import pnp_ref as ref
import pnp_twin as tw

FAMILIES = ref.edge_families()


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_candidate_contract_on_the_twin_and_under_the_sanitizers(name):
    f = FAMILIES[name]
    pose, mask, st = tw.ransac(f["X"], f["px"], f["K"], f["H"], f["threshold"], 3)
    ref.check_candidate(f, pose, mask, st)
    p2, m2, s2 = tw.san_ransac(f["X"], f["px"], f["K"], f["H"], f["threshold"], 3)
    assert np.array_equal(p2, pose) and np.array_equal(m2, mask) and np.array_equal(s2, st)


def test_solver_returns_nothing_on_degenerate_and_non_finite_samples():
    X, x = ref.solver_edge_samples()
    for pose, n in (tw.p3p(X, x), tw.san_p3p(X, x)):
        assert not n.any() and not pose.any()


def test_exact_ties_go_to_the_lower_hypothesis_and_solution():
    f = FAMILIES["integer_px"]
    pose, mask, st, counts = tw.ransac(f["X"], f["px"], f["K"], 64, 1.0, 3, with_counts=True)
    top = counts.max()
    h, r = np.argwhere(counts == top)[0]                                # row-major: the lowest h, then the lowest solution
    assert (st[0], st[1], st[2]) == (top, h, r)
    # a scene with an exact tie by construction: the noise-free candidate, where every all-inlier hypothesis counts n
    g = FAMILIES["h1"]
    pose, mask, st, counts = tw.ransac(g["X"], g["px"], g["K"], 64, 8.0, 3, with_counts=True)
    assert (counts == len(g["X"])).sum() > 1
    h, r = np.argwhere(counts == counts.max())[0]
    assert (st[1], st[2]) == (h, r) and st[0] == len(g["X"])
