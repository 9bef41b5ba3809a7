"""Absolute pose at its edges on the GPU: every family of tests/test_pnp_edges_cpu.py, held to the same stated answer
(tests/pnp_ref.py: check_candidate) and to the host twin of csrc/pnp.hip bit for bit."""
import numpy as np
import pytest

import pnp_ref as ref
import pnp_twin as tw

pytestmark = pytest.mark.gpu
FAMILIES = ref.edge_families()


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_candidate_contract_on_the_device_and_against_the_twin(gpu_ctx, name):
    import slamhip

    f = FAMILIES[name]
    n = len(f["X"])
    pose, mask, st = slamhip.solve_pnp_ransac_offsets(f["X"], f["px"], [0, n], f["K"], f["H"], f["threshold"], 3, ctx=gpu_ctx)
    ref.check_candidate(f, pose[0], mask, st[0])
    pt, mt, stt = tw.ransac(f["X"], f["px"], f["K"], f["H"], f["threshold"], 3)
    assert np.array_equal(pose[0].view(np.uint64), pt.view(np.uint64)) and np.array_equal(mask, mt) and np.array_equal(st[0], stt)


def test_all_families_in_one_batch_equal_their_single_calls(gpu_ctx):
    import slamhip

    names = [k for k in sorted(FAMILIES) if FAMILIES[k]["K"] == ref.EUROC and FAMILIES[k]["H"] == 32 and FAMILIES[k]["threshold"] == 8.0]
    cands = [(FAMILIES[k]["X"], FAMILIES[k]["px"]) for k in names]
    poses, masks, counts, st, _ = slamhip.solve_pnp_ransac_batch(cands, ref.EUROC, 32, 8.0, 3, refine=False, ctx=gpu_ctx)
    for i, k in enumerate(names):
        pt, mt, stt = tw.ransac(FAMILIES[k]["X"], FAMILIES[k]["px"], ref.EUROC, 32, 8.0, 3)
        assert np.array_equal(poses[i].view(np.uint64), pt.view(np.uint64)) and np.array_equal(masks[i], mt) and np.array_equal(st[i], stt), k
    fin = slamhip.solve_pnp_ransac_batch(cands, ref.EUROC, 32, 8.0, 3, refine=True, ctx=gpu_ctx)
    assert np.isfinite(fin[0]).all()                                     # the refinement keeps every pose finite
    for i, k in enumerate(names):
        if st[i, 1] < 0:
            assert np.array_equal(fin[0][i], np.eye(4)[:3]) and fin[4][i] == 0


def test_solver_returns_nothing_on_degenerate_and_non_finite_samples(gpu_ctx):
    import slamhip

    X, x = ref.solver_edge_samples()
    pose, n = slamhip.p3p_arrays(X, x, ctx=gpu_ctx)
    assert not n.any() and not pose.any()
    e, m = slamhip.p3p_arrays(np.zeros((0, 3, 3)), np.zeros((0, 3, 2)), ctx=gpu_ctx)
    assert e.shape == (0, 4, 3, 4) and m.shape == (0,)
