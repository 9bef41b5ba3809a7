"""CPU: the launch shape of the one-launch window bundle adjustment (slam_ba_optimize_shape needs no device).

The rule (bg_shape, csrc/ba_schur.hip): ntask = K + n_free (n_free + 1) / 2 pose and pair tasks; blocks = max(ceil(O / 512),
ntask) clamped to [8, 128]; every task cut into blocks / ntask slices, clamped to [1, 8].  The corners are pinned with
literal values, so that a retune of the rule fails here and in tests/test_ba_limits_gpu.py, whose cases sit on them."""
import itertools

import pytest


def shape(K, O, n_free):
    from slamhip.ba import one_launch_shape

    return one_launch_shape(K, O, n_free)


@pytest.mark.parametrize("K,O,n_free,want", [
    (2, 40, 1, (8, 2)),            # the 8-block floor: 3 tasks, 8 // 3 = 2 slices
    (2, 0, 0, (8, 4)),             # no observations at all: still the floor
    (2, 131072, 1, (128, 8)),      # the 128-workgroup cap and the 8-slice cap (128 // 3 = 42)
    (3, 24064, 2, (47, 7)),        # one short of 8 slices for 6 tasks ...
    (3, 24065, 2, (48, 8)),        # ... and the first size that reaches them
    (4, 40000, 3, (79, 7)),        # a slice count that is not a power of two (ceil(40000 / 512) = 79, 10 tasks)
    (64, 10000, 16, (128, 1)),     # 200 tasks on 128 workgroups: one slice, several tasks per workgroup
    (64, 131072, 16, (128, 1)),
    (64, 131072, 0, (128, 2)),     # no pair tasks: 64 pose tasks in two slices
    (16, 200, 15, (128, 1)),       # 136 tasks: more than the cap
    (7, 5792, 6, (28, 1)),         # the reference's window of 7 keyframes: one workgroup per task
])
def test_shape_at_the_corners_of_the_rule(built, K, O, n_free, want):
    assert shape(K, O, n_free) == want


@pytest.mark.parametrize("K,O,n_free,what", [
    (65, 10, 1, "bad sizes"),               # more than 64 poses (sT[64 * 12], s_ps_ptr[65] in LDS)
    (0, 10, 0, "bad sizes"),
    (20, 10, 17, "at most 16 free poses"),  # more than SLAM_BA_LM_MAX_FREE moving poses
    (3, 10, 4, "at most 16 free poses"),    # more moving poses than poses
    (2, 10, -1, "at most 16 free poses"),
    (2, 131073, 1, "bad sizes"),            # SLAM_BA_LM_MAX_OBS + 1
    (2, -1, 1, "bad sizes"),
])
def test_shape_refuses_what_the_launch_refuses(built, K, O, n_free, what):
    with pytest.raises(ValueError, match=what):
        shape(K, O, n_free)


def test_shape_agrees_with_the_launch_limits(built):
    """Every window at the limits gets a shape; the ones one past them get none (the same checks as slam_ba_optimize_f64)."""
    for K, O, n_free in ((64, 131072, 16), (1, 0, 0), (1, 0, 1), (16, 131072, 16)):
        shape(K, O, n_free)
    for K, O, n_free in ((65, 131072, 16), (64, 131073, 16), (64, 131072, 17)):
        with pytest.raises(ValueError):
            shape(K, O, n_free)


def test_shape_invariants_over_a_sweep(built):
    """Over a sweep of windows: 8 <= blocks <= 128; 1 <= slices <= 8; blocks cover every task or sit at the cap; the slices
    of all tasks fit in the launch; the launch is as wide as the observations ask for (512 each) up to the cap."""
    for K, n_free, O in itertools.product((1, 2, 3, 5, 7, 16, 17, 33, 64), (0, 1, 2, 3, 6, 11, 16),
                                          (0, 1, 40, 511, 512, 513, 4095, 24065, 40000, 65536, 131071, 131072)):
        if n_free > K:
            continue
        ntask = K + n_free * (n_free + 1) // 2
        blocks, slices = shape(K, O, n_free)
        assert 8 <= blocks <= 128 and 1 <= slices <= 8, (K, O, n_free)
        assert blocks >= min(ntask, 128) and blocks >= min(-(-O // 512), 128), (K, O, n_free)
        assert blocks == max(8, min(128, max(ntask, -(-O // 512)))), (K, O, n_free)
        if ntask <= blocks:
            assert slices * ntask <= blocks and (slices == 8 or (slices + 1) * ntask > blocks), (K, O, n_free)
        else:
            assert slices == 1, (K, O, n_free)
