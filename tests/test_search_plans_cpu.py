"""CPU suite: the planners of the top-k, radius and window searches return, value for value, what tests/golden/search_plans.json
holds - a recording of slam_bf_topk_plan_describe, slam_bf_radius_plan_describe and slam_bf_window_plan_describe made by
tests/golden/make_search_plans.py before the three files were given one copy of the chunk rule.  The planner tests of
test_topk_cpu.py, test_radius_cpu.py and test_window_cpu.py assert invariants only; this one pins the numbers.  It never
writes the file."""
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(HERE, "golden", "search_plans.json")) as f:
        return json.load(f)


def test_the_recording_covers_the_grid(recorded):
    """4 CU counts x (13 shapes x 9 k, 15 shapes, 11 shapes x 6 cell caps), no argument tuple twice"""
    for name, count in (("topk", 4 * 13 * 9), ("radius", 4 * 15), ("window", 4 * 11 * 6)):
        args = [tuple(a) for a, _ in recorded[name]]
        assert len(args) == count and len(set(args)) == count, name
        assert {a[0] for a in args} == {1, 80, 256, 304}
    assert {a[3] for a, _ in recorded["topk"]} == {1, 2, 4, 5, 8, 9, 16, 17, 32}
    assert {a[3] for a, _ in recorded["window"]} == {0, 1, 4, 37, 8464, 1 << 20}


def test_topk_plans_are_the_recorded_ones(built, recorded):
    import slamhip

    for (cu, n, m, k), plan in recorded["topk"]:
        assert list(slamhip.plan_describe_topk(n, m, k, num_cu=cu).values()) == plan, (cu, n, m, k)


def test_radius_plans_are_the_recorded_ones(built, recorded):
    import slamhip

    for (cu, n, m), plan in recorded["radius"]:
        assert list(slamhip.plan_describe_radius(n, m, num_cu=cu).values()) == plan, (cu, n, m)


def test_window_plans_are_the_recorded_ones(built, recorded):
    import slamhip

    for (cu, n, m, cells), plan in recorded["window"]:
        assert list(slamhip.plan_describe_window(n, m, cells=cells, num_cu=cu).values()) == plan, (cu, n, m, cells)
