"""GPU: every entry point of csrc/two_view.hip, pnp.hip, homography.hip and sim3.hip returns the bits it returned before
csrc/geometry_common.h gave the four files one copy of the code they share.  The `gpu` section of
tests/golden/geometry_parent.json was recorded on an MI355X at that parent commit by tests/golden/make_geometry_parent.py
through the public slamhip API; this replays the same calls - the minimal solvers on 65 samples, each RANSAC on four
candidates for three hypothesis counts and two seeds, an offsets table that leaves [0, M) with the index-error count it
leaves, and what follows the RANSAC on its winners - and asks for equality of every digest and every stat (no tolerance, no
skip).  A failure prints the recorded and the present figures and what both were made with."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_geometry_parent as M  # noqa: E402

pytestmark = pytest.mark.gpu
SECTION = "gpu"

with open(M.FIXTURE) as _f:
    RECORDED = json.load(_f)[SECTION]


def test_the_section_was_recorded_at_the_parent_and_is_complete():
    assert RECORDED["commit"].startswith(M.PARENT)
    assert sorted(RECORDED["cases"]) == sorted(M.CASES[SECTION])
    assert all(any(k.startswith("clamp/") for k in c) for c in RECORDED["cases"].values())     # every file's range clamp is pinned


@pytest.mark.parametrize("case", M.CASES[SECTION])
def test_same_bits_as_the_parent(gpu_ctx, case):
    M.compare(case, M.record_case(case, gpu_ctx), RECORDED["cases"][case], RECORDED)
