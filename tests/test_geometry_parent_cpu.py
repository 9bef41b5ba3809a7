"""The host twins of the four batched RANSAC estimators (two_view, pnp, homography, sim3) return the bits they returned before
csrc/geometry_common.h gave the four kernel files one copy of the sampler, the Jacobi sweeps, the triangulation, the
cheirality test, the range clamp and the model keys.  The `twin` section of tests/golden/geometry_parent.json was recorded at
that parent commit by tests/golden/make_geometry_parent.py; this replays the same calls and asks for equality of every digest
and every stat (no tolerance, no skip).  A different compiler or numpy may round differently, so a failure prints the recorded
and the present figures and what both were made with."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_geometry_parent as M  # noqa: E402

SECTION = "twin"

with open(M.FIXTURE) as _f:
    RECORDED = json.load(_f)[SECTION]


def test_the_section_was_recorded_at_the_parent_and_is_complete():
    assert RECORDED["commit"].startswith(M.PARENT)
    assert sorted(RECORDED["cases"]) == sorted(M.CASES[SECTION])
    assert all(not k.startswith("clamp/") for c in RECORDED["cases"].values() for k in c)      # the twins take no offsets


@pytest.mark.parametrize("case", M.CASES[SECTION])
def test_same_bits_as_the_parent(built, case):
    M.compare(case, M.record_case(case), RECORDED["cases"][case], RECORDED)
