"""GPU: the one-launch pose refinements (monocular and stereo / weighted) and the stereo phases of the sparse bundle adjustment
return the bits they returned before csrc/pose_lm_round.inc, csrc/ba_sparse_phases.h and slamhip/_frames.py gave each pair
one copy of its loops.  tests/golden/adjust_parent.json was recorded at that parent commit by tests/golden/make_adjust_parent.py;
this replays the same calls and asks for equality of every digest, every stat and every slam_index_errors count (no tolerance,
no skip).  A different compiler or numpy may round differently, so a failure prints the recorded and the present figures."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_adjust_parent as M  # noqa: E402

pytestmark = pytest.mark.gpu

with open(M.FIXTURE) as _f:
    RECORDED = json.load(_f)


def test_every_case_is_recorded():
    assert sorted(RECORDED["cases"]) == sorted(M.CASES)


@pytest.mark.parametrize("case", M.CASES)
def test_same_bits_as_the_parent(gpu_ctx, case):
    got, want = M.record_case(case, gpu_ctx), RECORDED["cases"][case]
    differing = sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))
    for k in differing:
        print(f"{case} {k}\n  recorded {want.get(k)}\n  got      {got.get(k)}")
    assert not differing, (f"{case}: {len(differing)} of {len(want)} figures differ from the parent's: {differing}\n"
                           f"recorded with: numpy {RECORDED['numpy']}, {RECORDED['toolchain']}\n"
                           f"running with:  numpy {np.__version__}, {M.toolchain()}")
