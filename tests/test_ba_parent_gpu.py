"""GPU: the dense and the sparse bundle adjustment return the bits they returned before csrc/ba_common.h and the helpers of
slamhip/ba.py gave them one copy of the code they share.  tests/golden/ba_parent.json was recorded at that parent commit by
tests/golden/make_ba_parent.py; this replays the same calls and asks for equality of every digest and every stat (no
tolerance, no skip).  The kernel-level figures (schur/*, sparse/*) and the whole adjustments are separate keys: where only
the latter differ, the host - the LM schedule or the numpy solve - is the lead.  A different compiler or numpy may round
differently, so a failure prints the recorded and the present ones.  bundle_adjust_one_launch is not retried: SlamHipBusy
fails the case with its message."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_ba_parent as M  # noqa: E402

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
