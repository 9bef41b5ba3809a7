"""GPU: the SE(3) and Sim(3) pose-graph solvers return the bits they returned before csrc/graph_lm.h gave them one copy of the
solver.  tests/golden/graph_solver_parent.json was recorded at that parent commit by tests/golden/make_graph_solver_parent.py;
this replays the same calls and asks for equality of every digest and every stat (no tolerance: "a result is a pure function
of the inputs" includes the bits).  A different compiler may round the libm calls of the edge routines differently, so a
failure prints the recorded and the present toolchain; it does not skip."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_graph_solver_parent as M  # noqa: E402

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
                           f"recorded with: {RECORDED['toolchain']}\nrunning with:  {M.toolchain()}")
