"""Maker of tests/golden/ba_parent.json: what the bundle-adjustment paths return, bit for bit, at the commit BEFORE
csrc/ba_common.h and slamhip/ba.py's shared helpers gave the dense (ba_schur.hip) and the sparse (ba_sparse.hip) path one copy
of the code they share.  tests/test_ba_parent_gpu.py replays record_case() and compares.

Windows, all noisy (their values are not exactly representable, so a sum that is regrouped anywhere changes a digest):
  smallest  `smallest` of tests/ba_sparse_ref.py: K = 3, 25 observations.  one_launch_shape gives it (8, 2), so it is also the
            smallest window of the existing helpers with more than one workgroup and more than one slice per task
  uneven    `uneven` of the same file: K = 7, (73, 4) - more tasks, four slices, lists of every awkward length; taken as well
            because the two-slice case above cuts lists of 1 and 12 entries only
  edges     case_edges of tests/ba_sparse_ref.py: K = 23, edges of 1 and of 130 pairs, unseen points, a free pose without
            observations
  hub       case_hub: K = 41, 780 edges
Each with Huber 0 and 1.  Per window and Huber: SchurProblem.reduce at lambda = 1e-3 (S, rhs, bp, cost), back_substitute of a
seeded random dp, cost, diag_max; SparseBAProblem.linearize, reduce -> reduced_system, solve (step and stats), step, the
candidate after accept(); LM_ITERATIONS of bundle_adjust_device, bundle_adjust_sparse (result and stats),
bundle_adjust_one_launch where the window is inside its limits, and bundle_adjust on `smallest`.  Arrays are recorded as
SHA-256 of their raw bytes, scalars and stats as hex floats.

Run on a GPU at that commit, from the repository root: python tests/golden/make_ba_parent.py  (there `smallest` and `uneven`
were _smallest and _uneven of tests/test_ba_limits_gpu.py: the same text, the same draws)."""
import functools
import hashlib
import json
import os
import shutil
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (TESTS, ROOT, os.path.join(ROOT, "slam-experiments_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import ba_sparse_ref as R  # noqa: E402

FIXTURE = os.path.join(HERE, "ba_parent.json")
WINDOWS = ("smallest", "uneven", "edges", "hub")
HUBERS = (0.0, 1.0)
CASES = tuple(f"{w}/huber{h:g}" for w in WINDOWS for h in HUBERS)
LM_ITERATIONS = 3
LAM = 1e-3
X_SEED = 77


def toolchain():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    try:
        return subprocess.run([hipcc, "--version"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError) as err:
        return f"hipcc --version failed: {err}"


@functools.lru_cache(maxsize=None)
def window(name):
    if name == "smallest":
        return R.smallest(np.random.default_rng(8))
    if name == "uneven":
        return R.uneven(np.random.default_rng(37002))
    return {"edges": R.case_edges, "hub": R.case_hub}[name]()


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float64).tobytes()).hexdigest()


def hexed(stats):
    return json.dumps({k: float(v).hex() for k, v in stats.items()}, sort_keys=True)


def result(r):
    return " ".join([sha(r.poses), sha(r.points), float(r.chi2_initial).hex(), float(r.chi2_final).hex(), str(r.iterations)])


def record_case(case, ctx):
    """every recorded figure of one case as {name: str}"""
    import slamhip.ba as ba
    import slamhip.ba_sparse as bs
    from slamhip.pose_graph import DEFAULT_PCG_MAX_ITER

    name, huber = case.split("/huber")
    huber = float(huber)
    w = window(name)
    K, L = len(w["T0"]), len(w["X0"])
    T12 = np.ascontiguousarray(w["T0"][:, :3, :4]).reshape(K, 12)
    fixed = np.zeros(K, bool)
    fixed[list(w["fixed"])] = True
    out = {}

    prob = ba.SchurProblem(ctx, K, L, w["op"], w["ol"], w["meas"], R.INTR)
    try:
        S, rhs, bp, cost = prob.reduce(T12, w["X0"], huber, LAM)
        out["schur/reduce"] = " ".join([sha(S), sha(rhs), sha(bp), float(cost).hex()])
        dl, bl = prob.back_substitute(1e-3 * np.random.default_rng(X_SEED).normal(size=(K, 6)))
        out["schur/back_substitute"] = " ".join([sha(dl), sha(bl)])
        out["schur/diag_max"] = float(prob.diag_max(np.flatnonzero(~fixed))).hex()
        out["schur/cost"] = float(prob.cost(T12, w["X0"], huber)).hex()
    finally:
        prob.free()

    prob = bs.SparseBAProblem(ctx, K, L, w["op"], w["ol"], w["meas"], R.INTR, fixed)
    try:
        prob.set_state(T12, w["X0"])
        out["sparse/linearize"] = " ".join(float(v).hex() for v in prob.linearize(huber))
        prob.reduce(LAM)
        out["sparse/reduced_system"] = " ".join(sha(a) for a in prob.reduced_system())
        st = prob.solve(LAM, bs.DEFAULT_PCG_TOL, DEFAULT_PCG_MAX_ITER)
        out["sparse/solve"] = " ".join([sha(prob.d_dp.download(np.float64, (K, 6))), hexed(st)])
        out["sparse/step"] = " ".join(float(v).hex() for v in prob.step(LAM, huber))
        prob.accept()
        out["sparse/accepted_state"] = " ".join(sha(a) for a in prob.state())
    finally:
        prob.free()

    args = (w["T0"], w["X0"], w["op"], w["ol"], w["meas"], R.INTR)
    kw = dict(iterations=LM_ITERATIONS, fixed_poses=w["fixed"], huber_delta=huber, ctx=ctx)
    out["bundle_adjust_device"] = result(ba.bundle_adjust_device(*args, **kw))
    res, st = bs.bundle_adjust_sparse(*args, **kw)
    out["bundle_adjust_sparse"] = " ".join([result(res), hexed(st)])
    try:
        ba.one_launch_shape(K, len(w["op"]), K - int(fixed.sum()))
    except ValueError:
        pass                                                  # outside the one-launch form's limits: nothing to record
    else:
        out["bundle_adjust_one_launch"] = result(ba.bundle_adjust_one_launch(*args, **kw))    # SlamHipBusy is a failure, not retried
    if name == "smallest":
        out["bundle_adjust"] = result(ba.bundle_adjust(*args, **kw))
    return out


def main():
    import slamhip

    ctx = slamhip.default_context()
    doc = {"toolchain": toolchain(), "numpy": np.__version__, "cases": {case: record_case(case, ctx) for case in CASES}}
    with open(FIXTURE, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {FIXTURE}: {len(CASES)} cases, {sum(len(c) for c in doc['cases'].values())} figures")


if __name__ == "__main__":
    main()
