"""Maker of tests/golden/graph_solver_parent.json: what the SE(3) and Sim(3) pose-graph solvers return, bit for bit, at the
commit BEFORE csrc/graph_lm.h gave the two of them one copy of the solver.  tests/test_graph_solver_parent_gpu.py replays
record() and compares.

Per graph: linearisation (cost, gradient, H diagonal, W, status) with Huber 0 and 3; the product of a seeded random x at
lambda = 0 and 1e-3; PCG (PCG_ITERATIONS, which is more than one read of the done flag); the full optimisation
(LM_ITERATIONS; Sim(3) with fix_scale 0 and 1).  Arrays are recorded as SHA-256 of their raw bytes, scalars and the
returned stats as hex floats.  The noisy scenes are the point: their values are not exactly representable, so a sum that is
regrouped anywhere changes a digest, which the exactly-stated graphs cannot see.

Run on a GPU at that commit, from the repository root: python tests/golden/make_graph_solver_parent.py"""
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
for p in (TESTS, os.path.join(os.path.dirname(TESTS), "slam-experiments_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import pose_graph_ref as P  # noqa: E402
import pose_graph_truth as T  # noqa: E402
import sim3_graph_ref as R  # noqa: E402

FIXTURE = os.path.join(HERE, "graph_solver_parent.json")
SE3_SCENES = ("sphere", "loop_closure", "hub")
SE3_EXACT = ("deg0_13", "hub_degrees", "V41", "E65")
SIM3_SCENES = ("drift_loop", "hub", "sphere_s1")
CASES = tuple(f"se3/{n}" for n in SE3_SCENES + SE3_EXACT) + tuple(f"sim3/{n}" for n in SIM3_SCENES)
LM_ITERATIONS = 3
PCG_ITERATIONS = 80
X_SEED = 77


def toolchain():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    try:
        return subprocess.run([hipcc, "--version"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError) as err:
        return f"hipcc --version failed: {err}"


@functools.lru_cache(maxsize=None)
def graph(case):
    """(initial vertices, edges, meas, info, fixed) of one case"""
    kind, name = case.split("/")
    if kind == "sim3":
        s = R.SMALL_SCENES[name]()
        return s.init, s.edges, s.meas, s.info, s.fixed
    if name in P.SMALL_SCENES:
        s = P.SMALL_SCENES[name]()
        return s.init, s.edges, s.meas, s.info, s.fixed
    g = {g.name: g for g in T.exact_graphs(big=False)}[name]
    return g.poses, g.edges, g.meas, g.info, g.masks[0]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float64).tobytes()).hexdigest()


def hexed(stats):
    return {k: float(v).hex() for k, v in stats.items()}


def record_case(case, ctx):
    """every recorded figure of one case as {name: str}"""
    import slamhip

    se3 = case.startswith("se3/")
    lin = slamhip.pose_graph_linearize if se3 else slamhip.sim3_graph_linearize
    mul = slamhip.pose_graph_hmul if se3 else slamhip.sim3_graph_hmul
    pcg = slamhip.pose_graph_pcg if se3 else slamhip.sim3_graph_pcg
    opt = slamhip.optimize_pose_graph if se3 else slamhip.optimize_sim3_graph
    init, edges, meas, info, fixed = graph(case)
    out = {}
    for huber in (0.0, 3.0):
        cost, b, Hd, W, status = lin(init, edges, meas, info, huber, ctx=ctx)
        out[f"linearize/huber{huber:g}"] = " ".join([float(cost).hex(), sha(b), sha(Hd), sha(W), str(status)])
    cost, b, Hd, W, status = lin(init, edges, meas, info, 0.0, ctx=ctx)
    x = np.random.default_rng(X_SEED).normal(size=b.shape)
    for lam in (0.0, 1e-3):
        out[f"hmul/lam{lam:g}"] = sha(mul(edges, fixed, Hd, W, lam, x, ctx=ctx))
    sol, st = pcg(edges, fixed, Hd, W, b, 1e-3, tol=1e-8, max_iter=PCG_ITERATIONS, ctx=ctx)
    out["pcg"] = " ".join([sha(sol), json.dumps(hexed(st), sort_keys=True)])
    for kw in ({"huber_delta": 0.0}, {"huber_delta": 3.0}) if se3 else ({"fix_scale": False}, {"fix_scale": True}):
        res, st = opt(init, edges, meas, info, fixed, iterations=LM_ITERATIONS, ctx=ctx, **kw)
        key = "optimize/" + ",".join(f"{k}={v:g}" for k, v in kw.items())
        out[key] = " ".join([sha(res), json.dumps(hexed(st), sort_keys=True)])
    return out


def main():
    import slamhip

    ctx = slamhip.default_context()
    doc = {"toolchain": toolchain(), "cases": {case: record_case(case, ctx) for case in CASES}}
    with open(FIXTURE, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {FIXTURE}: {len(CASES)} cases, {sum(len(c) for c in doc['cases'].values())} figures")


if __name__ == "__main__":
    main()
