"""The covisibility graph on the device (slamhip.covis, csrc/covis.hip) beside the numpy slamhip.covisibility, and the sparse
bundle adjustment on either, at the two problems of tools/ba_sparse_time.py: BASELINE configs[4] (200 keyframes x 50 000
points) and the map of 2 000 keyframes and 2 * 10^5 points.

Per problem, in ONE session: numpy covisibility; covisibility_device in total (uploads of the observation lists, the three
phases, the allocations between them, the download of edges and weights, the frees) and per phase; bundle_adjust_sparse for
three iterations end to end with covisibility="host" and "device", alternating, with the set-up split into its parts; at
configs[4] bundle_adjust_device beside them.  Every time is a host clock around work that ends in a device synchronise (each phase of the
build ends in a read-back); one warm-up run, then the median of REPS with every run listed.  Needs the GPU; writes to stdout
(kept as profiles/covis_time.log)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "slam-experiments_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ba_sparse_time import INTR, configs4, large_map  # noqa: E402
from slamhip import ba_sparse, covis  # noqa: E402
from slamhip.ba import bundle_adjust_device  # noqa: E402
from slamhip.device import default_context  # noqa: E402

REPS = 5
BA_REPS = 3
clock = time.perf_counter


def med(xs):
    return sorted(xs)[len(xs) // 2]


def listed(xs, unit=1.0, fmt="{:.3f}"):
    return ", ".join(fmt.format(x * unit) for x in sorted(xs))


def timed_ba(ctx, prob_args, mode, iterations, pcg_max_iter):
    """One bundle_adjust_sparse run; the parts of SparseBAProblem's set-up clocked (the device build waits by itself)."""
    T0, X0, op, ol, meas, fixed = prob_args
    spent = {}
    saved = dict(init=ba_sparse.SparseBAProblem.__init__, lists=ba_sparse.observation_lists, vertex=ba_sparse.vertex_lists,
                 build=covis.build_tables, cov=ba_sparse.covisibility)

    def clocked(name, fn, wait=False):
        def run(*a, **kw):
            t = clock()
            out = fn(*a, **kw)
            if wait:
                ctx.sync()
            spent[name] = spent.get(name, 0.0) + clock() - t
            return out
        return run

    try:
        ba_sparse.SparseBAProblem.__init__ = clocked("set-up", saved["init"], wait=True)
        ba_sparse.observation_lists = clocked("observation_lists", saved["lists"])
        ba_sparse.vertex_lists = clocked("vertex_lists", saved["vertex"])
        covis.build_tables = clocked("device covisibility", saved["build"])
        ba_sparse.covisibility = clocked("numpy covisibility", saved["cov"])
        t = clock()
        res, st = ba_sparse.bundle_adjust_sparse(T0, X0, op, ol, meas, INTR, iterations=iterations, fixed_poses=fixed, pcg_max_iter=pcg_max_iter,
                                                 ctx=ctx, covisibility=mode)
        total = clock() - t
    finally:
        ba_sparse.SparseBAProblem.__init__ = saved["init"]
        ba_sparse.observation_lists, ba_sparse.vertex_lists = saved["lists"], saved["vertex"]
        covis.build_tables, ba_sparse.covisibility = saved["build"], saved["cov"]
    return dict(total=total, spent=spent, res=res, st=st)


def report(name, ctx, prob_args, iterations, pcg_max_iter, dense):
    T0, X0, op, ol, meas, fixed = prob_args
    K, L, O = len(T0), len(X0), len(op)
    mask = np.zeros(K, bool)
    mask[list(fixed)] = True

    host = ba_sparse.covisibility(op, ol, K, mask, L)                                # warm-up, and the statement
    t_host = []
    for _ in range(REPS):
        t = clock()
        ba_sparse.covisibility(op, ol, K, mask, L)
        t_host.append(clock() - t)

    tab = covis.covisibility_device(op, ol, K, mask, L, ctx=ctx)                     # warm-up: code objects
    same = all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(tab.download(), host))
    E, P = tab.E, tab.P
    tab.free()
    t_dev, phases = [], []
    for _ in range(REPS):
        ph = {}
        ctx.sync()
        t = clock()
        tab = covis.covisibility_device(op, ol, K, mask, L, ctx=ctx, phases=ph)
        tab.free()
        ctx.sync()
        t_dev.append(clock() - t)
        ph["rest"] = t_dev[-1] - ph["count"] - ph["pairs"] - ph["edges"] - ph["allocations"]
        phases.append(ph)
    plan = covis.plan(K, L, O, P)
    print(f"== {name}: K={K} L={L} O={O}, {E} covisibility edges, {P} pairs ==")
    print(f"numpy covisibility: {med(t_host):.3f} s (median of {REPS}; all: {listed(t_host)})")
    print(f"covisibility_device: {med(t_dev) * 1e3:.2f} ms in total (median of {REPS}; all: {listed(t_dev, 1e3, '{:.2f}')}), "
          f"{med(t_host) / med(t_dev):.1f} x numpy; tables equal to numpy's in every bit: {same}")
    labels = dict(count=f"count (sort of {O} observation keys of {plan['obs_key_bits']} bits in {plan['obs_passes']} passes, point runs, pair scan)",
                  pairs=f"pairs (emit {P} pairs, sort by {plan['pair_key_bits']}-bit keys in {plan['pair_passes']} passes, run heads and their scan)",
                  edges="edges (edges, pair_ptr, weights; download of edges and weights)",
                  allocations="allocations (the two workspaces and the five tables)",
                  rest="rest (upload of the observation lists, the frees)")
    for k, label in labels.items():
        xs = [p[k] for p in phases]
        print(f"  {label}: {med(xs) * 1e3:.2f} ms (all: {listed(xs, 1e3, '{:.2f}')})")
    print(f"  workspaces: count {plan['count_workspace_bytes'] / 2**20:.0f} MiB, pairs {plan['pair_workspace_bytes'] / 2**20:.0f} MiB; "
          f"{P * 16 * (1 + 2 * plan['pair_passes']) / 2**20:.0f} MiB move through the pair sort")

    for mode in ("host", "device"):
        timed_ba(ctx, prob_args, mode, 1, pcg_max_iter)                              # warm-up
    runs = {"host": [], "device": []}
    for _ in range(BA_REPS):
        for mode in ("host", "device"):                                              # alternating
            runs[mode].append(timed_ba(ctx, prob_args, mode, iterations, pcg_max_iter))
    mid = {m: sorted(r, key=lambda x: x["total"])[BA_REPS // 2] for m, r in runs.items()}
    a, b = mid["host"]["res"], mid["device"]["res"]
    equal = a.poses.tobytes() == b.poses.tobytes() and a.points.tobytes() == b.points.tobytes() and mid["host"]["st"] == mid["device"]["st"]
    for mode in ("host", "device"):
        r = mid[mode]
        print(f"bundle_adjust_sparse, covisibility=\"{mode}\", {iterations} iterations: {r['total']:.3f} s end to end (median of {BA_REPS}; all: "
              f"{listed([x['total'] for x in runs[mode]])}), cost {r['res'].chi2_initial:.6g} -> {r['res'].chi2_final:.6g}")
        parts = {k: v for k, v in r["spent"].items() if k != "set-up"}
        other = r["spent"]["set-up"] - sum(parts.values())
        print(f"  set-up {r['spent']['set-up']:.3f} s: " + ", ".join(f"{k} {v * 1e3:.1f} ms ({100 * v / r['total']:.0f} % of the call)" for k, v in parts.items())
              + f", uploads and allocations {other * 1e3:.1f} ms ({100 * other / r['total']:.0f} %); "
              f"the LM trials and the state's round trip {1e3 * (r['total'] - r['spent']['set-up']):.1f} ms")
    print(f"  poses, points and stats of the two equal in every bit: {equal}")
    if dense:
        bundle_adjust_device(T0, X0, op, ol, meas, INTR, iterations=1, fixed_poses=fixed, ctx=ctx)
        times = []
        for _ in range(BA_REPS):
            t = clock()
            d = bundle_adjust_device(T0, X0, op, ol, meas, INTR, iterations=iterations, fixed_poses=fixed, ctx=ctx)
            times.append(clock() - t)
        print(f"bundle_adjust_device, {iterations} iterations: {med(times):.3f} s end to end (median of {BA_REPS}; all: {listed(times)}), "
              f"cost {d.chi2_initial:.6g} -> {d.chi2_final:.6g}; poses differ from the sparse path by {np.abs(d.poses - b.poses).max():.3g}")
        verdict = "WINS over" if mid["device"]["total"] < med(times) else "LOSES to"
        print(f"  the sparse path with covisibility=\"device\" {verdict} bundle_adjust_device here: {mid['device']['total']:.3f} s against {med(times):.3f} s")
    sys.stdout.flush()


if __name__ == "__main__":
    ctx = default_context()
    which = sys.argv[1:] or ["configs4", "large"]
    if "configs4" in which:
        report("BASELINE configs[4]", ctx, configs4(), 3, 500, dense=True)
    if "large" in which:
        report("large map", ctx, large_map(), 3, 5000, dense=False)
