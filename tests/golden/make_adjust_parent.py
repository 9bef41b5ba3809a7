"""Maker of tests/golden/adjust_parent.json: what the one-launch pose refinements (csrc/pose_opt.hip, csrc/pose_stereo.hip) and
the stereo / weighted phases of the sparse bundle adjustment (csrc/ba_stereo.hip) return, bit for bit, at the commit BEFORE
csrc/pose_lm_round.inc, csrc/ba_sparse_phases.h and slamhip/_frames.py gave each pair one copy of its loops.
tests/test_adjust_parent_gpu.py replays record_case() and compares.  The monocular phases of csrc/ba_sparse.hip are held by
tests/golden/ba_parent.json.

Every input is noisy (not exactly representable), so a sum that is regrouped or a product that is fused anywhere moves a digest.
  pose/oN          a frame of N = 0, 1, 12, 200, 512, 513 edges (512 = SLAM_POSE_STAGE, 513 the first frame on global memory with one
                   chi2 buffer; every frame of tests/stereo_opt_cases.pose_frame has gross outliers at i % 7 == 3, so the active
                   set shrinks between rounds) through slam_pose_optimize_host_f64 and as a batch of one through
                   slam_pose_optimize_batch_f64: Huber 0 and 1, rounds 0 and 4
  pose/batch       frames of 0, 1, 200 and 513 edges in one launch, the same four settings
  stereo_pose/oN   the same sizes with mixed monocular / stereo edges, level informations, informations 0: rounds 0 and 4
  stereo_pose/batch  0, 1, 200, 513 edges and a frame whose edges are all off, in one launch
  stereo_pose/raw  slam_pose_optimize_stereo_batch_f64 itself: one NaN and one negative information; offsets tables that descend
                   and that leave [0, total]
  bas/W/D          W = edges, hub of tests/ba_sparse_ref.py with u_right on about half of the observations, levels 0..7 and every
                   eleventh information 0; D = delta0 (no kernel), default (ORB-SLAM's widths): slam_bas_linearize_stereo_f64 (all
                   blocks), reduce, solve, the step (slam_bas_cost_stereo_f64), the accepted state, slam_bas_classify_stereo_f64,
                   slam_reproj_rj_stereo_f64
  bas/W/poison     one obs_point entry outside its range and one NaN information in the device tables: the same four entry points
  adjust/W         three iterations of bundle_adjust_sparse(stereo=...)
  adjust/local     local_bundle_adjust on tests/stereo_opt_cases.local_window
Arrays are recorded as SHA-256 of their raw bytes, scalars as hex floats, stats as ints, and behind every call the count of
slam_index_errors.

Run on a GPU at that commit, from the repository root: python tests/golden/make_adjust_parent.py"""
import ctypes
import functools
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (HERE, TESTS, ROOT, os.path.join(ROOT, "slam-experiments_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import ba_sparse_ref as R  # noqa: E402
import stereo_opt_cases as C  # noqa: E402
from make_ba_parent import hexed, toolchain  # noqa: E402

FIXTURE = os.path.join(HERE, "adjust_parent.json")
SIZES = (0, 1, 12, 200, 512, 513)
BATCH = (0, 1, 200, 513)
SETTINGS = tuple((h, r) for h in (0.0, 1.0) for r in (0, 4))       # (Huber width, rounds) of the monocular refinement
ROUNDS = (0, 4)
ITERATIONS = 10
WINDOWS = ("edges", "hub")
DELTAS = {"delta0": (0.0, 0.0), "default": (5.991 ** 0.5, 7.815 ** 0.5)}
GATES = (5.991, 7.815)
LM_ITERATIONS = 3
LAM = 1e-3
CASES = tuple([f"pose/o{n}" for n in SIZES] + ["pose/batch"] + [f"stereo_pose/o{n}" for n in SIZES] +
              ["stereo_pose/batch", "stereo_pose/raw"] + [f"bas/{w}/{d}" for w in WINDOWS for d in (*DELTAS, "poison")] +
              [f"adjust/{w}" for w in WINDOWS] + ["adjust/local"])


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def index_errors(ctx):
    """the count since the last look (the call resets it)"""
    n = ctypes.c_int64(0)
    assert ctx.lib.slam_index_errors(ctx.handle, ctypes.byref(n)) == 0
    return n.value


@functools.lru_cache(maxsize=None)
def frame(O):
    """a frame of O edges with planted outliers of both kinds and switched-off edges (seed: 100 + O)"""
    return C.pose_frame(100 + O, O)


@functools.lru_cache(maxsize=None)
def window(name):
    w = {"edges": R.case_edges, "hub": R.case_hub}[name]()
    meas3, info = C.stereo_window(w, 5 + WINDOWS.index(name))
    info = np.where(np.arange(len(info)) % 11 == 3, 0.0, info)
    return w, meas3, info


def pose_result(r, ctx, chi2_written=True):
    """chi2_written False: with rounds = 0 a frame beyond SLAM_POSE_STAGE leaves d_chi2 as the caller's buffer was (the staged
    form stores zeros, the global-memory form makes no evaluation): whatever the allocation held is no figure of the parent"""
    return " ".join([sha(r.pose), sha(r.inliers.astype(np.uint8)), sha(r.chi2) if chi2_written else "-", str(r.n_inliers), str(r.iterations),
                     str(index_errors(ctx))])


def result(r):
    return " ".join([sha(r.poses), sha(r.points), float(r.chi2_initial).hex(), float(r.chi2_final).hex(), str(r.iterations)])


def record_pose(sizes, ctx):
    from slamhip.pose_opt import optimize_pose_only_device, optimize_poses_batch

    fr = [frame(n) for n in sizes]
    out = {}
    for huber, rounds in SETTINGS:
        key = f"huber{huber:g}/rounds{rounds}"
        kw = dict(rounds=rounds, iterations=ITERATIONS, huber_delta=huber, ctx=ctx)
        if len(fr) == 1:
            f = fr[0]
            r = optimize_pose_only_device(f["T_init"], f["X"], f["meas3"][:, :2], R.INTR, **kw)
            out[f"host/{key}"] = pose_result(r, ctx, rounds > 0 or len(f["X"]) <= 512)
            if len(f["X"]) == 200 and rounds and huber:       # the walk over trials 1..9 ran: every round ends on rejected trials
                assert 0 < r.iterations < rounds * ITERATIONS and r.n_inliers < 200, (r.iterations, r.n_inliers)
        res = optimize_poses_batch(np.stack([f["T_init"] for f in fr]), [f["X"] for f in fr], [f["meas3"][:, :2] for f in fr], R.INTR, **kw)
        for b, r in enumerate(res):
            out[f"batch/{key}/frame{b}"] = pose_result(r, ctx, rounds > 0 or len(fr[b]["X"]) <= 512)
    return out


def record_stereo_pose(sizes, ctx, all_off=False):
    from slamhip import StereoEdges, optimize_poses_stereo

    fr = [frame(n) for n in sizes]
    if all_off:
        fr.append(dict(frame(200), info=np.zeros(200)))
    out = {}
    for rounds in ROUNDS:
        st = []
        res = optimize_poses_stereo(np.stack([f["T_init"] for f in fr]), [f["X"] for f in fr], [StereoEdges(f["meas3"], f["info"], C.BF) for f in fr],
                                    R.INTR, C.BF, rounds=rounds, iterations=ITERATIONS, ctx=ctx, stats_out=st)
        for b, r in enumerate(res):
            out[f"rounds{rounds}/frame{b}"] = pose_result(r, ctx) + " " + " ".join(str(int(v)) for v in st[0][b])
    return out


def record_stereo_raw(ctx):
    """four frames cut from the 513-edge frame by the caller's own table"""
    f = frame(513)
    O = 513
    pose = np.tile(f["T_init"][:3, :4].reshape(12), (4, 1))
    info = f["info"].copy()
    info[10], info[300] = -1.0, np.nan
    bufs = [ctx.upload(pose), ctx.upload(f["X"]), ctx.upload(f["meas3"]), ctx.upload(info), ctx.malloc(4 * 96), ctx.malloc(O), ctx.malloc(O * 8),
            ctx.malloc(64)]
    d_pose, d_pts, d_mes, d_inf, d_out, d_inl, d_chi, d_st = bufs
    out = {}
    try:
        for name, table in (("sane", [0, 60, 260, 261, 513]), ("descends", [0, 60, 30, 700, 513]), ("leaves", [-7, 60, 260, 1 << 30, 513])):
            for rounds in ROUNDS:
                for b, n in ((d_out, 4 * 96), (d_inl, O), (d_chi, O * 8), (d_st, 64)):
                    b.upload(np.zeros(n, np.uint8))               # what no frame owns stays as it was: make that a known value
                d_off = ctx.upload(np.array(table, np.int32))
                try:
                    assert ctx.lib.slam_pose_optimize_stereo_batch_f64(ctx.handle, 4, d_pose.ptr, d_pts.ptr, d_mes.ptr, d_inf.ptr, d_off.ptr, O,
                                                                       *R.INTR, C.BF, rounds, ITERATIONS, *GATES, *DELTAS["default"], d_out.ptr,
                                                                       d_inl.ptr, d_chi.ptr, d_st.ptr) == 0
                    ctx.sync()
                finally:
                    d_off.free()
                out[f"{name}/rounds{rounds}"] = " ".join([sha(d_out.download(np.float64, (4, 12))), sha(d_inl.download(np.uint8, (O,))),
                                                           sha(d_chi.download(np.float64, (O,))),
                                                           " ".join(str(int(v)) for v in d_st.download(np.int32, (16,))), str(index_errors(ctx))])
    finally:
        for b in bufs:
            b.free()
    return out


def record_bas(name, mode, ctx):
    import slamhip.ba_sparse as bs
    from slamhip import StereoEdges
    from slamhip.pose_graph import DEFAULT_PCG_MAX_ITER

    w, meas3, info = window(name)
    delta = DELTAS["default" if mode == "poison" else mode]
    K, L, O = len(w["T0"]), len(w["X0"]), len(w["op"])
    T12 = np.ascontiguousarray(w["T0"][:, :3, :4]).reshape(K, 12)
    fixed = np.zeros(K, bool)
    fixed[list(w["fixed"])] = True
    out = {}
    prob = bs.SparseBAProblem(ctx, K, L, w["op"], w["ol"], None, R.INTR, fixed, stereo=StereoEdges(meas3, info, C.BF))
    c = ctx
    try:
        prob.set_state(T12, w["X0"])
        if mode == "poison":
            ol, bad = np.ascontiguousarray(w["ol"], np.int32).copy(), info.copy()
            ol[O // 3] = L + 5
            bad[O // 2] = np.nan
            prob.d_ol.upload(ol)
            prob.d_info.upload(bad)
        index_errors(ctx)
        cost, dmax = prob.linearize(delta)
        blocks = [prob.d_Hpl.download(np.float64, (O, 18)), prob.d_Hll.download(np.float64, (L, 6)), prob.d_bl.download(np.float64, (L, 3)),
                  prob.d_Hpp.download(np.float64, (K, 21)), prob.d_bp.download(np.float64, (K, 6)), prob.d_cost.download(np.float64, (K,))]
        out["linearize"] = " ".join([float(cost).hex(), float(dmax).hex(), *(sha(a) for a in blocks), str(index_errors(ctx))])
        assert c.lib.slam_bas_cost_stereo_f64(c.handle, K, L, O, prob.d_T[0].ptr, prob.d_X[0].ptr, prob.d_op.ptr, prob.d_ol.ptr, prob.d_meas3.ptr,
                                              prob.d_info.ptr, prob.d_ps_ptr.ptr, prob.d_ps_obs.ptr, *R.INTR, C.BF, *delta, prob.d_cost2.ptr,
                                              prob.d_scal.view(24, 8).ptr) == 0
        out["cost"] = " ".join([float(prob.d_scal.download(np.float64, (4,))[3]).hex(), sha(prob.d_cost2.download(np.float64, (K,))),
                                str(index_errors(ctx))])
        chi2, inl = prob.classify(*GATES)
        out["classify"] = " ".join([sha(chi2), sha(inl.astype(np.uint8)), str(int(inl.sum())), str(index_errors(ctx))])
        rj = [c.malloc(O * n * 8) for n in (3, 18, 9, 1, 1)]
        try:
            assert c.lib.slam_reproj_rj_stereo_f64(c.handle, prob.d_T[0].ptr, K, prob.d_X[0].ptr, L, prob.d_op.ptr, prob.d_ol.ptr, prob.d_meas3.ptr,
                                                   prob.d_info.ptr, O, *R.INTR, C.BF, *delta, *(b.ptr for b in rj)) == 0
            out["rj"] = " ".join([*(sha(b.download(np.float64, (O * n,))) for b, n in zip(rj, (3, 18, 9, 1, 1))), str(index_errors(ctx))])
        finally:
            for b in rj:
                b.free()
        if mode != "poison":                                      # (a poisoned system has no step worth recording)
            prob.reduce(LAM)
            out["reduced_system"] = " ".join(sha(a) for a in prob.reduced_system())
            st = prob.solve(LAM, bs.DEFAULT_PCG_TOL, DEFAULT_PCG_MAX_ITER)
            out["solve"] = " ".join([sha(prob.d_dp.download(np.float64, (K, 6))), hexed(st)])
            out["step"] = " ".join(float(v).hex() for v in prob.step(LAM, delta))
            prob.accept()
            out["accepted_state"] = " ".join(sha(a) for a in prob.state())
            chi2, inl = prob.classify(*GATES)
            out["classify_accepted"] = " ".join([sha(chi2), sha(inl.astype(np.uint8)), str(index_errors(ctx))])
    finally:
        prob.free()
    return out


def record_adjust(name, ctx):
    import slamhip.ba_sparse as bs
    from slamhip import StereoEdges, local_bundle_adjust

    if name == "local":
        w = C.local_window()
        res, outliers, st = local_bundle_adjust(w["T0"], w["X0"], w["op"], w["ol"], StereoEdges(w["meas3"], w["info"], C.BF), R.INTR,
                                                fixed_poses=w["fixed"], first=3, second=3, ctx=ctx)
        return {"local_bundle_adjust": " ".join([result(res), sha(outliers.astype(np.int64)), hexed(st), str(index_errors(ctx))])}
    w, meas3, info = window(name)
    out = {}
    for mode, delta in DELTAS.items():
        res, st = bs.bundle_adjust_sparse(w["T0"], w["X0"], w["op"], w["ol"], None, R.INTR, iterations=LM_ITERATIONS, fixed_poses=w["fixed"],
                                          huber_delta=delta, ctx=ctx, stereo=StereoEdges(meas3, info, C.BF))
        out[f"bundle_adjust_sparse/{mode}"] = " ".join([result(res), hexed(st), str(index_errors(ctx))])
    return out


def record_case(case, ctx):
    """every recorded figure of one case as {name: str}"""
    index_errors(ctx)
    group, _, rest = case.partition("/")
    if group == "bas":
        return record_bas(*rest.split("/"), ctx)
    if group == "adjust":
        return record_adjust(rest, ctx)
    if rest == "raw":
        return record_stereo_raw(ctx)
    sizes = BATCH if rest == "batch" else (int(rest[1:]),)
    return record_pose(sizes, ctx) if group == "pose" else record_stereo_pose(sizes, ctx, all_off=rest == "batch")


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
