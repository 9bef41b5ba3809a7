"""Stereo / level-weighted adjustments: slam_pose_optimize_stereo_batch_f64 at 1, 16 and 256 frames x 200 edges
(half of them stereo, levels 0..7) beside slam_pose_optimize_batch_f64 on the same points in the same session (the monocular
parent: the ratio is reported, nothing is gated), and the stereo linearise / cost phases of the sparse bundle adjustment beside
slam_bas_linearize_f64 / slam_bas_cost_f64 at the 2 000 x 200 000 map of tools/ba_sparse_time.py.

HIP events (the context's timer) around one call on resident arrays, one warm-up call, then the median of 7 with the spread.
Not measured here: the statement's C twin of the whole optimisation on one host core (the twin covers the edge model only).
Needs the GPU; writes to stdout (kept as profiles/stereo_opt_time.log)."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "slam-experiments_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from slamhip import StereoEdges  # noqa: E402
from slamhip.ba_sparse import SparseBAProblem  # noqa: E402
from slamhip.device import default_context  # noqa: E402
from slamhip.pose_opt import se3_exp  # noqa: E402

FX, FY, CX, CY = 458.654, 457.296, 367.215, 248.375
INTR = (FX, FY, CX, CY)
BF = FX * 0.11
GATES, DELTAS = (5.991, 7.815), (5.991 ** 0.5, 7.815 ** 0.5)
REPS = 7


def timed(ctx, call):
    call()
    ctx.sync()
    ms = []
    for _ in range(REPS):
        ctx.timer_start()
        call()
        ms.append(ctx.timer_stop())
    ms = np.sort(ms)
    return float(np.median(ms)), float(ms[0]), float(ms[-1])


def frames(B, O, rng):
    """B frames of O edges: 0.6 px x scale noise, every seventh edge a gross outlier, even edges stereo."""
    T = np.tile(np.eye(4), (B, 1, 1))
    X = np.c_[rng.uniform(-4, 4, (B * O, 2)), rng.uniform(6, 15, B * O)]
    level = np.arange(B * O) % 8
    sig = 1.2 ** level
    u = FX * X[:, 0] / X[:, 2] + CX
    meas3 = np.stack([u, FY * X[:, 1] / X[:, 2] + CY, u - BF / X[:, 2]], 1) + rng.normal(0, 0.6, (B * O, 3)) * sig[:, None]
    meas3[::7, :2] += 60.0
    meas3[1::2, 2] = np.nan
    T0 = np.stack([se3_exp(rng.normal(0, 0.02, 6)) @ T[b] for b in range(B)])
    return T0[:, :3, :4].reshape(B, 12).copy(), X, meas3, 1.0 / (sig * sig)


def pose_figures(ctx):
    lib, rng = ctx.lib, np.random.default_rng(4)
    print("pose optimisation, 4 rounds x 10 iterations, 200 edges per frame (ms per call: median of 7 [min, max])")
    for B in (1, 16, 256):
        O = 200
        pose, X, meas3, info = frames(B, O, rng)
        off = (np.arange(B + 1) * O).astype(np.int32)
        bufs = [ctx.upload(a) for a in (pose, X, meas3, info, off, np.ascontiguousarray(meas3[:, :2]))]
        d_pose, d_X, d_m3, d_info, d_off, d_m2 = bufs
        outs = [ctx.malloc(B * 96), ctx.malloc(B * O), ctx.malloc(B * O * 8), ctx.malloc(B * 16)]
        bufs += outs
        stereo = lambda: lib.slam_pose_optimize_stereo_batch_f64(ctx.handle, B, d_pose.ptr, d_X.ptr, d_m3.ptr, d_info.ptr, d_off.ptr, B * O, *INTR,  # noqa: E731
                                                                 BF, 4, 10, *GATES, *DELTAS, *[o.ptr for o in outs])
        mono = lambda: lib.slam_pose_optimize_batch_f64(ctx.handle, B, d_pose.ptr, d_X.ptr, d_m2.ptr, d_off.ptr, B * O, *INTR, 4, 10,  # noqa: E731
                                                        5.991 ** 2, 1.0, *[o.ptr for o in outs])
        assert stereo() == 0 and mono() == 0
        s, m = timed(ctx, stereo), timed(ctx, mono)
        print(f"  B={B:4d}: stereo / weighted {s[0]:.3f} [{s[1]:.3f}, {s[2]:.3f}]  monocular parent {m[0]:.3f} [{m[1]:.3f}, {m[2]:.3f}]  "
              f"ratio {s[0] / m[0]:.2f}  ({1e3 * s[0] / B:.1f} us per frame)")
        for b in bufs:
            b.free()


def ba_figures(ctx):
    from ba_sparse_time import large_map

    T0, X0, op, ol, meas, fixed = large_map()
    K, L, O = len(T0), len(X0), len(op)
    rng = np.random.default_rng(9)
    pc = np.einsum("oij,oj->oi", T0[op, :3, :3], X0[ol]) + T0[op, :3, 3]
    ur = meas[:, 0] - BF / pc[:, 2] + rng.normal(0, 0.3, O)
    ur[rng.random(O) < 0.5] = np.nan
    info = 1.0 / 1.2 ** (2 * rng.integers(0, 8, O))
    mask = np.zeros(K, bool)
    mask[list(fixed)] = True
    print(f"sparse bundle adjustment phases at K={K}, L={L}, O={O} (ms per call: median of 7 [min, max])")
    rows = {}
    for name, stereo in (("parent", None), ("stereo / weighted", StereoEdges(np.c_[meas, ur], info, BF))):
        prob = SparseBAProblem(ctx, K, L, op, ol, meas, INTR, mask, stereo=stereo)
        try:
            prob.set_state(T0[:, :3, :4].reshape(K, 12), X0)
            prob.d_T[1].upload(np.ascontiguousarray(T0[:, :3, :4].reshape(K, 12)))
            prob.d_X[1].upload(np.ascontiguousarray(X0))
            c, lib = prob.ctx, prob.ctx.lib
            tail = (prob.d_Hpl.ptr, prob.d_Hll.ptr, prob.d_bl.ptr, prob.d_Hpp.ptr, prob.d_bp.ptr, prob.d_cost.ptr, prob.d_scal.ptr)
            if stereo is None:
                lin = lambda: lib.slam_bas_linearize_f64(c.handle, K, L, O, prob.d_T[0].ptr, prob.d_X[0].ptr, prob.d_op.ptr, prob.d_ol.ptr,  # noqa: E731
                                                         prob.d_meas.ptr, prob.d_pt_ptr.ptr, prob.d_pt_obs.ptr, prob.d_ps_ptr.ptr, prob.d_ps_obs.ptr,
                                                         prob.d_fixed.ptr, *INTR, DELTAS[0], *tail)
                cost = lambda: lib.slam_bas_cost_f64(c.handle, K, L, O, prob.d_T[1].ptr, prob.d_X[1].ptr, prob.d_op.ptr, prob.d_ol.ptr,  # noqa: E731
                                                     prob.d_meas.ptr, prob.d_ps_ptr.ptr, prob.d_ps_obs.ptr, *INTR, DELTAS[0], prob.d_cost2.ptr,
                                                     prob.d_scal.view(24, 8).ptr)
            else:
                lin = lambda: lib.slam_bas_linearize_stereo_f64(c.handle, K, L, O, prob.d_T[0].ptr, prob.d_X[0].ptr, prob.d_op.ptr,  # noqa: E731
                                                                prob.d_ol.ptr, prob.d_meas3.ptr, prob.d_info.ptr, prob.d_pt_ptr.ptr, prob.d_pt_obs.ptr,
                                                                prob.d_ps_ptr.ptr, prob.d_ps_obs.ptr, prob.d_fixed.ptr, *INTR, BF, *DELTAS, *tail)
                cost = lambda: lib.slam_bas_cost_stereo_f64(c.handle, K, L, O, prob.d_T[1].ptr, prob.d_X[1].ptr, prob.d_op.ptr, prob.d_ol.ptr,  # noqa: E731
                                                            prob.d_meas3.ptr, prob.d_info.ptr, prob.d_ps_ptr.ptr, prob.d_ps_obs.ptr, *INTR, BF,
                                                            *DELTAS, prob.d_cost2.ptr, prob.d_scal.view(24, 8).ptr)
            assert lin() == 0 and cost() == 0
            rows[name] = (timed(ctx, lin), timed(ctx, cost))
        finally:
            prob.free()
    for name, (a, b) in rows.items():
        print(f"  {name:18s}: linearise {a[0]:.3f} [{a[1]:.3f}, {a[2]:.3f}]  cost {b[0]:.3f} [{b[1]:.3f}, {b[2]:.3f}]")
    p, s = rows["parent"], rows["stereo / weighted"]
    print(f"  ratio stereo / parent: linearise {s[0][0] / p[0][0]:.2f}, cost {s[1][0] / p[1][0]:.2f}")


def main():
    ctx = default_context()
    name = ctypes.c_char_p(ctx.lib.slam_version()).value.decode()
    try:
        import torch

        name += " on " + torch.cuda.get_device_name(0)
    except Exception:                                            # the figures do not need torch
        pass
    print(f"stereo_opt_time: {name}")
    pose_figures(ctx)
    ba_figures(ctx)


if __name__ == "__main__":
    main()
