#!/usr/bin/env python3
"""bench.py — headline benchmark: descriptor pairs/sec, brute-force Hamming knn=2 at 64k x 64k.

    python bench.py --gpus N --steps K --warmup W [--workload 64k|loop-closure] [--dump-outputs DIR] [--full]

A "step" is one pass of the hot path over one batch: all 65536 query descriptors matched
(knn=2) against 65536 train descriptors, inputs resident in HBM before the timed region.
At N > 1 there is one process per GPU: the query rows are sharded across ranks, every rank
holds the 2 MiB train set, and each step ends with the RCCL all-gather of the per-shard top-2
rows, so every rank owns the full result (strong scaling: the total work is fixed).

`python bench.py --gpus N` is self-contained: with no WORLD_SIZE in the environment it starts
the N rank processes itself (before anything touches a GPU).  Under the driver's launcher
(`python -m torch.distributed.run ... bench.py --gpus N`) the ranks already exist and only their
RANK / LOCAL_RANK / WORLD_SIZE / MASTER_PORT variables are read.  Either way the rendezvous, the
barriers and the max-over-ranks are `slamhip.launch` (a Unix socket, standard library): no torch,
no MPI on the control or the data path; the data path is libslamhip.so + librccl.

--workload loop-closure is BASELINE configs[3]: 512 keyframes x 2048 descriptors matched all-to-all (2^20 x 2^20 pairs per
step), the query keyframes sharded over the ranks (64 per rank at 8 GPUs), the 32 MiB train collection replicated (over
the fabric with slam_comm_broadcast when RCCL is up, by per-rank upload otherwise), the per-shard top-2 rows all-gathered
and decoded on the device to OpenCV's multi-image form (imgIdx, trainIdx, distance).  The default workload stays 64k x 64k.

A plain run sets up, warms up, times the K steps and prints ONE JSON line from rank 0: the contract fields (`ms_per_step`
is the wall time of one timed step in milliseconds) and
  roofline      — the dominant kernel (bf_top2_kernel) against the HBM roofline on ALGORITHMIC
                  bytes, as the contract asks, plus the VALU-integer figures that actually bound it
                  (from the timed steps and the committed PMC summary: no run of its own).
--dump-outputs DIR writes the tables the last timed step computed, as a caller receives them, to DIR/<name>.npy in
float32 (row indices and distances are integers below 2^24: exact): train_idx and distance [n_query, 2], and img_idx for
the loop-closure workload (24 MiB in all there).  The inputs come from fixed seeds, so two builds compare output for output.
--full adds, after the timed region, everything else the benchmark measures or checks:
  parity_spot_check — 256 sampled rows of the last timed step against the CPU oracle (null in a plain run);
  cpu_baseline  — the CPU oracle (oracle/bf_hamming_oracle.c, a port: cv2 is not installable
                  here) timed on the host cores over the same arrays (N = 1 only; --no-cpu-baseline skips it);
  pipelined     — with --pipelined: the same searches issued alternately on two contexts (N = 1 only; reported, not `value`);
  reproj        — the second hot path (residual/Jacobian build, 200 poses x 50k points dense)
                  with its own HBM roofline (N = 1, default workload only; --no-reproj skips it);
  next_rows     — the rows SURVEY.md 8f marks "next", as the calls a frame loop makes: one pose-only refinement (200 edges)
                  and one window bundle adjustment at the reference's window, each beside the same loop in plain C on
                  one host core and checked against it (N = 1 only; reported, not `value`; --no-next-rows skips it).
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: required for multi-process RCCL on this pool
if int(os.environ.get("WORLD_SIZE", "1")) > 1:
    os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")       # single node: bootstrap over loopback, no NIC needed
    os.environ.setdefault("NCCL_IB_DISABLE", "1")           # ... and no InfiniBand probing; the data path is xGMI P2P
ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(ROOT, "slam-experiments_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

N_QUERY = 65536
N_TRAIN = 65536
LC_KEYFRAMES, LC_ROWS = 512, 2048   # loop closure, BASELINE configs[3]
HBM_PEAK_GBS = 8000.0             # MI355X HBM3E spec (MI355X_MICROARCH.md)
VALU_LANES_PER_S = 256 * 4 * 32 * 2.4e9   # 256 CU x 4 SIMD x 32 lanes x 2.4 GHz (nominal clock: a fraction of this can never exceed 1)
OPS_PER_PAIR = 16                 # 8 v_xor + 8 v_bcnt per 256-bit pair (algorithmic minimum, no MFMA)
# A gfx950 SIMD executes a wave64 VALU instruction in 4 cycles and runs two at once when they come from different waves
# and at most one of them is a v_bcnt (measured in shader cycles, tools/ubench/cycles.hip, profiles/r03_ubench_cycles.log):
# 16 instructions per wave-row cannot take fewer than 16 x 4 / 2 = 32 cycles per SIMD - the same bound as the 32-lane peak.
DUAL_ISSUE_CYCLES_PER_ROW = 16 * 4 / 2
SPIN_UP_PASSES = 24               # the GPU needs ~10 passes (~20 ms) of load before DVFS reaches its steady clock (tools/ramp.py)
HBM_COUNTERS = os.path.join(ROOT, "profiles", "hbm_counters.json")   # tools/profile.sh refreshes it; stamped with the kernel source hashes
KERNEL_SOURCES = {"bf_top2_kernel": ("bf_hamming.hip", "bf_scan_sgpr.h"), "reproj_rj_kernel": ("reproj.hip",)}


def source_sha(name: str) -> str:
    with open(os.path.join(ROOT, "slam-experiments_amd", "csrc", name), "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def profiled_traffic(kernel: str):
    """(HBM-side bytes per launch of `kernel`, where they come from) from the committed rocprofv3 PMC passes, or
    (None, why not).

    PMC counters cannot be collected from inside this process; the separate FETCH_SIZE / WRITE_SIZE passes over this
    same command are summarised (with the gfx950 corrections) by tools/pmc_summary.py, which stamps the file with the
    hashes of the kernel sources it was collected on.  A stamp that no longer matches the sources means the numbers
    describe an older kernel: they are then withheld instead of printed."""
    try:
        with open(HBM_COUNTERS) as f:
            rec = json.load(f)
        for src in KERNEL_SOURCES[kernel]:
            want, have = rec["source_sha"][src], source_sha(src)
            if want != have:
                return None, f"{os.path.relpath(HBM_COUNTERS, ROOT)} was collected on {src} {want}, the source is now {have}"
        return float(rec[kernel]["traffic_bytes"]), (f"{os.path.relpath(HBM_COUNTERS, ROOT)} (rocprofv3 PMC, separate passes, N=1 launch, "
                                                      f"sources {', '.join(KERNEL_SOURCES[kernel])} unchanged since)")
    except (OSError, KeyError, ValueError) as exc:
        return None, f"no usable PMC summary ({type(exc).__name__}: {exc})"


def make_descriptors(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)


DUMP_LIMIT_BYTES = 64 << 20


def write_outputs(out_dir: str, arrays: dict) -> None:
    """--dump-outputs: each array as <out_dir>/<name>.npy in float32; refuses values float32 cannot hold exactly and more
    than DUMP_LIMIT_BYTES in all."""
    conv = {name: np.ascontiguousarray(a, dtype=np.float32) for name, a in arrays.items()}
    for name, a in conv.items():
        if not np.array_equal(a.astype(arrays[name].dtype), arrays[name]):
            raise ValueError(f"--dump-outputs: {name} does not convert to float32 exactly")
    total = sum(a.nbytes for a in conv.values())
    if total > DUMP_LIMIT_BYTES:
        raise ValueError(f"--dump-outputs: {total} bytes, the limit is {DUMP_LIMIT_BYTES}")
    os.makedirs(out_dir, exist_ok=True)
    for name, a in conv.items():
        np.save(os.path.join(out_dir, f"{name}.npy"), a)


def launch_plan(ctx, n: int, m: int) -> dict:
    """The plan the search runs for n x m on this device (slam_bf_plan_info + what only slam_bf_plan_describe tells: whether it is
    a queue plan - `workers` resident blocks per query block draw the chunks by ticket - and how its workers exchange bounds)."""
    import slamhip

    plan = ctx.plan_info(n, m)
    more, _ = slamhip.plan_describe(n, m, num_cu=plan["cus"])
    plan.update(workers=more["workers"], merge_exchange=more["merge"], resident_blocks_per_cu=more["resident"])
    return plan


def cpu_baseline(query: np.ndarray, train: np.ndarray) -> dict:
    """Oracle (CPU port of the cv2 path) on a bounded sample of the same workload, all host cores."""
    from oracle import oracle

    cores = os.cpu_count() or 1
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        pass
    available = cores
    cores = min(cores, 16)                          # the one-GPU box's CPU share (said in the line when it bites: cores_capped_from)
    # 65536 x 65536: the whole workload (~15-20 core-seconds of popcnt per pass); loop closure: the first 65536 query rows
    # against the whole 2^20-row collection (the same cost per query row as the full job, 1/16 of its rows)
    rows = min(query.shape[0], max(4096, int(2 ** 36 // max(train.shape[0], 1))))
    q = query[:rows]
    oracle.bf_knn_c(q[:256], train, 2, threads=cores)   # page in / spin up the OpenMP team
    dt = float("inf")
    for _ in range(3):                               # best of 3: ~20 core-seconds in total
        t0 = time.perf_counter()
        oracle.bf_knn_c(q, train, 2, threads=cores)
        dt = min(dt, time.perf_counter() - t0)
    cv2_leg = "cv2 is not installed on this host"
    cv2_out = None
    try:                                             # the reference's own backend, only where it exists
        import cv2

        rows_cv = 4096
        t0 = time.perf_counter()
        cv2.BFMatcher(cv2.NORM_HAMMING).knnMatch(q[:rows_cv], train, k=2)
        dtc = time.perf_counter() - t0
        cv2_out = {"value": rows_cv * train.shape[0] / dtc, "unit": "pairs/s", "threads": cv2.getNumThreads(),
                   "sample": f"cv2.BFMatcher(NORM_HAMMING).knnMatch, first {rows_cv} query rows x {train.shape[0]}, {dtc:.2f} s"}
        cv2_leg = f"cv2 {cv2.__version__} timed separately (field cv2)"
    except ImportError:
        pass
    one_rows = 4096                                  # 1 thread on a 1/16 slice of the query rows: a few seconds
    t0 = time.perf_counter()
    oracle.bf_knn_c(q[:one_rows], train, 2, threads=1)
    dt1 = time.perf_counter() - t0
    return {"value": rows * train.shape[0] / dt, "unit": "pairs/s", "cores": cores, "cores_capped_from": available if available > cores else None,
            "kind": "port", "cv2": cv2_out,
            "single_thread": {"value": one_rows * train.shape[0] / dt1, "unit": "pairs/s",
                              "sample": f"first {one_rows} query rows x {train.shape[0]}, {dt1:.2f} s"},
            "sample": f"{'all' if rows == query.shape[0] else 'the first'} {rows} query rows x {train.shape[0]} train rows (the same arrays), oracle/bf_hamming_oracle.c "
                      f"(gcc -O3, {oracle.bf_simd()}, OpenMP {cores} threads), best of 3 = {dt:.2f} s wall; {cv2_leg}"}


def reproj_cpu_baseline(poses, points, obs_pose, obs_point, meas, intr) -> dict:
    """Oracle (f64 C loop restating frontend.py:272-291) on all 1e7 observations, all cores and one thread."""
    from oracle import oracle

    cores = min(len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1), 16)
    n = obs_pose.shape[0]
    sl = slice(0, n)
    args = (poses, points, obs_pose[sl], obs_point[sl], meas[sl], *intr)
    out = oracle.reproj_rj_c(*args, with_point=True, threads=cores)     # page in; the output arrays are reused below
    best = {}
    for threads in (cores, 1):
        dt = float("inf")
        for _ in range(3):
            t0 = time.perf_counter()
            oracle.reproj_rj_c(*args, with_point=True, threads=threads, out=out)
            dt = min(dt, time.perf_counter() - t0)
        best[threads] = dt
    return {"value": n / best[cores], "unit": "observations/s", "cores": cores, "kind": "port",
            "single_thread": {"value": n / best[1], "unit": "observations/s"},
            "sample": f"all {n} observations (the same arrays), oracle/reproj_oracle.c (gcc -O3, OpenMP {cores} threads), "
                      f"best of 3 = {best[cores]:.3f} s ({best[1]:.3f} s on one thread) into preallocated outputs"}


def reproj_bench(ctx, steps: int, warmup: int, cpu: bool = True) -> dict:
    """BASELINE configs[4]: 200 keyframes x 50k landmarks, dense 1e7 observations, residual + both Jacobians."""
    import slamhip

    rng = np.random.default_rng(228)
    K, L = 200, 50000
    O = K * L
    ang = rng.uniform(-0.3, 0.3, (K, 3))
    poses = np.zeros((K, 12))
    for k in range(K):                                   # small-angle rotations, translations in a 10 m box
        wx, wy, wz = ang[k]
        W = np.array([[0, -wz, wy], [wz, 0, -wx], [-wy, wx, 0]])
        th = np.linalg.norm(ang[k]) + 1e-12
        Rm = np.eye(3) + np.sin(th) / th * W + (1 - np.cos(th)) / th**2 * (W @ W)
        poses[k] = np.c_[Rm, rng.uniform(-5, 5, 3)].reshape(12)
    points = np.c_[rng.uniform(-10, 10, (L, 2)), rng.uniform(8, 30, L)]
    obs_pose = np.repeat(np.arange(K, dtype=np.int32), L)
    obs_point = np.tile(np.arange(L, dtype=np.int32), K)
    meas = rng.uniform(0, 752, (O, 2)).astype(np.int32).astype(np.float64)   # int-truncated pixels (primitives.py:110-112)
    prob = slamhip.ReprojProblem(ctx, poses, points, obs_pose, obs_point, meas,
                                 (458.654, 457.296, 367.215, 248.375), with_point=True)
    for _ in range(SPIN_UP_PASSES * 4 + warmup):         # same clock spin-up as the matcher gets (a pass is 0.27 ms here)
        prob.linearize()
    ctx.sync()
    ctx.timer_start()
    for _ in range(steps):
        prob.linearize()
    ms = ctx.timer_stop() / steps
    prob.free()
    bytes_per_obs = 4 + 4 + 16 + 16 + 96 + 48           # two indices + pixel read; e, J_pose, J_point written
    kernel_ms = ms                                       # one event pair around the back-to-back launches, / launches (see main)
    gbs = O * bytes_per_obs / (kernel_ms * 1e-3) / 1e9
    traffic, traffic_source = profiled_traffic("reproj_rj_kernel")
    out = {"workload": "200 poses x 50000 points dense = 1e7 observations, e + J_pose(2x6) + J_point(2x3), f64",
           "observations_per_s": O / (ms * 1e-3), "ms_per_step": ms, "kernel_ms": kernel_ms,
           "roofline": {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": gbs / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_source,
                        "bytes_per_observation": bytes_per_obs}}
    if cpu:
        out["cpu_baseline"] = reproj_cpu_baseline(poses, points, obs_pose, obs_point, meas,
                                                  (458.654, 457.296, 367.215, 248.375))
    return out


def next_rows_leg(ctx, cpu: bool = True) -> dict:
    """SURVEY.md 8f rows f3 / f4 beside one host core: the pose-only refinement of one frame (200 edges, the whole
    `_correct_current_pose` schedule in one launch, frontend.py:298-393) and a window bundle adjustment at the reference's
    window (7 keyframes, backend.py:11; five LM steps in one launch), each as the host-buffer call a frame loop would make,
    with the plain-C statement of the same loop (oracle/pose_lm_oracle.c, oracle/ba_lm_oracle.c: test infrastructure, the
    CPU baseline of these rows) timed on ONE core and compared with what the GPU returned.  Not part of `value`."""
    sys.path.insert(0, os.path.join(ROOT, "slam-experiments_amd"))
    from backend import Backend
    from slamhip.ba import bundle_adjust_one_launch
    from slamhip.pose_opt import se3_exp
    from scipy.spatial.transform import Rotation

    fx, fy, cx, cy = 458.654, 457.296, 367.215, 248.375
    rng = np.random.default_rng(2026)
    best = lambda f, n: min(_timed(f) for _ in range(n))
    out = {}
    # f3: one frame, 200 edges, every ninth a gross outlier, integer pixels as the reference's keypoints are
    E = 200
    X = np.c_[rng.uniform(-4, 4, (E, 2)), rng.uniform(6, 15, E)]
    pix = np.c_[fx * X[:, 0] / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy] + rng.normal(0, 0.3, (E, 2))
    pix[::9] += 70.0
    pix = pix.astype(np.int32).astype(np.float64)
    T0 = se3_exp([0.01, -0.01, 0.005, 0.05, -0.03, 0.04])
    be = Backend()
    call = lambda: be.optimize_pose(T0, X, pix, fx, fy, cx, cy, on_device=True)
    r = call()
    out["pose_lm"] = {"edges": E, "ms_per_call": best(call, 20) * 1e3, "accepted_steps": int(r.iterations), "inliers": int(r.n_inliers),
                      "call": "Backend.optimize_pose (slam_pose_optimize_host_f64: the kernel reads and writes the pinned block, one launch, completion polled)"}
    if cpu:
        from oracle import oracle
        p12 = np.ascontiguousarray(T0[:3, :4].reshape(12))
        ref = lambda: oracle.pose_lm_c(p12, X, pix, fx, fy, cx, cy)
        Tc, inl_c, _, _ = ref()
        out["pose_lm"]["cpu_baseline"] = {"ms_per_call": best(ref, 10) * 1e3, "cores": 1, "kind": "port", "sample": "the same frame, oracle/pose_lm_oracle.c"}
        out["pose_lm"]["parity"] = bool(np.abs(r.pose[:3, :4] - np.asarray(Tc).reshape(-1)[:12].reshape(3, 4)).max() <= 1e-7 and np.array_equal(np.asarray(r.inliers, bool), np.asarray(inl_c, bool)))
    # f4: the reference's window
    K, L = 7, 1400
    T = np.tile(np.eye(4), (K, 1, 1))
    T[:, :3, :3] = Rotation.from_rotvec(rng.uniform(-0.15, 0.15, (K, 3))).as_matrix()
    T[:, :3, 3] = rng.uniform(-0.5, 0.5, (K, 3))
    P = np.c_[rng.uniform(-4, 4, (L, 2)), rng.uniform(6, 15, L)]
    op = np.repeat(np.arange(K), L).astype(np.int32); ol = np.tile(np.arange(L), K).astype(np.int32)
    keep = rng.uniform(size=K * L) < 0.6
    op, ol = op[keep], ol[keep]
    pc = np.einsum("oij,oj->oi", T[op, :3, :3], P[ol]) + T[op, :3, 3]
    meas = np.c_[fx * pc[:, 0] / pc[:, 2] + cx, fy * pc[:, 1] / pc[:, 2] + cy] + rng.normal(0, 0.2, (len(op), 2))
    Ts = np.stack([T[0], T[1]] + [se3_exp(rng.normal(0, 0.01, 6)) @ T[k] for k in range(2, K)])
    Ps = P + rng.normal(0, 0.05, P.shape)
    call = lambda: bundle_adjust_one_launch(Ts, Ps, op, ol, meas, (fx, fy, cx, cy), iterations=5, fixed_poses=(0, 1), ctx=ctx)
    r = call()
    out["window_ba"] = {"poses": K, "points": L, "observations": int(len(op)), "lm_steps": int(r.iterations), "ms_per_call": best(call, 20) * 1e3,
                        "cost": [float(r.chi2_initial), float(r.chi2_final)],
                        "call": "bundle_adjust_one_launch (slam_ba_optimize_host_f64: index tables, one upload, one launch, one download)"}
    if cpu:
        from oracle import oracle
        p0 = np.ascontiguousarray(Ts[:, :3, :4]).reshape(K, 12)
        ref = lambda: oracle.ba_lm_c(p0, Ps, op, ol, meas, fx, fy, cx, cy, 5, (0, 1), 0.0)
        Tc, Xc, _, c1, acc, _ = ref()
        out["window_ba"]["cpu_baseline"] = {"ms_per_call": best(ref, 5) * 1e3, "cores": 1, "kind": "port", "sample": "the same window, oracle/ba_lm_oracle.c"}
        out["window_ba"]["parity"] = bool(acc == r.iterations and abs(c1 - r.chi2_final) <= 1e-9 * max(c1, 1.0) and np.abs(r.poses - Tc).max() <= 1e-8
                                          and np.abs(r.points - Xc).max() <= 1e-7)
    return out


def _timed(f) -> float:
    t0 = time.perf_counter()
    f()
    return time.perf_counter() - t0


def pipelined_leg(query, train, steps: int) -> dict:
    """The same 64k x 64k searches issued alternately on two contexts of the one GPU (two streams, two merge states):
    the drain of one launch overlaps the start of the next.  Reported beside `value`, never as `value`: the contract's
    roofline is per kernel launch, and overlapped launches stretch each other."""
    import slamhip

    ctxs = [slamhip.Context(0 if os.environ.get("SLAM_BENCH_SINGLE_DEVICE") == "1" else int(os.environ.get("LOCAL_RANK", "0")))
            for _ in range(2)]
    sets = []
    for c in ctxs:
        sets.append((c, slamhip.DeviceDescriptors(c, query), slamhip.DeviceDescriptors(c, train), slamhip.Top2Table(c, N_QUERY)))

    def one(i):
        c, dq, dt, tab = sets[i & 1]
        slamhip.knn2_device(c, dq.buf, N_QUERY, dt.buf, N_TRAIN, tab.idx, tab.dist)

    for i in range(SPIN_UP_PASSES):
        one(i)
    for c in ctxs:
        c.sync()
    t0 = time.perf_counter()
    for i in range(steps):
        one(i)
    for c in ctxs:
        c.sync()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    a, b = sets[0][3].download(), sets[1][3].download()
    same = bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))
    for c, dq, dt, tab in sets:
        for o in (tab, dq, dt):
            o.free()
        c.close()
    return {"value": float(N_QUERY) * N_TRAIN / (ms * 1e-3), "unit": "pairs/s", "ms_per_step": ms, "steps": steps,
            "streams": 2, "tables_identical": same,
            "note": "searches alternate between two contexts (streams) of the same GPU; wall time / steps"}


def bench_line(*, world, steps, warmup, loop_closure, n_query, n_train, n_local, wall_ms, dev_ms, rank_kernel_ms, launches,
               collective, fallback_reason, rccl_version, plan, ok, train_replication) -> dict:
    """The JSON line of a run from its measurements (pure: the CPU suite checks its schema and invariants without a GPU)."""
    ms_per_step = wall_ms / steps
    pairs = float(n_query) * float(n_train)
    value = pairs / (ms_per_step * 1e-3)
    kernel_ms = max(rank_kernel_ms)                             # the slowest rank's shard kernel bounds the step
    local_pairs = float(n_local) * n_train                      # pairs one launch of the dominant kernel covers
    alg_bytes = 32.0 * (n_local + n_train) + 16.0 * n_local     # each descriptor read once, top-2 written once
    achieved = alg_bytes / (kernel_ms * 1e-3) / 1e9
    lane_ops = local_pairs * OPS_PER_PAIR / (kernel_ms * 1e-3)
    floor_ms = local_pairs / 64 * DUAL_ISSUE_CYCLES_PER_ROW / (256 * 4) / 2.4e9 * 1e3
    if world == 1 and not loop_closure:
        traffic, traffic_source = profiled_traffic("bf_top2_kernel")
    else:
        traffic, traffic_source = None, "PMC passes are collected on the default command only (N=1, 64k x 64k)"
    if loop_closure:
        metric = "descriptor pairs/sec BF-Hamming knn=2 loop-closure 512x2k all-to-all"
        workload = (f"loop closure: {LC_KEYFRAMES} keyframes x {LC_ROWS} synthetic random 256-bit descriptors (rng seed 228) matched "
                    f"all-to-all = 2^20 x 2^20 pairs per step, BF-Hamming knn=2 over the collection, result as "
                    f"(imgIdx, trainIdx, distance) (BASELINE configs[3])")
        sharding = (f"query keyframes / {world} ({LC_KEYFRAMES // world if LC_KEYFRAMES % world == 0 else 'about ' + str(LC_KEYFRAMES // world)} per rank), "
                    f"train collection replicated ({train_replication}), all-gather of top-2, decode on every rank") if world > 1 else "single GPU"
    else:
        metric = "descriptor pairs/sec BF-Hamming knn=2 @64kx64k"
        workload = ("65536x65536 synthetic random 256-bit descriptors (rng seeds 228/229), "
                    "BF-Hamming knn=2 (BASELINE configs[2])")
        sharding = f"query rows / {world}, train replicated, all-gather of top-2" if world > 1 else "single GPU"
    return {
        "metric": metric,
        "value": value, "unit": "pairs/s", "n_gpus": world, "steps": steps, "warmup": warmup,
        "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": "u32", "data": "synthetic",
        "config": {"workload": workload, "n_query": n_query, "n_train": n_train, "sharding": sharding,
                   "collective": collective, "collective_fallback_reason": fallback_reason,
                   "rccl_version": rccl_version, "launch_plan": plan},
        "device_ms_per_step": dev_ms / steps,
        "parity_spot_check": ok,
        "roofline": {
            "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": achieved / HBM_PEAK_GBS,
            "traffic": traffic, "traffic_source": traffic_source,
            "kernel": "bf_top2_kernel", "kernel_ms": kernel_ms, "launches": launches,
            "kernel_ms_per_rank": {"min": min(rank_kernel_ms), "max": max(rank_kernel_ms)},
            "algorithmic_bytes_per_launch": alg_bytes,
            "note": "contractual HBM figure on algorithmic bytes; the kernel is VALU-integer bound "
                    "(1.2e-3 B/pair), see valu_int",
            "valu_int": {"lane_ops_per_pair": OPS_PER_PAIR, "achieved_lane_ops_per_s": lane_ops,
                         "peak_lane_ops_per_s": VALU_LANES_PER_S, "frac_of_32lane_peak": lane_ops / VALU_LANES_PER_S,
                         "issue_floor_ms": floor_ms, "frac_of_issue_floor": floor_ms / kernel_ms,
                         "issue_model": "16 wave64 VALU instructions per wave-row, 4 cycles each, two issue slots per SIMD "
                                        "(one v_bcnt + one other at a time; measured in shader cycles, tools/ubench/cycles.hip), "
                                        "at the NOMINAL 2.4 GHz: wall-clock fractions, at most 1 by construction; the in-kernel "
                                        "clock and the cycles per wave-row at that clock are in profiles/ (tools/cycle_probe.py)"}},
    }


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", choices=("64k", "loop-closure"), default="64k",
                    help="64k: 65536 x 65536 (BASELINE configs[2], the headline); loop-closure: 512 keyframes x 2048 rows "
                         "all-to-all (BASELINE configs[3])")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the tables of the last timed step to DIR/<name>.npy (float32)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run the oracle spot check, the CPU baselines, the residual kernel and the "
                         "'next' rows (the options below trim this)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-reproj", action="store_true")
    ap.add_argument("--no-next-rows", action="store_true", help="skip the pose-refinement / window-BA calls (SURVEY 8f rows f3, f4)")
    ap.add_argument("--pipelined", action="store_true",
                    help="with --full: also time the searches alternating between two contexts (extra object `pipelined`; "
                         "off by default so that a rocprofv3 summary of the default command only holds back-to-back launches)")
    ap.add_argument("--no-pipelined", action="store_true", help=argparse.SUPPRESS)   # accepted for older command lines
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.pipelined and not args.full:
        ap.error("--pipelined is a leg of --full")

    from slamhip.launch import Rendezvous, from_env, spawn_ranks

    if args.gpus > 1 and int(os.environ.get("WORLD_SIZE", "1")) == 1 and "SLAM_RDZV" not in os.environ:
        # self-contained launch: this parent never touches a GPU, it starts one process per rank and relays rank 0's line
        return spawn_ranks(os.path.abspath(__file__), sys.argv[1:], args.gpus)

    rank, local_rank, world, rdzv_name = from_env()
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    rz = Rendezvous(rank, world, rdzv_name or "single")

    import ctypes

    import slamhip
    from slamhip.dist import ShardedMatcher, init_comm

    # SLAM_BENCH_SINGLE_DEVICE=1 (tests on a 1-GPU box): every rank uses GPU 0
    ctx = slamhip.Context(0 if os.environ.get("SLAM_BENCH_SINGLE_DEVICE") == "1" else local_rank)
    loop_closure = args.workload == "loop-closure"
    if loop_closure:
        # every keyframe's rows are query AND train: the collection is searched with itself (each row finds itself at
        # distance 0 first, its true nearest neighbour second - the case a loop-closure detector then has to skip)
        n_query = n_train = LC_KEYFRAMES * LC_ROWS
        query = train = make_descriptors(n_query, 228)
        image_rows = [LC_ROWS] * LC_KEYFRAMES
    else:
        n_query, n_train = N_QUERY, N_TRAIN
        query, train = make_descriptors(N_QUERY, 228), make_descriptors(N_TRAIN, 229)
        image_rows = None

    def barrier():
        ctx.sync()
        rz.barrier()

    collective = "none"
    rccl_ok = False
    fallback_reason = None
    rccl_version = ctypes.c_int(0)
    if ctx.lib.slam_comm_version(ctypes.byref(rccl_version)) != 0:
        rccl_version = None
    # A multi-rank RCCL communicator has never run on the boxes this was developed on (one GPU each; RCCL refuses ranks that
    # share a device), so its set-up and its first collective round run under a deadline: a bootstrap that waits for a rank
    # that will not come, or a collective on a fabric that does not answer, becomes a labelled fall-back to the next tier
    # instead of a run that hangs until somebody kills it.  After a deadline the native call is still running in its helper
    # thread: the communicator and the context whose stream holds the collective are abandoned (nothing is destroyed), the
    # rest of the run uses a fresh context, and the process leaves with os._exit once the line is out.
    deadline = float(os.environ.get("SLAM_BENCH_DEADLINE", "90"))
    fake_hang = os.environ.get("SLAM_BENCH_FAKE_HANG", "")     # test hook: "init" / "step" - rank 1 never returns from that call
    abandoned = False
    sm = None
    device_index = 0 if os.environ.get("SLAM_BENCH_SINGLE_DEVICE") == "1" else local_rank
    if world > 1:
        # RCCL is the data path.  If its communicator cannot be created on this node, say so loudly and use the
        # library's own direct all-gather over xGMI peer mappings (HIP IPC); if that cannot be set up either,
        # gather through the host, so that a scaling number - labelled as such - still exists.
        from slamhip.dist import call_with_deadline

        force = os.environ.get("SLAM_BENCH_COLLECTIVE", "")    # test hook: "p2p" / "host" skip the tiers above them
        os.environ.setdefault("NCCL_DEBUG", "WARN")            # a failing communicator says why on stderr
        try:
            if force in ("p2p", "host"):
                raise RuntimeError(f"skipped: SLAM_BENCH_COLLECTIVE={force}")
            if fake_hang == "init" and rank == 1:
                rz.bcast(None)                                 # takes part in the id exchange, then "never returns"
                call_with_deadline(lambda: time.sleep(1e6), deadline, "ncclCommInitRank (simulated hang)")
            else:
                init_comm(ctx, rank, world, rz.bcast, deadline=deadline)
            failed = None
        except Exception as exc:   # noqa: BLE001 - any failure of the native init
            failed = f"rccl: {type(exc).__name__}: {exc}"
            print(f"[bench] rank {rank}: RCCL communicator init failed ({exc}); trying peer copies over HIP IPC", file=sys.stderr)
        verdicts = rz.allgather(failed)                        # every rank reaches this collective on every path
        rccl_ok = not any(verdicts)
        if rccl_ok:
            # the communicator exists everywhere: prove it with the first pass (train broadcast, search, all-gather, sync)
            def first_round():
                m = ShardedMatcher(ctx, rank, world, query, train, collective="rccl", broadcast_train=loop_closure,
                                   image_rows=image_rows)
                if fake_hang == "step" and rank == 1:
                    time.sleep(1e6)
                m.step()
                ctx.sync()
                return m

            try:
                sm = call_with_deadline(first_round, deadline, "the first RCCL all-gather")
                failed = None
            except Exception as exc:   # noqa: BLE001
                failed = f"rccl: {type(exc).__name__}: {exc}"
                print(f"[bench] rank {rank}: the first RCCL round failed ({exc}); trying peer copies over HIP IPC", file=sys.stderr)
            verdicts = rz.allgather(failed)
            rccl_ok = not any(verdicts)
        if not rccl_ok:
            fallback_reason = "; ".join(f"rank {r}: {v}" for r, v in enumerate(verdicts) if v)
            abandoned = any(v and "did not return within" in v for v in verdicts)
            sm = None
            if abandoned:
                # somebody is still inside a native call: nothing RCCL touched is reused or destroyed (the old context is
                # simply left alone: it has no finaliser, and the process leaves through os._exit)
                ctx = slamhip.Context(device_index)
            else:
                ctx.lib.slam_comm_destroy(ctx.handle)

    if sm is None:
        sm = ShardedMatcher(ctx, rank, world, query, train, collective=None, broadcast_train=False, image_rows=image_rows)
    host_gather = False
    if world > 1 and rccl_ok:
        collective = "rccl"
    elif world > 1 and os.environ.get("SLAM_BENCH_COLLECTIVE") != "host" and sm.enable_p2p(rz.allgather, barrier):
        collective = "xgmi-p2p-copies"
    elif world > 1:
        collective = "host-fallback"
        why = getattr(sm, "p2p_error", "marker check failed" if os.environ.get("SLAM_BENCH_COLLECTIVE") != "host" else "skipped: SLAM_BENCH_COLLECTIVE=host")
        fallback_reason = f"{fallback_reason}; p2p: {why}"
        print(f"[bench] rank {rank}: peer mapping failed too ({why}); gathering through the host", file=sys.stderr)
        host_gather = True

    device_step = sm.step

    def step():
        device_step()
        if host_gather:
            mine = sm.gathered[sm.last].view(rank * sm.slot_bytes, sm.slot_bytes).download(np.uint8, (sm.slot_bytes,))
            sm.gathered[sm.last].upload(np.concatenate(rz.allgather(mine)))   # every rank ends up with the full table on its device
        if loop_closure:
            if collective == "xgmi-p2p-copies":
                barrier()                                      # the peers' copies into this rank's buffer have landed
            sm.decode_images()                                 # global train row -> (imgIdx, trainIdx), on the device

    # device spin-up, not part of the measurement (see SPIN_UP_PASSES; a loop-closure pass is 0.3 s of load by itself)
    # The kernel's average launch duration is taken from ONE pair of HIP events around the K timed launches on the stream
    # the kernel runs on (ctx.timer_start / timer_stop), divided by K: back-to-back launches leave no gap on that stream
    # (8192 x 65536: 152.0 us per step = the kernel; 64k x 64k: 1053.1 us), whereas an event pair around EVERY launch costs
    # 7-10 us per step and stretches the kernel it brackets (159.5 us per step and 154.5 us "per kernel"; 1063.7 and
    # 1058.7 us) - 5 % of a 1/8-shard step.  The figure is an upper bound of the launch duration (it contains whatever gap
    # there is), which is the conservative side for a roofline fraction.
    # (the COUNT is the same on every rank - a pass contains a collective - and covers ~30 ms of load whatever the shard
    # size: at eight ranks a pass is 0.15 ms, and 24 of them would end before the clock has settled)
    spin_up = 2 if loop_closure else max(SPIN_UP_PASSES, int(0.030 / (float(sm.per) * n_train / 3.5e12)) + 1)
    for _ in range(spin_up):
        step()
    barrier()
    for _ in range(args.warmup):
        step()
    barrier()
    # The timed bracket: device synchronised and all ranks aligned on both sides.  The alignment inside the bracket is the
    # shared-memory barrier (a few microseconds); the socket barrier is a round trip per rank through rank 0 - 0.63 ms at
    # eight ranks, a sixth of twenty 0.16 ms shard steps - and stays outside, where its robustness is wanted.
    rz.spin_barrier()
    t0 = time.perf_counter()
    ctx.timer_start()
    for _ in range(args.steps):
        step()
    dev_ms = ctx.timer_stop()          # HIP events on the stream the kernels run on; synchronises (both streams: slam_sync)
    ctx.sync()
    rz.spin_barrier()
    wall_ms = (time.perf_counter() - t0) * 1e3
    barrier()
    launches = args.steps
    my_kernel_ms = dev_ms / max(launches, 1)

    times = rz.allgather((wall_ms, dev_ms, my_kernel_ms))      # MAX over ranks
    wall_ms, dev_ms = max(t[0] for t in times), max(t[1] for t in times)
    rank_kernel_ms = [t[2] for t in times]

    # what the last timed step computed: the full table on every rank; dumped by rank 0, spot-checked against the oracle there
    # with --full (parity_spot_check stays null in a plain run)
    if args.full or args.dump_outputs:
        if loop_closure:
            img, local, dist_tab = sm.result_images()
            outputs = {"img_idx": img, "train_idx": local, "distance": dist_tab}
        else:
            idx, dist_tab = sm.result()
            outputs = {"train_idx": idx, "distance": dist_tab}
        if rank == 0 and args.dump_outputs:
            write_outputs(args.dump_outputs, outputs)
    ok = None
    if rank == 0 and args.full:
        from oracle import oracle

        sel = np.random.default_rng(1).choice(n_query, 256, replace=False)
        if loop_closure:
            # the oracle's multi-image search (imgIdx << 18 | trainIdx encoding, OpenCV matchers.cpp) over the 512 images
            rimg, rlocal, rdist = oracle.bf_knn_multi_c(query[sel], [train[i * LC_ROWS:(i + 1) * LC_ROWS] for i in range(LC_KEYFRAMES)], 2,
                                                        threads=os.cpu_count() or 1)
            ok = bool(np.array_equal(img[sel], rimg) and np.array_equal(local[sel], rlocal) and np.array_equal(dist_tab[sel], rdist))
            # every row is in the collection: it must find itself first, at distance 0
            ok = ok and bool(np.array_equal(img[sel, 0], sel // LC_ROWS) and np.array_equal(local[sel, 0], sel % LC_ROWS)
                             and not dist_tab[sel, 0].any())
        else:
            ridx, rdist = oracle.bf_knn_c(query[sel], train, 2, threads=os.cpu_count() or 1)
            ok = bool(np.array_equal(idx[sel], ridx) and np.array_equal(dist_tab[sel], rdist))

    out = None
    if rank == 0:
        out = bench_line(world=world, steps=args.steps, warmup=args.warmup, loop_closure=loop_closure, n_query=n_query, n_train=n_train,
                         n_local=sm.n_local, wall_ms=wall_ms, dev_ms=dev_ms, rank_kernel_ms=rank_kernel_ms, launches=launches,
                         collective=collective, fallback_reason=fallback_reason,
                         rccl_version=None if rccl_version is None else rccl_version.value,
                         plan=launch_plan(ctx, max(sm.n_local, 1), n_train), ok=ok, train_replication=sm.train_replication)
        if args.full and world > 1:
            out["cpu_baseline"] = None
            out["cpu_baseline_note"] = "the CPU leg is timed at N=1 only (same arrays; see the N=1 line)"
        elif args.full and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(query, train)
    sm.free(barrier)                   # unmap peers -> barrier -> free the exported buffers (HIP IPC teardown order)
    full_n1 = rank == 0 and world == 1 and args.full and not loop_closure
    if full_n1 and args.pipelined:
        out["pipelined"] = pipelined_leg(query, train, max(args.steps, 20))
    if full_n1 and not args.no_reproj:
        out["reproj"] = reproj_bench(ctx, max(3, min(args.steps, 20)), args.warmup, cpu=not args.no_cpu_baseline)
    if full_n1 and not args.no_next_rows:
        try:
            out["next_rows"] = next_rows_leg(ctx, cpu=not args.no_cpu_baseline)
        except Exception as exc:   # noqa: BLE001 - an extra leg must never cost the line
            out["next_rows"] = {"error": f"{type(exc).__name__}: {exc}"}
    check_rc = 0
    if world > 1:
        check_rc = ctx.lib.slam_comm_destroy(ctx.handle) if collective == "rccl" else 0
        rz.barrier()
    rz.close()
    ctx.close()
    if check_rc:
        raise SystemExit("slam_comm_destroy failed")
    if rank == 0:
        print(json.dumps(out), flush=True)
    rc = 0 if ok is not False or rank != 0 else 1
    if abandoned:
        # a helper thread is still inside a native call that never returned: a normal interpreter exit would wait for
        # the runtime's teardown behind it
        sys.stderr.flush()
        os._exit(rc)
    return rc


if __name__ == "__main__":
    sys.exit(main())
