// pose_stereo.hip — ORB-SLAM's Optimizer::PoseOptimization for B frames in ONE launch on gfx950: monocular
// (EdgeSE3ProjectXYZOnlyPose) and stereo (EdgeStereoSE3ProjectXYZOnlyPose) edges mixed, every edge weighted by its
// information (1 / scale[level]^2), the chi2 gate and the Huber width chosen by the kind of the edge.
//
// One workgroup of 256 threads per frame, the frame's edges staged in LDS up to SLAM_POSE_STEREO_STAGE, 28 sums per evaluation
// through po_block_sums (a third residual row adds terms to the sums, not sums).  The Levenberg-Marquardt round - lanes 0..9 of
// wave 0 proposing the ten trials of an iteration together, trial 0 evaluated in full, trials 1..9 by one cost-only pass - is
// pose_lm_round.inc, the one copy that pose_opt.hip includes too; pose_lm_run.h holds its shared-memory block and the offsets
// clamp, pose_lm.h the update, the solve and the block sums.  What is this file's own:
//   - the edge model (stereo_edge.h), and the whole file compiled without contraction (stereo_edge.h asks for it; the round is
//     included behind the pragma), so the evaluation and the cost-only pass round alike because they call the same text, not
//     because every fma is written out;
//   - a round ends with a classification pass of its own over ALL edges (weighted chi2 without the kernel, information,
//     Z > 0: se_inlier), which recomputes the active set - an edge may come back - and leaves chi2 per edge; one chi2 buffer,
//     so nothing happens when an evaluation becomes the current one;
//   - an edge with information 0 is never active; a frame whose edges are all switched off returns pose_in.
// Deviations from ORB-SLAM: the Z > 0 test is part of the classification here too (ORB-SLAM applies it in the bundle
// adjustment only), there is no early exit below ten edges, and the order of the edges is the caller's.
//
// Every buffer is the caller's; the call takes neither the context's call lock nor its workspace.
#include "internal.h"
#include <math.h>
#include "pose_lm.h"

#pragma clang fp contract(off)
#include "stereo_edge.h"

#include "pose_lm_run.h"

#define PS_STAGE SLAM_POSE_STEREO_STAGE   // edges kept in LDS: 3 + 3 + 1 + 1 doubles and a flag each (32.5 KiB at 512)

struct ps_params {
    int rounds, iterations;
    se_gate gate;
    se_huber hub;
};

// the edges of one frame: LDS copies when the frame is staged, else the global arrays
struct ps_edges {
    const double* points; const double* meas3; const double* info;
    uint8_t* active; double* chi2;
    int O;
};

// One block-wide evaluation at pose T over the active edges: out[0..20] = upper H, [21..26] = b, [27] = robust cost.
__device__ __forceinline__ void ps_evaluate(const double* T, const ps_edges& g, const se_cam& cam, const se_huber& hub, double* red,
                                            double* part, double* out) {
    double acc[PO_TERMS];
#pragma unroll
    for (int i = 0; i < PO_TERMS; i++) acc[i] = 0.0;
    for (int o = threadIdx.x; o < g.O; o += PO_THREADS) {
        if (!g.active[o]) continue;
        se_res r;
        se_residual(T, g.points + 3 * o, g.meas3[3 * o], g.meas3[3 * o + 1], g.meas3[3 * o + 2], g.info[o], cam, hub, r);
        se_jac j;
        se_jacobians(T, r, cam, j);
        const double ws = r.w * r.s;
        int t = 0;
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int b = a; b < 6; b++) acc[t++] += ws * ((j.jp[0][a] * j.jp[0][b] + j.jp[1][a] * j.jp[1][b]) + j.jp[2][a] * j.jp[2][b]);
#pragma unroll
        for (int a = 0; a < 6; a++) acc[21 + a] += ws * ((j.jp[0][a] * r.e[0] + j.jp[1][a] * r.e[1]) + j.jp[2][a] * r.e[2]);
        acc[27] += r.rho;
    }
    po_block_sums<PO_TERMS>(acc, red, part, out);
}

// The robust cost of the active edges at up to PO_SPEC candidate poses in one pass: costs[j] for every j with solved[j].
__device__ __forceinline__ void ps_costs(const double* Tk /*[PO_SPEC][12]*/, const int* solved, const ps_edges& g, const se_cam& cam,
                                         const se_huber& hub, double* red, double* part, double* costs) {
    double acc[PO_SPEC];
#pragma unroll
    for (int j = 0; j < PO_SPEC; j++) acc[j] = 0.0;
    for (int o = threadIdx.x; o < g.O; o += PO_THREADS) {
        if (!g.active[o]) continue;
        const double p[3] = {g.points[3 * o], g.points[3 * o + 1], g.points[3 * o + 2]};
        const double mu = g.meas3[3 * o], mv = g.meas3[3 * o + 1], mr = g.meas3[3 * o + 2], s = g.info[o];
#pragma unroll
        for (int j = 0; j < PO_SPEC; j++) {
            if (!solved[j]) continue;                                   // block-uniform
            se_res r;
            se_residual(Tk + 12 * j, p, mu, mv, mr, s, cam, hub, r);
            acc[j] += r.rho;
        }
    }
    po_block_sums<PO_SPEC>(acc, red, part, costs);
}

struct ps_shared {
    po_lm_shared lm;
    int count[3];                                   // inliers, stereo inliers (a classification), edges with s > 0 (once)
};

// chi2 and the active flag of EVERY edge at pose T (no kernel), the two counts into sh.count[0..1]; all threads return
// behind a barrier with the counts readable
__device__ __forceinline__ void ps_classify(ps_shared& sh, const double* T, const ps_edges& g, const se_cam& cam, const se_gate& gate) {
    if (threadIdx.x == 0) sh.count[0] = sh.count[1] = 0;
    __syncthreads();
    const se_huber none = {0.0, 0.0};
    int in = 0, st = 0;
    for (int o = threadIdx.x; o < g.O; o += PO_THREADS) {
        se_res r;
        se_residual(T, g.points + 3 * o, g.meas3[3 * o], g.meas3[3 * o + 1], g.meas3[3 * o + 2], g.info[o], cam, none, r);
        const int ok = se_inlier(r, gate) ? 1 : 0;
        g.chi2[o] = r.chi2;
        g.active[o] = (uint8_t)ok;
        in += ok;
        st += ok & r.stereo;
    }
    if (in) atomicAdd(&sh.count[0], in);             // integers: the order does not matter
    if (st) atomicAdd(&sh.count[1], st);
    __syncthreads();
}

// The rounds of one refinement on the edges above; the LM round proper is pose_lm_round.inc.  Force-inlined into both call sites so that the staged instance
// addresses the edges as LDS and the large-frame instance as global memory.  The Levenberg-Marquardt state lives in registers
// of every thread: all threads read the same sums behind the same barrier and take the same decision.
__device__ __forceinline__ const double* ps_run(ps_shared& sh, const ps_edges& g, const se_cam& cam, const ps_params& prm,
                                                unsigned int* index_errors, int* accepted_out) {
    const int tid = threadIdx.x;
    po_lm_shared& lm = sh.lm;
    double* red = lm.red; double* part = lm.part;
    double* cur = lm.sums[0]; double* cand = lm.sums[1];
    const double* T = lm.Tcur;
    int p = 0, accepted = 0;
    {   // every edge with an information starts active; an information that is none is counted and taken as 0
        int mine = 0, bad = 0;
        for (int o = tid; o < g.O; o += PO_THREADS) {
            const double s = g.info[o];
            const int on = se_info(s) > 0.0 ? 1 : 0;
            bad += se_info_ok(s) ? 0 : 1;
            g.active[o] = (uint8_t)on;
            mine += on;
        }
        if (mine) atomicAdd(&sh.count[2], mine);
        if (bad) atomicAdd(index_errors, (unsigned)bad);
    }
    __syncthreads();
    int nactive = sh.count[2];
    se_huber hub = prm.hub;
    for (int round = 0; round < prm.rounds; round++) {
        if (tid < 12) lm.Tcur[tid] = lm.T0[tid];        // every round restarts from the frame's pose
        T = lm.Tcur;
        __syncthreads();
        ps_evaluate(T, g, cam, hub, red, part, cur);
        {   // lambda0 and the iterations: the one copy that pose_opt.hip includes too, here behind contract(off)
#define PO_LM_EVALUATE(T_, out_) ps_evaluate(T_, g, cam, hub, red, part, out_)
#define PO_LM_COSTS(Tk_, solved_, out_) ps_costs(Tk_, solved_, g, cam, hub, red, part, out_)
#define PO_LM_CURRENT() ((void)0)
#include "pose_lm_round.inc"
#undef PO_LM_EVALUATE
#undef PO_LM_COSTS
#undef PO_LM_CURRENT
        }
        ps_classify(sh, T, g, cam, prm.gate);           // the active set of the next round, from ALL edges
        nactive = sh.count[0];
        if (round == 2) hub.delta_mono = hub.delta_stereo = 0.0;
    }
    if (prm.rounds == 0) ps_classify(sh, T, g, cam, prm.gate);
    *accepted_out = accepted;
    return T;
}

// One workgroup per frame: frame b = blockIdx.x owns the edges [offsets[b], offsets[b+1]) of the concatenated arrays.
__global__ __launch_bounds__(PO_THREADS) void pose_stereo_kernel(const double* __restrict__ pose_in, const double* __restrict__ g_points,
                                                                 const double* __restrict__ g_meas3, const double* __restrict__ g_info,
                                                                 int total, const int* __restrict__ offsets, se_cam cam, ps_params prm,
                                                                 double* __restrict__ pose_out, uint8_t* __restrict__ g_active,
                                                                 double* __restrict__ g_chi2, int* __restrict__ stats,
                                                                 unsigned int* __restrict__ index_errors) {
    const int b = blockIdx.x;
    const po_range r = po_frame_range(offsets, b, total, index_errors);
    const int first = r.first, O = r.count;
    pose_in += 12 * (size_t)b; pose_out += 12 * (size_t)b; stats += 4 * (size_t)b;
    g_points += 3 * (size_t)first; g_meas3 += 3 * (size_t)first; g_info += first; g_active += first; g_chi2 += first;
    __shared__ double s_points[PS_STAGE * 3];
    __shared__ double s_meas3[PS_STAGE * 3];
    __shared__ double s_info[PS_STAGE];
    __shared__ double s_chi2[PS_STAGE];
    __shared__ uint8_t s_active[PS_STAGE];
    __shared__ ps_shared sh;
    const int tid = threadIdx.x;
    if (tid < 12) sh.lm.T0[tid] = sh.lm.Tcur[tid] = pose_in[tid];
    if (tid < 3) sh.count[tid] = 0;
    int accepted = 0;
    const double* pose;
    if (O <= PS_STAGE) {
        for (int i = tid; i < O * 3; i += PO_THREADS) { s_points[i] = g_points[i]; s_meas3[i] = g_meas3[i]; }
        for (int o = tid; o < O; o += PO_THREADS) s_info[o] = g_info[o];
        __syncthreads();
        const ps_edges g = {s_points, s_meas3, s_info, s_active, s_chi2, O};
        pose = ps_run(sh, g, cam, prm, index_errors, &accepted);
        for (int o = tid; o < O; o += PO_THREADS) { g_active[o] = s_active[o]; g_chi2[o] = s_chi2[o]; }
    } else {
        __syncthreads();
        const ps_edges g = {g_points, g_meas3, g_info, g_active, g_chi2, O};
        pose = ps_run(sh, g, cam, prm, index_errors, &accepted);
    }
    if (tid < 12) pose_out[tid] = pose[tid];
    if (tid == 0) {
        stats[0] = sh.count[0];                     // inliers at the returned pose
        stats[1] = accepted;                        // accepted LM steps over all rounds
        stats[2] = sh.count[1];                     // stereo inliers
        stats[3] = sh.count[2];                     // edges with an information > 0
    }
}

extern "C" int slam_pose_optimize_stereo_batch_f64(slam_ctx* ctx, int64_t B, const double* d_pose_in, const double* d_points,
                                                   const double* d_meas3, const double* d_info, const int32_t* d_offsets, int64_t O_total,
                                                   double fx, double fy, double cx, double cy, double bf, int rounds, int iterations,
                                                   double chi2_mono, double chi2_stereo, double delta_mono, double delta_stereo,
                                                   double* d_pose_out, uint8_t* d_inlier, double* d_chi2, int32_t* d_stats) {
    SLAM_REQUIRE(ctx, "slam_pose_optimize_stereo_batch_f64: null ctx");
    SLAM_REQUIRE(B >= 0 && B <= (1 << 20) && O_total >= 0 && O_total <= (1 << 28), "slam_pose_optimize_stereo_batch_f64: bad sizes (B=%lld, O=%lld)",
                 (long long)B, (long long)O_total);
    SLAM_REQUIRE(rounds >= 0 && iterations >= 0 && rounds <= 64 && iterations <= 1000, "slam_pose_optimize_stereo_batch_f64: bad rounds / iterations");
    SLAM_REQUIRE(isfinite(fx) && isfinite(fy) && fx != 0.0 && fy != 0.0, "slam_pose_optimize_stereo_batch_f64: fx and fy must be finite and not 0");
    SLAM_REQUIRE(bf > 0.0 && isfinite(bf), "slam_pose_optimize_stereo_batch_f64: bf must be positive and finite");
    SLAM_REQUIRE(chi2_mono >= 0.0 && chi2_stereo >= 0.0, "slam_pose_optimize_stereo_batch_f64: the gates must not be negative");
    SLAM_REQUIRE(delta_mono >= 0.0 && delta_stereo >= 0.0, "slam_pose_optimize_stereo_batch_f64: the Huber widths must not be negative");
    if (B == 0) return SLAM_OK;
    SLAM_REQUIRE(d_pose_in && d_pose_out && d_stats && d_offsets && (O_total == 0 || (d_points && d_meas3 && d_info && d_inlier && d_chi2)),
                 "slam_pose_optimize_stereo_batch_f64: null device pointer");
    SLAM_HIP(hipSetDevice(ctx->device));
    const se_cam cam = {fx, fy, cx, cy, bf};
    const ps_params prm = {rounds, iterations, {chi2_mono, chi2_stereo}, {delta_mono, delta_stereo}};
    pose_stereo_kernel<<<(unsigned)B, PO_THREADS, 0, ctx->stream>>>(d_pose_in, d_points, d_meas3, d_info, (int)O_total, d_offsets, cam, prm,
                                                                    d_pose_out, d_inlier, d_chi2, d_stats, slam_index_error_counter(ctx));
    return slam_launch_check("slam_pose_optimize_stereo_batch_f64");
}
