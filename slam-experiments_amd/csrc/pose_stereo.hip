// pose_stereo.hip — ORB-SLAM's Optimizer::PoseOptimization for B frames in ONE launch on gfx950: monocular
// (EdgeSE3ProjectXYZOnlyPose) and stereo (EdgeStereoSE3ProjectXYZOnlyPose) edges mixed, every edge weighted by its
// information (1 / scale[level]^2), the chi2 gate and the Huber width chosen by the kind of the edge.
//
// The kernel is pose_opt.hip's with the edge model of stereo_edge.h under it: one workgroup of 256 threads per frame, the
// frame's edges staged in LDS up to SLAM_POSE_STEREO_STAGE, 28 sums per evaluation through po_block_sums (a third residual row
// adds terms to the sums, not sums), lanes 0..9 of wave 0 proposing the ten trials of an iteration together, the same
// Levenberg-Marquardt schedule (pose_lm.h holds what the two files share: update, solve, block sums).  What differs from
// pose_opt.hip besides the model:
//   - the whole file is compiled without contraction (stereo_edge.h asks for it), so the evaluation and the cost-only pass
//     round alike because they call the same text, not because every fma is written out;
//   - a round ends with a classification pass of its own over ALL edges (weighted chi2 without the kernel, information,
//     Z > 0: se_inlier), which recomputes the active set - an edge may come back - and leaves chi2 per edge; one chi2 buffer
//     instead of two, four cheap passes more per call;
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

#define PS_STAGE SLAM_POSE_STEREO_STAGE   // edges kept in LDS: 3 + 3 + 1 + 1 doubles and a flag each (32.5 KiB at 512)
#define PS_SPEC 9                         // trials 1..9 of an iteration, evaluated together after trial 0 was turned down
#define PS_TRIALS (PS_SPEC + 1)           // maxTrialsAfterFailure of g2o's Levenberg-Marquardt

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

// The robust cost of the active edges at up to PS_SPEC candidate poses in one pass: costs[j] for every j with solved[j].
__device__ __forceinline__ void ps_costs(const double* Tk /*[PS_SPEC][12]*/, const int* solved, const ps_edges& g, const se_cam& cam,
                                         const se_huber& hub, double* red, double* part, double* costs) {
    double acc[PS_SPEC];
#pragma unroll
    for (int j = 0; j < PS_SPEC; j++) acc[j] = 0.0;
    for (int o = threadIdx.x; o < g.O; o += PO_THREADS) {
        if (!g.active[o]) continue;
        const double p[3] = {g.points[3 * o], g.points[3 * o + 1], g.points[3 * o + 2]};
        const double mu = g.meas3[3 * o], mv = g.meas3[3 * o + 1], mr = g.meas3[3 * o + 2], s = g.info[o];
#pragma unroll
        for (int j = 0; j < PS_SPEC; j++) {
            if (!solved[j]) continue;                                   // block-uniform
            se_res r;
            se_residual(Tk + 12 * j, p, mu, mv, mr, s, cam, hub, r);
            acc[j] += r.rho;
        }
    }
    po_block_sums<PS_SPEC>(acc, red, part, costs);
}

struct ps_shared {
    double red[PO_TERMS * PO_RED_STRIDE];
    double part[PO_TERMS * 8];
    double sums[2][PO_TERMS];                       // the evaluation at the current pose / at the candidate: swapped, not copied
    double T0[12], Tcur[12];
    double pose[2][PS_TRIALS * 12];                 // the candidates of an iteration; the buffers alternate
    double scale_k[PS_TRIALS], cost_k[PS_SPEC];
    int solved_k[PS_TRIALS];
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

// The LM loop proper, pose_opt.hip's po_run on the edges above.  Force-inlined into both call sites so that the staged instance
// addresses the edges as LDS and the large-frame instance as global memory.  The Levenberg-Marquardt state lives in registers
// of every thread: all threads read the same sums behind the same barrier and take the same decision.
__device__ __forceinline__ const double* ps_run(ps_shared& sh, const ps_edges& g, const se_cam& cam, const ps_params& prm,
                                                unsigned int* index_errors, int* accepted_out) {
    const int tid = threadIdx.x;
    double* red = sh.red; double* part = sh.part;
    double* cur = sh.sums[0]; double* cand = sh.sums[1];
    const double* T = sh.Tcur;
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
        if (tid < 12) sh.Tcur[tid] = sh.T0[tid];        // every round restarts from the frame's pose
        T = sh.Tcur;
        __syncthreads();
        ps_evaluate(T, g, cam, hub, red, part, cur);
        double lambda, ni = 2.0;
        {
            double dmax = 0.0;
            const int diag[6] = {0, 6, 11, 15, 18, 20};
#pragma unroll
            for (int i = 0; i < 6; i++) dmax = fmax(dmax, cur[diag[i]]);
            lambda = 1e-5 * fmax(dmax, 1e-12);          // tau * max diagonal
        }
        for (int it = 0; it < prm.iterations && nactive > 0; it++) {
            // the ten trials of this iteration are proposed together: a trial that is turned down changes nothing but the
            // damping, so lane j of wave 0 solves with the damping trial j would meet (pose_opt.hip)
            double* cands = sh.pose[p];
            if (tid < PS_TRIALS) {
                double lam = lambda, n2 = ni;
                for (int k = 0; k < tid; k++) { lam *= n2; n2 *= 2.0; }
                double dx[6];
                const bool ok_j = po_solve(cur, cur + 21, lam, dx);
                double sc = 1e-3;
                for (int i = 0; i < 6; i++) sc += dx[i] * (lam * dx[i] - cur[21 + i]);
                sh.solved_k[tid] = ok_j ? 1 : 0;
                if (ok_j) { po_apply_update(dx, T, cands + 12 * tid); sh.scale_k[tid] = sc; }
            }
            __syncthreads();
            const int solved = sh.solved_k[0];          // read now: the next iteration's proposals overwrite them
            const double scale = sh.scale_k[0];
            if (solved) ps_evaluate(cands, g, cam, hub, red, part, cand);
            const double rho0 = solved ? (cur[27] - cand[27]) / scale : -1.0;
            if (solved && rho0 > 0.0 && isfinite(cand[27])) {
                { double* t = cur; cur = cand; cand = t; }
                T = cands;
                p ^= 1;
                const double gq = 2.0 * rho0 - 1.0;
                lambda *= fmax(1.0 / 3.0, fmin(1.0 - gq * gq * gq, 2.0 / 3.0));
                ni = 2.0;
                accepted++;
                continue;
            }
            lambda *= ni;
            ni *= 2.0;
            if (solved && !isfinite(lambda)) break;     // (an unsolvable system never ends the iteration by itself)
            // trial 0 was turned down: the costs of trials 1..9 in one pass, walked in order
            ps_costs(cands + 12, sh.solved_k + 1, g, cam, hub, red, part, sh.cost_k);
            int taken = -1;
            for (int j = 0; j < PS_SPEC; j++) {
                if (sh.solved_k[j + 1]) {
                    const double rho = (cur[27] - sh.cost_k[j]) / sh.scale_k[j + 1];
                    if (rho > 0.0 && isfinite(sh.cost_k[j])) {
                        const double gq = 2.0 * rho - 1.0;
                        lambda *= fmax(1.0 / 3.0, fmin(1.0 - gq * gq * gq, 2.0 / 3.0));
                        ni = 2.0;
                        taken = j + 1;
                        break;
                    }
                }
                lambda *= ni;
                ni *= 2.0;
                if (sh.solved_k[j + 1] && !isfinite(lambda)) break;
            }
            if (taken < 0) break;                       // ten trials turned down (or the damping overflowed)
            accepted++;
            T = cands + 12 * taken;
            p ^= 1;
            ps_evaluate(T, g, cam, hub, red, part, cur);   // H, b, cost at the accepted pose
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
    // A table that is not ascending or leaves [0, total] is the caller's bug; it is reported (slam_index_errors) and the frame
    // shrinks to what lies inside, never a wild access.
    const int b = blockIdx.x, lo = offsets[b], hi = offsets[b + 1];
    const int first = min(max(lo, 0), total), last = min(max(hi, first), total);
    if ((first != lo || last != hi) && threadIdx.x == 0) atomicAdd(index_errors, 1u);
    const int O = last - first;
    pose_in += 12 * (size_t)b; pose_out += 12 * (size_t)b; stats += 4 * (size_t)b;
    g_points += 3 * (size_t)first; g_meas3 += 3 * (size_t)first; g_info += first; g_active += first; g_chi2 += first;
    __shared__ double s_points[PS_STAGE * 3];
    __shared__ double s_meas3[PS_STAGE * 3];
    __shared__ double s_info[PS_STAGE];
    __shared__ double s_chi2[PS_STAGE];
    __shared__ uint8_t s_active[PS_STAGE];
    __shared__ ps_shared sh;
    const int tid = threadIdx.x;
    if (tid < 12) sh.T0[tid] = sh.Tcur[tid] = pose_in[tid];
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
