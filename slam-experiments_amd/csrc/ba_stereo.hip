// ba_stereo.hip — the stereo / level-weighted forms of the phases of the sparse bundle adjustment that read a measurement
// (DESIGN.md 4v): the linearisation, the cost and the classification of ORB-SLAM's LocalBundleAdjustment with
// EdgeSE3ProjectXYZ and EdgeStereoSE3ProjectXYZ mixed, and the per-edge linearisation on its own (slam_reproj_rj_stereo_f64).
//
// An observation carries d_meas3 [O,3] = (mu, mv, mr), mr NaN for a monocular edge, and an information d_info [O] (inverse
// variance, ORB-SLAM's 1 / scale[level]^2; 0 switches the edge off).  The edge model is stereo_edge.h.  Everything downstream
// of the blocks - slam_bas_reduce_f64, _backsub_f64, _candidate_f64, slam_pg_pcg_f64 - works on Hpl / Hll / bl / Hpp / bp and
// is called as it is.
//
// Kernels: those of ba_sparse.hip's linearisation and cost, one for one, with the same lists, the same thread mapping and the
// same ba_block_sum, so every sum has the order it has there.
//   bast_obs_kernel      a thread per observation   Hpl_o = (w s) Jp^T Jq over two or three rows; indices and informations are
//                                                    checked here and counted (slam_index_errors)
//   bast_point_kernel    a thread per point         Hll (6), bl (3) over pt_obs, in list order
//   bast_pose_kernel     a workgroup per pose       Hpp (21), bp (6), cost; a bad ps_ptr slice is counted here
//   bast_cost_kernel     a workgroup per pose       robust cost at a state
//   bast_classify_kernel a thread per observation   weighted chi2 and the inlier flag (se_inlier) at a state
//   stereo_rj_kernel     a thread per observation   e, Jpose, Jpoint, chi2, w of every edge
// Parent rule: with every mr NaN, every s = 1 and delta_mono = huber_delta the blocks, the per-pose cost and d_scal equal those
// of slam_bas_linearize_f64 / slam_bas_cost_f64 in value: rows 0 and 1 are ba_linearise's text, (w s) is formed first (w * 1 = w)
// and the third row of a monocular edge adds an exact 0 to each term.
//
// No entry point here takes the context's call lock or its workspace: every buffer is the caller's.
#include "internal.h"
#include <math.h>

#pragma clang fp contract(off)
#include "ba_common.h"
#include "ba_sparse_common.h"
#include "stereo_edge.h"

struct bast_tab {
    const int* obs_pose; const int* obs_point; const double* meas3; const double* info;
    int K, L, O;
};

// observation o of an index table at (T, X): residuals, chi2, weight; false (nothing dereferenced) when o or one of its
// indices is outside.  k and l come back for the Jacobians.
__device__ __forceinline__ bool bast_at(const bast_tab& t, const double* __restrict__ T, const double* __restrict__ X, const int o,
                                        const se_cam& cam, const se_huber& hub, se_res& r, int& k, int& l) {
    if ((unsigned)o >= (unsigned)t.O) return false;
    k = t.obs_pose[o]; l = t.obs_point[o];
    if ((unsigned)k >= (unsigned)t.K || (unsigned)l >= (unsigned)t.L) return false;
    const double* m = t.meas3 + (size_t)o * 3;
    se_residual(T + (size_t)k * 12, X + (size_t)l * 3, m[0], m[1], m[2], t.info[o], cam, hub, r);
    return true;
}

__global__ __launch_bounds__(BA_THREADS) void bast_obs_kernel(const bast_tab t, const double* __restrict__ T, const double* __restrict__ X,
                                                               se_cam cam, se_huber hub, unsigned int* __restrict__ index_errors,
                                                               double* __restrict__ Hpl /*[O,18]*/) {
    const int o = (int)(blockIdx.x * BA_THREADS + threadIdx.x);
    if (o >= t.O) return;
    se_res r;
    int k, l;
    double* h = Hpl + (size_t)o * 18;
    if (!bast_at(t, T, X, o, cam, hub, r, k, l)) {           // reported, never dereferenced; its block poisons what reads it
        atomicAdd(index_errors, 1u);
#pragma unroll
        for (int i = 0; i < 18; i++) h[i] = __builtin_nan("");
        return;
    }
    if (!se_info_ok(t.info[o])) atomicAdd(index_errors, 1u);  // an information that is none: counted, taken as 0
    if (!(r.s > 0.0)) {                                       // switched off: adds nothing anywhere
#pragma unroll
        for (int i = 0; i < 18; i++) h[i] = 0.0;
        return;
    }
    se_jac j;
    se_jacobians(T + (size_t)k * 12, r, cam, j);
    const double ws = r.w * r.s;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int c = 0; c < 3; c++) h[a * 3 + c] = ws * ((j.jp[0][a] * j.jq[0][c] + j.jp[1][a] * j.jq[1][c]) + j.jp[2][a] * j.jq[2][c]);
}

__global__ __launch_bounds__(BA_THREADS) void bast_point_kernel(const bast_tab t, const double* __restrict__ T, const double* __restrict__ X,
                                                                 const int* __restrict__ pt_ptr, const int* __restrict__ pt_obs, se_cam cam,
                                                                 se_huber hub, unsigned int* __restrict__ index_errors,
                                                                 double* __restrict__ Hll /*[L,6]*/, double* __restrict__ bl /*[L,3]*/) {
    const int l = (int)(blockIdx.x * BA_THREADS + threadIdx.x);
    if (l >= t.L) return;
    double h[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};
    int a0 = pt_ptr[l], a1 = pt_ptr[l + 1];
    if (a0 < 0 || a1 < a0 || a1 > t.O) { atomicAdd(index_errors, 1u); a1 = a0 = 0; }
    for (int i = a0; i < a1; i++) {
        se_res r;
        int k, l2;
        if (!bast_at(t, T, X, pt_obs[i], cam, hub, r, k, l2)) { h[0] = __builtin_nan(""); continue; }
        if (!(r.s > 0.0)) continue;
        se_jac j;
        se_jacobians(T + (size_t)k * 12, r, cam, j);
        const double ws = r.w * r.s;
        int n = 0;
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int c = a; c < 3; c++) h[n++] += ws * ((j.jq[0][a] * j.jq[0][c] + j.jq[1][a] * j.jq[1][c]) + j.jq[2][a] * j.jq[2][c]);
#pragma unroll
        for (int a = 0; a < 3; a++) b[a] += ws * ((j.jq[0][a] * r.e[0] + j.jq[1][a] * r.e[1]) + j.jq[2][a] * r.e[2]);
    }
#pragma unroll
    for (int i = 0; i < 6; i++) Hll[(size_t)l * 6 + i] = h[i];
#pragma unroll
    for (int i = 0; i < 3; i++) bl[(size_t)l * 3 + i] = b[i];
}

__global__ __launch_bounds__(BA_THREADS) void bast_pose_kernel(const bast_tab t, const double* __restrict__ T, const double* __restrict__ X,
                                                                const int* __restrict__ ps_ptr, const int* __restrict__ ps_obs, se_cam cam,
                                                                se_huber hub, unsigned int* __restrict__ index_errors,
                                                                double* __restrict__ Hpp /*[K,21]*/, double* __restrict__ bp /*[K,6]*/,
                                                                double* __restrict__ cost /*[K]*/) {
    __shared__ double sw[BAS_WAVES][28];
    __shared__ double out[28];
    const int k = (int)blockIdx.x;
    double acc[28];
#pragma unroll
    for (int i = 0; i < 28; i++) acc[i] = 0.0;
    int a0, a1;
    if (!bas_pose_range(ps_ptr, k, t.O, a0, a1) && threadIdx.x == 0) atomicAdd(index_errors, 1u);
    for (int i = a0 + (int)threadIdx.x; i < a1; i += BA_THREADS) {
        se_res r;
        int k2, l;
        if (!bast_at(t, T, X, ps_obs[i], cam, hub, r, k2, l)) { acc[27] = __builtin_nan(""); continue; }
        if (!(r.s > 0.0)) continue;
        se_jac j;
        se_jacobians(T + (size_t)k2 * 12, r, cam, j);
        const double ws = r.w * r.s;
        int n = 0;
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int c = a; c < 6; c++) acc[n++] += ws * ((j.jp[0][a] * j.jp[0][c] + j.jp[1][a] * j.jp[1][c]) + j.jp[2][a] * j.jp[2][c]);
#pragma unroll
        for (int a = 0; a < 6; a++) acc[21 + a] += ws * ((j.jp[0][a] * r.e[0] + j.jp[1][a] * r.e[1]) + j.jp[2][a] * r.e[2]);
        acc[27] += r.rho;
    }
    ba_block_sum<28>(acc, sw, out);
    if (threadIdx.x < 21) Hpp[(size_t)k * 21 + threadIdx.x] = out[threadIdx.x];
    else if (threadIdx.x < 27) bp[(size_t)k * 6 + threadIdx.x - 21] = out[threadIdx.x];
    else if (threadIdx.x == 27) cost[k] = out[27];
}

__global__ __launch_bounds__(BA_THREADS) void bast_cost_kernel(const bast_tab t, const double* __restrict__ T, const double* __restrict__ X,
                                                                const int* __restrict__ ps_ptr, const int* __restrict__ ps_obs, se_cam cam,
                                                                se_huber hub, double* __restrict__ cost /*[K]*/) {
    __shared__ double sw[BAS_WAVES][1];
    __shared__ double out[1];
    const int k = (int)blockIdx.x;
    double acc[1] = {0.0};
    int a0, a1;
    bas_pose_range(ps_ptr, k, t.O, a0, a1);
    for (int i = a0 + (int)threadIdx.x; i < a1; i += BA_THREADS) {
        se_res r;
        int k2, l;
        if (!bast_at(t, T, X, ps_obs[i], cam, hub, r, k2, l)) { acc[0] = __builtin_nan(""); continue; }
        if (!(r.s > 0.0)) continue;
        acc[0] += r.rho;
    }
    ba_block_sum<1>(acc, sw, out);
    if (threadIdx.x == 0) cost[k] = out[0];
}

// chi2 and the inlier flag of every observation at a state (no kernel: the gate is on the plain weighted chi2); an observation
// with an index outside its range has chi2 NaN and is no inlier, and is not counted here (the linearisation counts it)
__global__ __launch_bounds__(BA_THREADS) void bast_classify_kernel(const bast_tab t, const double* __restrict__ T, const double* __restrict__ X,
                                                                    se_cam cam, se_gate gate, double* __restrict__ chi2 /*[O]*/,
                                                                    uint8_t* __restrict__ inlier /*[O]*/) {
    const int o = (int)(blockIdx.x * BA_THREADS + threadIdx.x);
    if (o >= t.O) return;
    se_res r;
    int k, l;
    const se_huber none = {0.0, 0.0};
    if (!bast_at(t, T, X, o, cam, none, r, k, l)) { chi2[o] = __builtin_nan(""); inlier[o] = 0; return; }
    chi2[o] = r.chi2;
    inlier[o] = se_inlier(r, gate) ? 1 : 0;
}

// slam_reproj_rj_stereo_f64: a thread per observation, 35 doubles out.  Plain stores: not transposed through LDS as reproj.hip's
// two-row kernel is (unmeasured here; the adjustments above never materialise these arrays).
__global__ __launch_bounds__(BA_THREADS) void stereo_rj_kernel(const bast_tab t, const double* __restrict__ T, const double* __restrict__ X,
                                                                se_cam cam, se_huber hub, unsigned int* __restrict__ index_errors,
                                                                double* __restrict__ e /*[O,3]*/, double* __restrict__ Jpose /*[O,18]*/,
                                                                double* __restrict__ Jpoint /*[O,9]*/, double* __restrict__ chi2 /*[O]*/,
                                                                double* __restrict__ w /*[O]*/) {
    const int o = (int)(blockIdx.x * BA_THREADS + threadIdx.x);
    if (o >= t.O) return;
    se_res r;
    int k, l;
    double* eo = e + (size_t)o * 3; double* jp = Jpose + (size_t)o * 18; double* jq = Jpoint + (size_t)o * 9;
    if (!bast_at(t, T, X, o, cam, hub, r, k, l)) {
        atomicAdd(index_errors, 1u);
        const double nan = __builtin_nan("");
#pragma unroll
        for (int i = 0; i < 3; i++) eo[i] = nan;
#pragma unroll
        for (int i = 0; i < 18; i++) jp[i] = nan;
#pragma unroll
        for (int i = 0; i < 9; i++) jq[i] = nan;
        chi2[o] = nan; w[o] = nan;
        return;
    }
    if (!se_info_ok(t.info[o])) atomicAdd(index_errors, 1u);
    se_jac j;
    se_jacobians(T + (size_t)k * 12, r, cam, j);
#pragma unroll
    for (int i = 0; i < 3; i++) eo[i] = r.e[i];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int a = 0; a < 6; a++) jp[i * 6 + a] = j.jp[i][a];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int c = 0; c < 3; c++) jq[i * 3 + c] = j.jq[i][c];
    chi2[o] = r.chi2; w[o] = r.w;
}

// ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
static int bast_model(const char* who, double fx, double fy, double bf, double delta_mono, double delta_stereo) {
    SLAM_REQUIRE(isfinite(fx) && isfinite(fy) && fx != 0.0 && fy != 0.0, "%s: fx and fy must be finite and not 0", who);
    SLAM_REQUIRE(bf > 0.0 && isfinite(bf), "%s: bf must be positive and finite", who);
    SLAM_REQUIRE(delta_mono >= 0.0 && delta_stereo >= 0.0, "%s: the Huber widths must not be negative", who);
    return SLAM_OK;
}

extern "C" int slam_reproj_rj_stereo_f64(slam_ctx* ctx, const double* d_poses, int64_t K, const double* d_points, int64_t L,
                                       const int32_t* d_obs_pose, const int32_t* d_obs_point, const double* d_meas3, const double* d_info,
                                       int64_t O, double fx, double fy, double cx, double cy, double bf, double delta_mono,
                                       double delta_stereo, double* d_e, double* d_Jpose, double* d_Jpoint, double* d_chi2, double* d_w) {
    SLAM_REQUIRE(ctx, "slam_reproj_rj_stereo_f64: null ctx");
    SLAM_REQUIRE(O >= 0 && O <= SLAM_BAS_MAX_OBS && K >= 0 && L >= 0 && K <= 0x7FFFFFFF && L <= 0x7FFFFFFF,
                 "slam_reproj_rj_stereo_f64: bad sizes (K=%lld, L=%lld, O=%lld)", (long long)K, (long long)L, (long long)O);
    if (int rc = bast_model("slam_reproj_rj_stereo_f64", fx, fy, bf, delta_mono, delta_stereo)) return rc;
    if (O == 0) return SLAM_OK;
    SLAM_REQUIRE(K > 0 && L > 0, "slam_reproj_rj_stereo_f64: observations given but no poses / points");
    SLAM_REQUIRE(d_poses && d_points && d_obs_pose && d_obs_point && d_meas3 && d_info && d_e && d_Jpose && d_Jpoint && d_chi2 && d_w,
                 "slam_reproj_rj_stereo_f64: null device pointer");
    SLAM_HIP(hipSetDevice(ctx->device));
    const se_cam cam = {fx, fy, cx, cy, bf};
    const se_huber hub = {delta_mono, delta_stereo};
    const bast_tab t = {d_obs_pose, d_obs_point, d_meas3, d_info, (int)K, (int)L, (int)O};
    stereo_rj_kernel<<<bas_blocks(O), BA_THREADS, 0, ctx->stream>>>(t, d_poses, d_points, cam, hub, slam_index_error_counter(ctx), d_e, d_Jpose,
                                                                    d_Jpoint, d_chi2, d_w);
    return slam_launch_check("slam_reproj_rj_stereo_f64");
}

extern "C" int slam_bas_linearize_stereo_f64(slam_ctx* ctx, int64_t K, int64_t L, int64_t O, const double* d_poses, const double* d_points,
                                             const int32_t* d_obs_pose, const int32_t* d_obs_point, const double* d_meas3,
                                             const double* d_info, const int32_t* d_pt_ptr, const int32_t* d_pt_obs, const int32_t* d_ps_ptr,
                                             const int32_t* d_ps_obs, const uint8_t* d_fixed, double fx, double fy, double cx, double cy,
                                             double bf, double delta_mono, double delta_stereo, double* d_Hpl, double* d_Hll, double* d_bl,
                                             double* d_Hpp, double* d_bp, double* d_cost, double* d_scal) {
    SLAM_REQUIRE(ctx, "slam_bas_linearize_stereo_f64: null ctx");
    if (int rc = bas_sizes("slam_bas_linearize_stereo_f64", K, L, O, 0, 0)) return rc;
    if (int rc = bast_model("slam_bas_linearize_stereo_f64", fx, fy, bf, delta_mono, delta_stereo)) return rc;
    SLAM_REQUIRE(d_poses && d_points && d_obs_pose && d_obs_point && d_meas3 && d_info && d_pt_ptr && d_pt_obs && d_ps_ptr && d_ps_obs &&
                     d_fixed && d_Hpl && d_Hll && d_bl && d_Hpp && d_bp && d_cost && d_scal, "slam_bas_linearize_stereo_f64: null device pointer");
    SLAM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const se_cam cam = {fx, fy, cx, cy, bf};
    const se_huber hub = {delta_mono, delta_stereo};
    const bast_tab t = {d_obs_pose, d_obs_point, d_meas3, d_info, (int)K, (int)L, (int)O};
    unsigned int* ie = slam_index_error_counter(ctx);
    if (O) bast_obs_kernel<<<bas_blocks(O), BA_THREADS, 0, st>>>(t, d_poses, d_points, cam, hub, ie, d_Hpl);
    bast_point_kernel<<<bas_blocks(L), BA_THREADS, 0, st>>>(t, d_poses, d_points, d_pt_ptr, d_pt_obs, cam, hub, ie, d_Hll, d_bl);
    bast_pose_kernel<<<(unsigned)K, BA_THREADS, 0, st>>>(t, d_poses, d_points, d_ps_ptr, d_ps_obs, cam, hub, ie, d_Hpp, d_bp, d_cost);
    bas_finish_launch(st, d_cost, (int)K, d_scal, d_Hpp, d_fixed, (int)K, d_Hll, (int)L);
    return slam_launch_check("slam_bas_linearize_stereo_f64");
}

extern "C" int slam_bas_cost_stereo_f64(slam_ctx* ctx, int64_t K, int64_t L, int64_t O, const double* d_poses, const double* d_points,
                                        const int32_t* d_obs_pose, const int32_t* d_obs_point, const double* d_meas3, const double* d_info,
                                        const int32_t* d_ps_ptr, const int32_t* d_ps_obs, double fx, double fy, double cx, double cy, double bf,
                                        double delta_mono, double delta_stereo, double* d_cost, double* d_total) {
    SLAM_REQUIRE(ctx, "slam_bas_cost_stereo_f64: null ctx");
    if (int rc = bas_sizes("slam_bas_cost_stereo_f64", K, L, O, 0, 0)) return rc;
    if (int rc = bast_model("slam_bas_cost_stereo_f64", fx, fy, bf, delta_mono, delta_stereo)) return rc;
    SLAM_REQUIRE(d_poses && d_points && d_obs_pose && d_obs_point && d_meas3 && d_info && d_ps_ptr && d_ps_obs && d_cost && d_total,
                 "slam_bas_cost_stereo_f64: null device pointer");
    SLAM_HIP(hipSetDevice(ctx->device));
    const se_cam cam = {fx, fy, cx, cy, bf};
    const se_huber hub = {delta_mono, delta_stereo};
    const bast_tab t = {d_obs_pose, d_obs_point, d_meas3, d_info, (int)K, (int)L, (int)O};
    bast_cost_kernel<<<(unsigned)K, BA_THREADS, 0, ctx->stream>>>(t, d_poses, d_points, d_ps_ptr, d_ps_obs, cam, hub, d_cost);
    bas_finish_launch(ctx->stream, d_cost, (int)K, d_total, nullptr, nullptr, 0, nullptr, 0);
    return slam_launch_check("slam_bas_cost_stereo_f64");
}

extern "C" int slam_bas_classify_stereo_f64(slam_ctx* ctx, int64_t K, int64_t L, int64_t O, const double* d_poses, const double* d_points,
                                            const int32_t* d_obs_pose, const int32_t* d_obs_point, const double* d_meas3,
                                            const double* d_info, double fx, double fy, double cx, double cy, double bf, double chi2_mono,
                                            double chi2_stereo, double* d_chi2, uint8_t* d_inlier) {
    SLAM_REQUIRE(ctx, "slam_bas_classify_stereo_f64: null ctx");
    if (int rc = bas_sizes("slam_bas_classify_stereo_f64", K, L, O, 0, 0)) return rc;
    if (int rc = bast_model("slam_bas_classify_stereo_f64", fx, fy, bf, 0.0, 0.0)) return rc;
    SLAM_REQUIRE(chi2_mono >= 0.0 && chi2_stereo >= 0.0, "slam_bas_classify_stereo_f64: the gates must not be negative");
    if (O == 0) return SLAM_OK;
    SLAM_REQUIRE(d_poses && d_points && d_obs_pose && d_obs_point && d_meas3 && d_info && d_chi2 && d_inlier,
                 "slam_bas_classify_stereo_f64: null device pointer");
    SLAM_HIP(hipSetDevice(ctx->device));
    const se_cam cam = {fx, fy, cx, cy, bf};
    const se_gate gate = {chi2_mono, chi2_stereo};
    const bast_tab t = {d_obs_pose, d_obs_point, d_meas3, d_info, (int)K, (int)L, (int)O};
    bast_classify_kernel<<<bas_blocks(O), BA_THREADS, 0, ctx->stream>>>(t, d_poses, d_points, cam, gate, d_chi2, d_inlier);
    return slam_launch_check("slam_bas_classify_stereo_f64");
}
