// ba_stereo.hip — the stereo / level-weighted forms of the phases of the sparse bundle adjustment that read a measurement
// (DESIGN.md 4v): the linearisation, the cost and the classification of ORB-SLAM's LocalBundleAdjustment with
// EdgeSE3ProjectXYZ and EdgeStereoSE3ProjectXYZ mixed, and the per-edge linearisation on its own (slam_reproj_rj_stereo_f64).
//
// An observation carries d_meas3 [O,3] = (mu, mv, mr), mr NaN for a monocular edge, and an information d_info [O] (inverse
// variance, ORB-SLAM's 1 / scale[level]^2; 0 switches the edge off).  The edge model is stereo_edge.h.  Everything downstream
// of the blocks - slam_bas_reduce_f64, _backsub_f64, _candidate_f64, slam_pg_pcg_f64 - works on Hpl / Hll / bl / Hpp / bp and
// is called as it is.
//
// Kernels: the linearisation and the cost are the four phase templates of ba_sparse_phases.h - the one copy that ba_sparse.hip
// instantiates too: same lists, same thread mapping, same NaN poisoning, same ba_block_sum - over bast_edge below:
//   bas_obs_kernel<bast_edge>    a thread per observation   Hpl_o = (w s) Jp^T Jq over three rows (the third 0 for a monocular
//                                                            edge); indices and informations are checked here and counted
//   bas_point_kernel<bast_edge>  a thread per point         Hll (6), bl (3) over pt_obs, in list order
//   bas_pose_kernel<bast_edge>   a workgroup per pose       Hpp (21), bp (6), cost; a bad ps_ptr slice is counted here
//   bas_cost_kernel<bast_edge>   a workgroup per pose       robust cost at a state
// and two of this file's own:
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

// the edge model of this file under the phases of ba_sparse_phases.h: stereo_edge.h - three rows (the third 0 for a monocular
// edge), weight w s, an edge live iff s > 0, the Jacobians made for live edges only
struct bast_edge {
    static constexpr int ROWS = 3;
    typedef bast_tab tab;
    typedef se_cam cam;
    typedef se_huber robust;
    se_res r;
    se_jac j;
    __device__ __forceinline__ void residual(const tab& t, int o, const double* T, const double* X, int k, int l, const cam& c, const se_huber& hub) {
        const double* m = t.meas3 + (size_t)o * 3;
        se_residual(T + (size_t)k * 12, X + (size_t)l * 3, m[0], m[1], m[2], t.info[o], c, hub, r);
    }
    __device__ __forceinline__ static bool info_ok(const tab& t, int o) { return se_info_ok(t.info[o]); }
    __device__ __forceinline__ bool live() const { return r.s > 0.0; }
    __device__ __forceinline__ void jacobians(const double* P, const cam& c) { se_jacobians(P, r, c, j); }
    __device__ __forceinline__ double weight() const { return r.w * r.s; }
    __device__ __forceinline__ double rho() const { return r.rho; }
    __device__ __forceinline__ const double* e() const { return r.e; }
    __device__ __forceinline__ const double* jp() const { return &j.jp[0][0]; }
    __device__ __forceinline__ const double* jq() const { return &j.jq[0][0]; }
};

#include "ba_sparse_phases.h"   // bas_obs_kernel, bas_point_kernel, bas_pose_kernel, bas_cost_kernel: behind the pragma above

// chi2 and the inlier flag of every observation at a state (no kernel: the gate is on the plain weighted chi2); an observation
// with an index outside its range has chi2 NaN and is no inlier, and is not counted here (the linearisation counts it)
__global__ __launch_bounds__(BA_THREADS) void bast_classify_kernel(const bast_tab t, const double* __restrict__ T, const double* __restrict__ X,
                                                                    se_cam cam, se_gate gate, double* __restrict__ chi2 /*[O]*/,
                                                                    uint8_t* __restrict__ inlier /*[O]*/) {
    const int o = (int)(blockIdx.x * BA_THREADS + threadIdx.x);
    if (o >= t.O) return;
    bast_edge m;
    int k, l;
    const se_huber none = {0.0, 0.0};
    if (!bas_at(t, T, X, o, cam, none, m, k, l)) { chi2[o] = __builtin_nan(""); inlier[o] = 0; return; }
    chi2[o] = m.r.chi2;
    inlier[o] = se_inlier(m.r, gate) ? 1 : 0;
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
    bast_edge m;
    int k, l;
    double* eo = e + (size_t)o * 3; double* jp = Jpose + (size_t)o * 18; double* jq = Jpoint + (size_t)o * 9;
    if (!bas_at(t, T, X, o, cam, hub, m, k, l)) {
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
    m.jacobians(T + (size_t)k * 12, cam);
    const se_res& r = m.r;
    const se_jac& j = m.j;
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
    if (O) bas_obs_kernel<bast_edge><<<bas_blocks(O), BA_THREADS, 0, st>>>(t, d_poses, d_points, cam, hub, ie, d_Hpl);
    bas_point_kernel<bast_edge><<<bas_blocks(L), BA_THREADS, 0, st>>>(t, d_poses, d_points, d_pt_ptr, d_pt_obs, cam, hub, ie, d_Hll, d_bl);
    bas_pose_kernel<bast_edge><<<(unsigned)K, BA_THREADS, 0, st>>>(t, d_poses, d_points, d_ps_ptr, d_ps_obs, cam, hub, ie, d_Hpp, d_bp, d_cost);
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
    bas_cost_kernel<bast_edge><<<(unsigned)K, BA_THREADS, 0, ctx->stream>>>(t, d_poses, d_points, d_ps_ptr, d_ps_obs, cam, hub, d_cost);
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
