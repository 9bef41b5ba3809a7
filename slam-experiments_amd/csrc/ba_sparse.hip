// ba_sparse.hip — sparse bundle adjustment on gfx950: the points are eliminated into a block-sparse reduced camera system over
// the covisibility graph, in the layout the pose-graph solver takes (slam_pg_pcg_f64 / slam_pg_hmul_f64, graph_lm.h).
//
// ba_schur.hip forms the reduced system densely ([K,K,36] blocks behind a [K,L] lookup table) and the host factors it; that
// holds a keyframe window, not the map behind a closed loop.  Here the system exists only where two free poses see a common
// point: diagonal blocks d_Hdiag [K,36], one block d_W [E,36] per covisibility edge (k1 < k2, row block k1, column block k2),
// the gradient d_b [K,6] - and (S + lambda I) dp = -b is exactly what slam_pg_pcg_f64 solves.  With J = [Jp | Jq] per
// observation and w its Huber weight (the arithmetic of reproj.hip / ba_schur.hip: ba_linearise of ba_common.h):
//   Hpp_k = sum w Jp^T Jp, bp_k = sum w Jp^T e (per pose)      Hll_l = sum w Jq^T Jq, bl_l = sum w Jq^T e (per point)
//   Hpl_o = w Jp^T Jq (6x3, per observation)                   E_l = (Hll_l + lambda I)^-1 (0 for a point nobody observes)
//   W_e     = - sum_{pairs (a, b) of e} Hpl_a E_l Hpl_b^T
//   Hdiag_k = Hpp_k - sum_{o of k} Hpl_o E_l Hpl_o^T           (no lambda: the solver adds lambda I)
//   b_k     = bp_k - sum_{o of k} Hpl_o E_l bl_l
//   dl_l    = - E_l (bl_l + sum_{o of l} Hpl_o^T dp_pose(o))
//
// Kernels (f64, no contraction, no floating-point atomics; every sum in an order that depends on the index tables only);
// the four that read a measurement (obs, point, pose, cost) are the templates of ba_sparse_phases.h over bas_mono_edge below,
// the one copy that ba_stereo.hip instantiates over its stereo / weighted edges.
//   bas_obs_kernel      a thread per observation   Hpl_o; the two indices are checked here and counted (slam_index_errors)
//   bas_point_kernel    a thread per point         Hll (6), bl (3) over its list pt_obs, in list order
//   bas_pose_kernel     a workgroup per pose       Hpp (21), bp (6), cost: thread t takes entries t, t + 256, .. of ps_obs,
//                                                  then ba_block_sum (xor tree inside a wave, the four waves in order); a
//                                                  ps_ptr slice outside the table is counted here, once per slice
//   bas_inverse_kernel  a thread per point         E_l, E_l bl_l
//   bas_edge_kernel     a WAVE per edge            lane i takes pairs i, i + 64, .. of the edge's pair list, the 64 lane sums
//                                                  meet in the xor tree: the order is a function of the pair count alone, an
//                                                  edge of one pair and one of thousands take the same path
//   bas_diag_kernel     a workgroup per pose       Hdiag, b over ps_obs as bas_pose_kernel
//   bas_backsub_kernel  a thread per point         dl
//   bas_candidate_kernel a thread per pose / point T' = exp(dp) T (fixed poses copied), X' = X + dl, the gain-ratio
//                                                  denominator as one partial sum per workgroup
//   bas_cost_kernel     a workgroup per pose       robust cost at a state, summed as bas_pose_kernel sums it
//   bas_finish_kernel   one workgroup              partial sums -> one scalar (thread t takes t, t + 256, ..; ba_block_sum)
// Hpl is kept (18 doubles per observation) because three phases of every trial read it while the state stands still;
// the per-pose and per-point sums are consumed once, so their terms are linearised again instead of stored.
//
// No entry point here takes the context's call lock or its workspace: every buffer is the caller's (slam_bas_workspace says
// how large), the launches are asynchronous on the context's stream, and slam_pg_pcg_f64 - which does take the lock - is
// called by the driver between them.
//
// The linearisation of one observation, the block sum, the damped 3x3 inverse and the pose update are ba_schur.hip's, from
// ba_common.h; it and ba_sparse_phases.h are included BEHIND the pragma below, so here they are compiled without contraction
// like everything else.
#include "internal.h"
#include <math.h>

#pragma clang fp contract(off)
#include "ba_common.h"

#include "ba_sparse_common.h"

#define BAS_MAX_PART 1024          // partial sums of the candidate kernel (its grid)

struct bas_obs_tab {
    const int* obs_pose; const int* obs_point; const double2* meas;
    int K, L, O;
};

// the edge model of this file under the phases of ba_sparse_phases.h: ba_linearise of ba_common.h - two rows, weight w, every
// edge live, the Jacobians made with the residual
struct bas_mono_edge {
    static constexpr int ROWS = 2;
    typedef bas_obs_tab tab;
    typedef ba_cam cam;
    typedef double robust;
    ba_lin q;
    double r[2];
    __device__ __forceinline__ void residual(const tab& t, int o, const double* T, const double* X, int k, int l, const cam& c, double delta) {
        ba_linearise(T + (size_t)k * 12, X + (size_t)l * 3, t.meas[o], c, delta, q);
        r[0] = q.e0; r[1] = q.e1;
    }
    __device__ __forceinline__ static bool info_ok(const tab&, int) { return true; }
    __device__ __forceinline__ bool live() const { return true; }
    __device__ __forceinline__ void jacobians(const double*, const cam&) {}
    __device__ __forceinline__ double weight() const { return q.w; }
    __device__ __forceinline__ double rho() const { return q.rho; }
    __device__ __forceinline__ const double* e() const { return r; }
    __device__ __forceinline__ const double* jp() const { return &q.jp[0][0]; }
    __device__ __forceinline__ const double* jq() const { return &q.jq[0][0]; }
};

#include "ba_sparse_phases.h"   // bas_obs_kernel, bas_point_kernel, bas_pose_kernel, bas_cost_kernel: behind the pragma above

// out[0] = sum of part[0..n) (thread t takes t, t + 256, ..); with diagonals given, out[1] = the largest diagonal entry of the
// Hpp of the free poses and of every Hll (the maximum does not depend on an order)
__global__ __launch_bounds__(BA_THREADS) void bas_finish_kernel(const double* __restrict__ part, int n, double* __restrict__ out,
                                                                 const double* __restrict__ Hpp, const uint8_t* __restrict__ fixed, int K,
                                                                 const double* __restrict__ Hll, int L) {
    __shared__ double sw[BAS_WAVES][1];
    __shared__ double res[1];
    __shared__ double mx[BAS_WAVES];
    double acc[1] = {0.0};
    for (int i = (int)threadIdx.x; i < n; i += BA_THREADS) acc[0] += part[i];
    ba_block_sum<1>(acc, sw, res);
    if (threadIdx.x == 0) out[0] = res[0];
    if (!Hpp) return;
    double m = 0.0;
    for (int k = (int)threadIdx.x; k < K; k += BA_THREADS) {
        if (fixed[k]) continue;
        const double* h = Hpp + (size_t)k * 21;
        m = fmax(m, fmax(fmax(h[0], h[6]), fmax(fmax(h[11], h[15]), fmax(h[18], h[20]))));
    }
    for (int l = (int)threadIdx.x; l < L; l += BA_THREADS) {
        const double* h = Hll + (size_t)l * 6;
        m = fmax(m, fmax(h[0], fmax(h[3], h[5])));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0) mx[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) out[1] = fmax(fmax(mx[0], mx[1]), fmax(mx[2], mx[3]));
}

// E_l = (Hll_l + lambda I)^-1 (ba_damped_inverse), 0 for a point nobody observes; Ebl = E bl
__global__ __launch_bounds__(BA_THREADS) void bas_inverse_kernel(int L, const int* __restrict__ pt_ptr, const double* __restrict__ Hll,
                                                                  const double* __restrict__ bl, double lam, double* __restrict__ E /*[L,9]*/,
                                                                  double* __restrict__ Ebl /*[L,3]*/) {
    const int l = (int)(blockIdx.x * BA_THREADS + threadIdx.x);
    if (l >= L) return;
    double e[9];
    if (pt_ptr[l + 1] > pt_ptr[l]) {
        double h[6];
#pragma unroll
        for (int i = 0; i < 6; i++) h[i] = Hll[(size_t)l * 6 + i];
        ba_damped_inverse(h, lam, true, e);
    } else {
#pragma unroll
        for (int i = 0; i < 9; i++) e[i] = 0.0;
    }
    const double* b = bl + (size_t)l * 3;
#pragma unroll
    for (int i = 0; i < 9; i++) E[(size_t)l * 9 + i] = e[i];
#pragma unroll
    for (int r = 0; r < 3; r++) Ebl[(size_t)l * 3 + r] = e[r * 3] * b[0] + e[r * 3 + 1] * b[1] + e[r * 3 + 2] * b[2];
}

// y = h E (6x3 times symmetric 3x3)
__device__ __forceinline__ void bas_he(const double* __restrict__ h, const double* __restrict__ e, double (&y)[6][3]) {
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int c = 0; c < 3; c++) y[a][c] = h[a * 3] * e[c] + h[a * 3 + 1] * e[3 + c] + h[a * 3 + 2] * e[6 + c];
}

// a wave per edge: W_e = - sum over the edge's pairs of Hpl_a E_l Hpl_b^T
__global__ __launch_bounds__(BA_THREADS) void bas_edge_kernel(int E, int O, int L, int64_t P, const int* __restrict__ pair_ptr,
                                                               const int* __restrict__ pair_a, const int* __restrict__ pair_b,
                                                               const int* __restrict__ obs_point, const double* __restrict__ Hpl,
                                                               const double* __restrict__ Einv, unsigned int* __restrict__ index_errors,
                                                               double* __restrict__ W /*[E,36]*/) {
    const int lane = threadIdx.x & 63;
    const int e = (int)blockIdx.x * BAS_WAVES + (int)(threadIdx.x >> 6);
    if (e >= E) return;                                       // wave-uniform
    double acc[36];
#pragma unroll
    for (int i = 0; i < 36; i++) acc[i] = 0.0;
    int p0 = pair_ptr[e], p1 = pair_ptr[e + 1];
    if (p0 < 0 || p1 < p0 || (int64_t)p1 > P) { if (lane == 0) atomicAdd(index_errors, 1u); p0 = p1 = 0; acc[0] = __builtin_nan(""); }
    for (int p = p0 + lane; p < p1; p += 64) {
        const int oa = pair_a[p], ob = pair_b[p];
        if ((unsigned)oa >= (unsigned)O || (unsigned)ob >= (unsigned)O) { atomicAdd(index_errors, 1u); acc[0] = __builtin_nan(""); continue; }
        const int l = obs_point[oa];
        if ((unsigned)l >= (unsigned)L) { acc[0] = __builtin_nan(""); continue; }   // counted by bas_obs_kernel
        double y[6][3];
        bas_he(Hpl + (size_t)oa * 18, Einv + (size_t)l * 9, y);
        const double* hb = Hpl + (size_t)ob * 18;
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int b = 0; b < 6; b++) acc[a * 6 + b] += y[a][0] * hb[b * 3] + y[a][1] * hb[b * 3 + 1] + y[a][2] * hb[b * 3 + 2];
    }
    double mine = 0.0;
#pragma unroll
    for (int i = 0; i < 36; i++) {
        const double s = ba_wave_sum(acc[i]);
        if (lane == i) mine = s;
    }
    if (lane < 36) W[(size_t)e * 36 + lane] = -mine;
}

// a workgroup per pose: Hdiag_k = Hpp_k - sum Hpl_o E_l Hpl_o^T (full symmetric 6x6), b_k = bp_k - sum Hpl_o (E_l bl_l)
__global__ __launch_bounds__(BA_THREADS) void bas_diag_kernel(int O, int L, const int* __restrict__ ps_ptr, const int* __restrict__ ps_obs,
                                                               const int* __restrict__ obs_point, const double* __restrict__ Hpl,
                                                               const double* __restrict__ Einv, const double* __restrict__ Ebl,
                                                               const double* __restrict__ Hpp, const double* __restrict__ bp,
                                                               double* __restrict__ Hdiag /*[K,36]*/, double* __restrict__ b /*[K,6]*/) {
    __shared__ double sw[BAS_WAVES][27];
    __shared__ double out[27];
    const int k = (int)blockIdx.x;
    double acc[27];
#pragma unroll
    for (int i = 0; i < 27; i++) acc[i] = 0.0;
    int a0, a1;
    bas_pose_range(ps_ptr, k, O, a0, a1);
    for (int i = a0 + (int)threadIdx.x; i < a1; i += BA_THREADS) {
        const int o = ps_obs[i];
        if ((unsigned)o >= (unsigned)O) { acc[0] = __builtin_nan(""); continue; }
        const int l = obs_point[o];
        if ((unsigned)l >= (unsigned)L) { acc[0] = __builtin_nan(""); continue; }
        const double* h = Hpl + (size_t)o * 18;
        const double* eb = Ebl + (size_t)l * 3;
        double y[6][3];
        bas_he(h, Einv + (size_t)l * 9, y);
        int n = 0;
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int c = a; c < 6; c++) acc[n++] += y[a][0] * h[c * 3] + y[a][1] * h[c * 3 + 1] + y[a][2] * h[c * 3 + 2];
#pragma unroll
        for (int a = 0; a < 6; a++) acc[21 + a] += h[a * 3] * eb[0] + h[a * 3 + 1] * eb[1] + h[a * 3 + 2] * eb[2];
    }
    ba_block_sum<27>(acc, sw, out);
    if (threadIdx.x < 36) {
        const int r = threadIdx.x / 6, c = threadIdx.x % 6, a = r < c ? r : c, d = r < c ? c : r;
        const int n = a * 6 - a * (a - 1) / 2 + (d - a);      // packed upper triangle, rows of 6, 5, .. entries
        Hdiag[(size_t)k * 36 + threadIdx.x] = Hpp[(size_t)k * 21 + n] - out[n];
    } else if (threadIdx.x < 42) {
        const int a = threadIdx.x - 36;
        b[(size_t)k * 6 + a] = bp[(size_t)k * 6 + a] - out[21 + a];
    }
}

// a thread per point: dl_l = - E_l (bl_l + sum_{o of l} Hpl_o^T dp_pose(o)), in list order
__global__ __launch_bounds__(BA_THREADS) void bas_backsub_kernel(int K, int L, int O, const int* __restrict__ pt_ptr, const int* __restrict__ pt_obs,
                                                                  const int* __restrict__ obs_pose, const double* __restrict__ Hpl,
                                                                  const double* __restrict__ Einv, const double* __restrict__ bl,
                                                                  const double* __restrict__ dp /*[K,6]*/, double* __restrict__ dl /*[L,3]*/) {
    const int l = (int)(blockIdx.x * BA_THREADS + threadIdx.x);
    if (l >= L) return;
    double t[3] = {bl[(size_t)l * 3], bl[(size_t)l * 3 + 1], bl[(size_t)l * 3 + 2]};
    int a0 = pt_ptr[l], a1 = pt_ptr[l + 1];
    if (a0 < 0 || a1 < a0 || a1 > O) a0 = a1 = 0;
    for (int i = a0; i < a1; i++) {
        const int o = pt_obs[i];
        if ((unsigned)o >= (unsigned)O) { t[0] = __builtin_nan(""); continue; }
        const int k = obs_pose[o];
        if ((unsigned)k >= (unsigned)K) { t[0] = __builtin_nan(""); continue; }
        const double* h = Hpl + (size_t)o * 18;
        const double* d = dp + (size_t)k * 6;
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int a = 0; a < 6; a++) t[c] += h[a * 3 + c] * d[a];
    }
    const double* e = Einv + (size_t)l * 9;
#pragma unroll
    for (int c = 0; c < 3; c++) dl[(size_t)l * 3 + c] = a1 > a0 ? -(e[c * 3] * t[0] + e[c * 3 + 1] * t[1] + e[c * 3 + 2] * t[2]) : 0.0;
}

// items 0..K-1 are the poses, K..K+L-1 the points; thread t of workgroup g takes items g * 256 + t + j * (grid * 256), its
// terms of the gain-ratio denominator dp.(lambda dp - bp) / dl.(lambda dl - bl) summed in that order, then ba_block_sum
__global__ __launch_bounds__(BA_THREADS) void bas_candidate_kernel(int K, int L, const uint8_t* __restrict__ fixed, const double* __restrict__ T,
                                                                    const double* __restrict__ X, const double* __restrict__ dp,
                                                                    const double* __restrict__ dl, const double* __restrict__ bp,
                                                                    const double* __restrict__ bl, double lam, double* __restrict__ Tn,
                                                                    double* __restrict__ Xn, double* __restrict__ part) {
    __shared__ double sw[BAS_WAVES][1];
    __shared__ double out[1];
    double acc[1] = {0.0};
    const int64_t n = (int64_t)K + L, step = (int64_t)gridDim.x * BA_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * BA_THREADS + threadIdx.x; i < n; i += step) {
        if (i < K) {
            const size_t k = (size_t)i;
            if (fixed[k]) {
#pragma unroll
                for (int j = 0; j < 12; j++) Tn[k * 12 + j] = T[k * 12 + j];
            } else {
                double d[6];
#pragma unroll
                for (int j = 0; j < 6; j++) d[j] = dp[k * 6 + j];
                ba_apply_update(d, T + k * 12, Tn + k * 12);
                double s = 0.0;
#pragma unroll
                for (int j = 0; j < 6; j++) s += d[j] * (lam * d[j] - bp[k * 6 + j]);
                acc[0] += s;
            }
        } else {
            const size_t l = (size_t)(i - K);
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const double d = dl[l * 3 + j];
                Xn[l * 3 + j] = X[l * 3 + j] + d;
                s += d * (lam * d - bl[l * 3 + j]);
            }
            acc[0] += s;
        }
    }
    ba_block_sum<1>(acc, sw, out);
    if (threadIdx.x == 0) part[blockIdx.x] = out[0];
}

// ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
static inline int bas_cand_blocks(int64_t K, int64_t L) {
    const int64_t n = (K + L + BA_THREADS - 1) / BA_THREADS;
    return (int)(n < 1 ? 1 : n > BAS_MAX_PART ? BAS_MAX_PART : n);
}
int bas_sizes(const char* who, int64_t K, int64_t L, int64_t O, int64_t E, int64_t P) {
    SLAM_REQUIRE(K >= 1 && K <= SLAM_PG_MAX_VERTICES && L >= 1 && L <= SLAM_BAS_MAX_POINTS && O >= 0 && O <= SLAM_BAS_MAX_OBS && E >= 0 &&
                     E <= SLAM_PG_MAX_EDGES && P >= E && P <= SLAM_BAS_MAX_PAIRS,
                 "%s: bad sizes (K=%lld, L=%lld, O=%lld, E=%lld, P=%lld)", who, (long long)K, (long long)L, (long long)O, (long long)E,
                 (long long)P);
    return SLAM_OK;
}

extern "C" int slam_bas_workspace(int64_t K, int64_t L, int64_t O, int64_t E, int64_t P, uint64_t* bytes) {
    SLAM_REQUIRE(bytes, "slam_bas_workspace: null bytes");
    if (int rc = bas_sizes("slam_bas_workspace", K, L, O, E, P)) return rc;
    const uint64_t k = (uint64_t)K, l = (uint64_t)L, o = (uint64_t)(O > 0 ? O : 1), e = (uint64_t)(E > 0 ? E : 1), p = (uint64_t)(P > 0 ? P : 1);
    uint64_t n = 0;
    auto take = [&](uint64_t b) { n += slam_align_up(b); };
    take(o * 4); take(o * 4); take(o * 16); take((l + 1) * 4); take(o * 4); take((k + 1) * 4); take(o * 4);      // observations, the two groupings
    take(e * 8); take((e + 1) * 4); take(p * 4); take(p * 4); take((k + 1) * 4); take(2 * e * 4); take(k);         // edges, pairs, vertex lists, mask
    take(2 * k * 96); take(2 * l * 24);                                                                          // state and candidate
    take(o * 144); take(l * 48); take(l * 24); take(l * 72); take(l * 24);                                       // Hpl, Hll, bl, E, E bl
    take(k * 168); take(k * 48); take(k * 8); take(k * 8);                                                       // Hpp, bp, cost, candidate cost
    take(k * 288); take(e * 288); take(k * 48); take(k * 48); take(l * 24);                                      // Hdiag, W, b, dp, dl
    take(BAS_MAX_PART * 8); take(64);                                                                            // partial sums, scalars
    *bytes = n;
    return SLAM_OK;
}

extern "C" int slam_bas_plan(int64_t K, int64_t L, int64_t O, int64_t E, int64_t P, int32_t* plan) {
    SLAM_REQUIRE(plan, "slam_bas_plan: null plan");
    if (int rc = bas_sizes("slam_bas_plan", K, L, O, E, P)) return rc;
    plan[0] = bas_blocks(O);                              // observation kernel
    plan[1] = bas_blocks(L);                              // point kernels (sums, inverse, back-substitution)
    plan[2] = (int)K;                                     // pose kernels: a workgroup per pose
    plan[3] = (int)((E + BAS_WAVES - 1) / BAS_WAVES);     // edge kernel: a wave per edge, four to a workgroup
    plan[4] = bas_cand_blocks(K, L);                      // candidate kernel = partial sums of the gain-ratio denominator
    plan[5] = BA_THREADS;
    plan[6] = 64;                                         // lanes that share an edge's pairs
    plan[7] = 0;
    return SLAM_OK;
}

// partial sums -> one scalar behind a phase of ba_stereo.hip, on the stream of that phase (bas_finish_kernel as the phases here launch it)
void bas_finish_launch(hipStream_t st, const double* part, int n, double* out, const double* Hpp, const uint8_t* fixed, int K, const double* Hll,
                       int L) {
    bas_finish_kernel<<<1, BA_THREADS, 0, st>>>(part, n, out, Hpp, fixed, K, Hll, L);
}

extern "C" int slam_bas_linearize_f64(slam_ctx* ctx, int64_t K, int64_t L, int64_t O, const double* d_poses, const double* d_points,
                                      const int32_t* d_obs_pose, const int32_t* d_obs_point, const double* d_meas, const int32_t* d_pt_ptr,
                                      const int32_t* d_pt_obs, const int32_t* d_ps_ptr, const int32_t* d_ps_obs, const uint8_t* d_fixed,
                                      double fx, double fy, double cx, double cy, double huber_delta, double* d_Hpl, double* d_Hll,
                                      double* d_bl, double* d_Hpp, double* d_bp, double* d_cost, double* d_scal) {
    SLAM_REQUIRE(ctx, "slam_bas_linearize_f64: null ctx");
    if (int rc = bas_sizes("slam_bas_linearize_f64", K, L, O, 0, 0)) return rc;
    SLAM_REQUIRE(d_poses && d_points && d_obs_pose && d_obs_point && d_meas && d_pt_ptr && d_pt_obs && d_ps_ptr && d_ps_obs && d_fixed &&
                     d_Hpl && d_Hll && d_bl && d_Hpp && d_bp && d_cost && d_scal, "slam_bas_linearize_f64: null device pointer");
    SLAM_REQUIRE(BAS_ALIGNED16(d_meas), "slam_bas_linearize_f64: d_meas must be 16-byte aligned");
    SLAM_REQUIRE(huber_delta >= 0.0, "slam_bas_linearize_f64: huber_delta must not be negative");
    SLAM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const ba_cam cam = {fx, fy, cx, cy};
    const bas_obs_tab t = {d_obs_pose, d_obs_point, (const double2*)d_meas, (int)K, (int)L, (int)O};
    unsigned int* ie = slam_index_error_counter(ctx);
    if (O) bas_obs_kernel<bas_mono_edge><<<bas_blocks(O), BA_THREADS, 0, st>>>(t, d_poses, d_points, cam, huber_delta, ie, d_Hpl);
    bas_point_kernel<bas_mono_edge><<<bas_blocks(L), BA_THREADS, 0, st>>>(t, d_poses, d_points, d_pt_ptr, d_pt_obs, cam, huber_delta, ie, d_Hll, d_bl);
    bas_pose_kernel<bas_mono_edge><<<(unsigned)K, BA_THREADS, 0, st>>>(t, d_poses, d_points, d_ps_ptr, d_ps_obs, cam, huber_delta, ie, d_Hpp, d_bp, d_cost);
    bas_finish_kernel<<<1, BA_THREADS, 0, st>>>(d_cost, (int)K, d_scal, d_Hpp, d_fixed, (int)K, d_Hll, (int)L);
    return slam_launch_check("slam_bas_linearize_f64");
}

extern "C" int slam_bas_cost_f64(slam_ctx* ctx, int64_t K, int64_t L, int64_t O, const double* d_poses, const double* d_points,
                                 const int32_t* d_obs_pose, const int32_t* d_obs_point, const double* d_meas, const int32_t* d_ps_ptr,
                                 const int32_t* d_ps_obs, double fx, double fy, double cx, double cy, double huber_delta, double* d_cost,
                                 double* d_total) {
    SLAM_REQUIRE(ctx, "slam_bas_cost_f64: null ctx");
    if (int rc = bas_sizes("slam_bas_cost_f64", K, L, O, 0, 0)) return rc;
    SLAM_REQUIRE(d_poses && d_points && d_obs_pose && d_obs_point && d_meas && d_ps_ptr && d_ps_obs && d_cost && d_total,
                 "slam_bas_cost_f64: null device pointer");
    SLAM_REQUIRE(BAS_ALIGNED16(d_meas), "slam_bas_cost_f64: d_meas must be 16-byte aligned");
    SLAM_HIP(hipSetDevice(ctx->device));
    const ba_cam cam = {fx, fy, cx, cy};
    const bas_obs_tab t = {d_obs_pose, d_obs_point, (const double2*)d_meas, (int)K, (int)L, (int)O};
    bas_cost_kernel<bas_mono_edge><<<(unsigned)K, BA_THREADS, 0, ctx->stream>>>(t, d_poses, d_points, d_ps_ptr, d_ps_obs, cam, huber_delta, d_cost);
    bas_finish_kernel<<<1, BA_THREADS, 0, ctx->stream>>>(d_cost, (int)K, d_total, nullptr, nullptr, 0, nullptr, 0);
    return slam_launch_check("slam_bas_cost_f64");
}

extern "C" int slam_bas_reduce_f64(slam_ctx* ctx, int64_t K, int64_t L, int64_t O, int64_t E, int64_t P, const int32_t* d_obs_point,
                                   const int32_t* d_pt_ptr, const int32_t* d_ps_ptr, const int32_t* d_ps_obs, const int32_t* d_pair_ptr,
                                   const int32_t* d_pair_a, const int32_t* d_pair_b, const double* d_Hpl, const double* d_Hll,
                                   const double* d_bl, const double* d_Hpp, const double* d_bp, double lambda, double* d_E, double* d_Ebl,
                                   double* d_Hdiag, double* d_W, double* d_b) {
    SLAM_REQUIRE(ctx, "slam_bas_reduce_f64: null ctx");
    if (int rc = bas_sizes("slam_bas_reduce_f64", K, L, O, E, P)) return rc;
    SLAM_REQUIRE(d_obs_point && d_pt_ptr && d_ps_ptr && d_ps_obs && d_Hpl && d_Hll && d_bl && d_Hpp && d_bp && d_E && d_Ebl && d_Hdiag && d_b &&
                     (E == 0 || (d_pair_ptr && d_pair_a && d_pair_b && d_W)), "slam_bas_reduce_f64: null device pointer");
    SLAM_REQUIRE(lambda >= 0.0, "slam_bas_reduce_f64: lambda must not be negative");
    SLAM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    bas_inverse_kernel<<<bas_blocks(L), BA_THREADS, 0, st>>>((int)L, d_pt_ptr, d_Hll, d_bl, lambda, d_E, d_Ebl);
    if (E)
        bas_edge_kernel<<<(unsigned)((E + BAS_WAVES - 1) / BAS_WAVES), BA_THREADS, 0, st>>>((int)E, (int)O, (int)L, P, d_pair_ptr, d_pair_a, d_pair_b,
                                                                                         d_obs_point, d_Hpl, d_E, slam_index_error_counter(ctx), d_W);
    bas_diag_kernel<<<(unsigned)K, BA_THREADS, 0, st>>>((int)O, (int)L, d_ps_ptr, d_ps_obs, d_obs_point, d_Hpl, d_E, d_Ebl, d_Hpp, d_bp, d_Hdiag, d_b);
    return slam_launch_check("slam_bas_reduce_f64");
}

extern "C" int slam_bas_backsub_f64(slam_ctx* ctx, int64_t K, int64_t L, int64_t O, const int32_t* d_pt_ptr, const int32_t* d_pt_obs,
                                    const int32_t* d_obs_pose, const double* d_Hpl, const double* d_E, const double* d_bl, const double* d_dp,
                                    double* d_dl) {
    SLAM_REQUIRE(ctx, "slam_bas_backsub_f64: null ctx");
    if (int rc = bas_sizes("slam_bas_backsub_f64", K, L, O, 0, 0)) return rc;
    SLAM_REQUIRE(d_pt_ptr && d_pt_obs && d_obs_pose && d_Hpl && d_E && d_bl && d_dp && d_dl, "slam_bas_backsub_f64: null device pointer");
    SLAM_HIP(hipSetDevice(ctx->device));
    bas_backsub_kernel<<<bas_blocks(L), BA_THREADS, 0, ctx->stream>>>((int)K, (int)L, (int)O, d_pt_ptr, d_pt_obs, d_obs_pose, d_Hpl, d_E, d_bl, d_dp,
                                                                      d_dl);
    return slam_launch_check("slam_bas_backsub_f64");
}

extern "C" int slam_bas_candidate_f64(slam_ctx* ctx, int64_t K, int64_t L, const uint8_t* d_fixed, const double* d_poses, const double* d_points,
                                      const double* d_dp, const double* d_dl, const double* d_bp, const double* d_bl, double lambda,
                                      double* d_poses_out, double* d_points_out, double* d_part, double* d_denominator) {
    SLAM_REQUIRE(ctx, "slam_bas_candidate_f64: null ctx");
    if (int rc = bas_sizes("slam_bas_candidate_f64", K, L, 0, 0, 0)) return rc;
    SLAM_REQUIRE(d_fixed && d_poses && d_points && d_dp && d_dl && d_bp && d_bl && d_poses_out && d_points_out && d_part && d_denominator,
                 "slam_bas_candidate_f64: null device pointer");
    SLAM_REQUIRE(d_poses != d_poses_out && d_points != d_points_out, "slam_bas_candidate_f64: the candidate must not alias the state");
    SLAM_HIP(hipSetDevice(ctx->device));
    const int nb = bas_cand_blocks(K, L);
    bas_candidate_kernel<<<nb, BA_THREADS, 0, ctx->stream>>>((int)K, (int)L, d_fixed, d_poses, d_points, d_dp, d_dl, d_bp, d_bl, lambda, d_poses_out,
                                                             d_points_out, d_part);
    bas_finish_kernel<<<1, BA_THREADS, 0, ctx->stream>>>(d_part, nb, d_denominator, nullptr, nullptr, 0, nullptr, 0);
    return slam_launch_check("slam_bas_candidate_f64");
}
