// sim3_opt.hip — batched Sim(3) refinement by reprojection error on gfx950: ORB-SLAM's Optimizer::OptimizeSim3, the step its
// ComputeSim3 runs between the Sim3Solver (sim3.hip) and the fusion, for MANY loop candidates in one call.  A 7-DoF
// Levenberg-Marquardt refinement of the similarity between two keyframes that minimises the reprojection error of the matched
// map points in BOTH images against the MEASURED keypoints under a Huber kernel, drops the correspondences above a chi-square
// gate, refines again without the kernel and reports how many survived.  The reference has no call site (it closes no loops).
//
//   slam_sim3_optimize_f64     one 256-lane workgroup per candidate; the whole schedule in one launch
//
// The specification (residuals, chart, Jacobians, schedule, the order of the sums) is stated in include/slamhip.h; this file
// keeps sim3.hip's rule - f64, contraction OFF, only + - * / sqrt - so that the host build of the routines below
// (SIM3_OPT_HOST_ONLY, the test suite's twin) gives the device's bits.  That is why the retraction is rational (Cayley for the
// rotation, 1 + x + x^2 / 2 for the scale) and not Exp.
//
// How the kernel runs it: the Levenberg-Marquardt state (model, damping, the 36 sums of the current linearisation) lives in
// the registers of EVERY lane - all lanes read the same sums behind the same barrier, solve the same 7x7 system and take the
// same decision, so a verdict needs no lane-0 section.  The trials of an iteration are made one after the other, as the
// header states them: an evaluation is one block-wide pass (36 sums for a linearisation, 1 for a trial's cost).
#ifndef SIM3_OPT_HOST_ONLY           // a host build of the routines alone (the test suite's twin) defines it
#include "internal.h"
#endif
#include <math.h>
#include <stdint.h>
#include "geometry_common.h"         // intrinsics, GEO_HD

#pragma clang fp contract(off)

#define SO_HD __host__ __device__ __forceinline__
#define SO_LANES 256                 // lanes of the stated summation order (the host twin restates it)
#define SO_TERMS 36                  // 28 (upper H, row by row) + 7 (b) + 1 (cost)
#define SO_TRIALS 10                 // g2o's maxTrialsAfterFailure
#define SO_REJECTED 1                // status bits of d_stats[b][3]
#define SO_BAD_MODEL 2
#define SO_STALLED 4
#define SO_DBL_MAX 1.7976931348623157e308

struct so_params {
    double th2;
    int it0, it_bad, it_clean, min_pairs, fix_scale;
};

// ---- one correspondence p [12]: X1 (0..2), X2 (3..5), px1 (6, 7), px2 (8, 9), sigma2 (10, 11) ----------------------------
SO_HD bool so_finite(double x) { return fabs(x) <= SO_DBL_MAX; }     // false for inf and NaN
SO_HD bool so_pair_ok(const double* p) {
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 12; k++) fin = fin && so_finite(p[k]);
    return fin && p[2] > 0.0 && p[5] > 0.0 && p[10] > 0.0 && p[11] > 0.0;
}
SO_HD bool so_model_ok(const double* model) {
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 13; k++) fin = fin && so_finite(model[k]);
    return fin && model[12] > 0.0;
}
SO_HD void so_identity(double* model) {
#pragma unroll
    for (int i = 0; i < 12; i++) model[i] = (i % 5 == 0) ? 1.0 : 0.0;
    model[12] = 1.0;
}
// a model in the form it is evaluated in, m [21]: A = s R (9), t (3), R (9) - the scoring form of sim3.hip
SO_HD void so_form(const double* model, double* m) {
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            m[3 * i + j] = model[12] * model[4 * i + j];
            m[12 + 3 * i + j] = model[4 * i + j];
        }
        m[9 + i] = model[4 * i + 3];
    }
}

// Y = s R X1 + t seen in image 2, W = R^T (X2 - t) seen in image 1, in the operation order of the RANSAC score
struct so_res { double Y[3], W[3], e2[2], e1[2], c2, c1; };
SO_HD void so_residual(const double* m, const double* p, const geo_cam& cam, so_res& r) {
    const double* A = m;
    const double* t = m + 9;
    const double* R = m + 12;
    r.Y[0] = ((A[0] * p[0] + A[1] * p[1]) + A[2] * p[2]) + t[0];
    r.Y[1] = ((A[3] * p[0] + A[4] * p[1]) + A[5] * p[2]) + t[1];
    r.Y[2] = ((A[6] * p[0] + A[7] * p[1]) + A[8] * p[2]) + t[2];
    r.e2[0] = p[8] - (cam.fx * (r.Y[0] / r.Y[2]) + cam.cx);
    r.e2[1] = p[9] - (cam.fy * (r.Y[1] / r.Y[2]) + cam.cy);
    const double y0 = p[3] - t[0], y1 = p[4] - t[1], y2 = p[5] - t[2];
    r.W[0] = (R[0] * y0 + R[3] * y1) + R[6] * y2;
    r.W[1] = (R[1] * y0 + R[4] * y1) + R[7] * y2;
    r.W[2] = (R[2] * y0 + R[5] * y1) + R[8] * y2;
    r.e1[0] = p[6] - (cam.fx * (r.W[0] / r.W[2]) + cam.cx);
    r.e1[1] = p[7] - (cam.fy * (r.W[1] / r.W[2]) + cam.cy);
    r.c2 = (r.e2[0] * r.e2[0] + r.e2[1] * r.e2[1]) / p[11];
    r.c1 = (r.e1[0] * r.e1[0] + r.e1[1] * r.e1[1]) / p[10];
}
SO_HD bool so_front(const so_res& r) { return r.Y[2] > 0.0 && r.W[2] > 0.0; }
SO_HD bool so_keep(const so_res& r, double th2) { return r.c1 <= th2 && r.c2 <= th2 && so_front(r); }
// Huber on sqrt(c) (delta = 0: none): the weight rho' and the robust cost rho
SO_HD void so_huber(double c, double delta, double* w, double* rho) {
    *w = 1.0;
    *rho = c;
    if (delta > 0.0) {
        const double en = sqrt(c);
        if (en > delta) { *w = delta / en; *rho = (2.0 * delta) * en - delta * delta; }
    }
}
// what a pair adds to a trial's cost; *bad is set when one of its depths is not positive
SO_HD double so_cost_pair(const double* m, const double* p, const geo_cam& cam, double delta, bool* bad) {
    so_res r;
    so_residual(m, p, cam, r);
    double w2, w1, rho2, rho1;
    so_huber(r.c2, delta, &w2, &rho2);
    so_huber(r.c1, delta, &w1, &rho1);
    if (!so_front(r)) *bad = true;
    return rho2 + rho1;
}
// J = -Jpi(P) D for a 3x7 D; the scale column is zero with fix_scale
SO_HD void so_project_jac(const double* P, const double (&D)[3][7], const geo_cam& cam, int fix_scale, double (&J)[2][7]) {
    const double zi = 1.0 / P[2];
    const double a0 = cam.fx * zi, a2 = (cam.fx * P[0]) * (zi * zi);
    const double b1 = cam.fy * zi, b2 = (cam.fy * P[1]) * (zi * zi);
#pragma unroll
    for (int c = 0; c < 7; c++) {
        J[0][c] = -(a0 * D[0][c] - a2 * D[2][c]);
        J[1][c] = -(b1 * D[1][c] - b2 * D[2][c]);
    }
    if (fix_scale) { J[0][6] = 0.0; J[1][6] = 0.0; }
}
// the Jacobians of e2 and e1 in the tangent order [omega, upsilon, sigma] at delta = 0
SO_HD void so_jacobians(const double* m, const double* p, const so_res& r, const geo_cam& cam, int fix_scale, double (&J2)[2][7],
                        double (&J1)[2][7]) {
    const double* R = m + 12;
    const double* Y = r.Y;
    const double D2[3][7] = {{0.0, Y[2], -Y[1], 1.0, 0.0, 0.0, Y[0]},          // [-[Y]x, I, Y]
                             {-Y[2], 0.0, Y[0], 0.0, 1.0, 0.0, Y[1]},
                             {Y[1], -Y[0], 0.0, 0.0, 0.0, 1.0, Y[2]}};
    so_project_jac(Y, D2, cam, fix_scale, J2);
    const double x = p[3], y = p[4], z = p[5];
    const double G[3][7] = {{0.0, -z, y, -1.0, 0.0, 0.0, -x},                   // [[X2]x, -I, -X2]
                            {z, 0.0, -x, 0.0, -1.0, 0.0, -y},
                            {-y, x, 0.0, 0.0, 0.0, -1.0, -z}};
    double D1[3][7];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int c = 0; c < 7; c++) D1[i][c] = (R[i] * G[0][c] + R[3 + i] * G[1][c]) + R[6 + i] * G[2][c];      // R^T G
    so_project_jac(r.W, D1, cam, fix_scale, J1);
}
// what a pair adds to a linearisation, acc [36]: edge 2 first, then edge 1, each with the weight rho' / sigma2
SO_HD void so_acc_edge(double* acc, const double (&J)[2][7], const double* e, double w) {
    int t = 0;
#pragma unroll
    for (int a = 0; a < 7; a++)
#pragma unroll
        for (int b = a; b < 7; b++) acc[t++] += w * (J[0][a] * J[0][b] + J[1][a] * J[1][b]);
#pragma unroll
    for (int a = 0; a < 7; a++) acc[28 + a] += w * (J[0][a] * e[0] + J[1][a] * e[1]);
}
SO_HD void so_acc_pair(double* acc, const double* m, const double* p, const geo_cam& cam, double delta, int fix_scale) {
    so_res r;
    so_residual(m, p, cam, r);
    double J2[2][7], J1[2][7], w2, w1, rho2, rho1;
    so_jacobians(m, p, r, cam, fix_scale, J2, J1);
    so_huber(r.c2, delta, &w2, &rho2);
    so_huber(r.c1, delta, &w1, &rho1);
    so_acc_edge(acc, J2, r.e2, w2 / p[11]);
    so_acc_edge(acc, J1, r.e1, w1 / p[10]);
    acc[35] += rho2 + rho1;
}

// ---- one Levenberg-Marquardt step on the combined sums s [36] -----------------------------------------------------------------
SO_HD double so_lambda0(const double* s) {
    const int diag[7] = {0, 7, 13, 18, 22, 25, 27};
    double dmax = 1e-12;
#pragma unroll
    for (int i = 0; i < 7; i++) dmax = s[diag[i]] > dmax ? s[diag[i]] : dmax;
    return 1e-5 * dmax;
}
// (H + lam I) x = -b by LDL^T; false when a pivot is not finite and positive
SO_HD bool so_solve(const double* s, double lam, int fix_scale, double* x) {
    double A[7][7], L[7][7], d[7], dinv[7], y[7];
    int t = 0;
#pragma unroll
    for (int i = 0; i < 7; i++)
#pragma unroll
        for (int j = i; j < 7; j++) { A[i][j] = s[t]; A[j][i] = s[t]; t++; }
#pragma unroll
    for (int i = 0; i < 7; i++) A[i][i] += lam;
    bool spd = true;
#pragma unroll
    for (int j = 0; j < 7; j++) {
        double v = A[j][j];
#pragma unroll
        for (int k = 0; k < j; k++) v -= (L[j][k] * L[j][k]) * d[k];
        spd = spd && v > 0.0 && so_finite(v);
        d[j] = v;
        dinv[j] = 1.0 / v;
#pragma unroll
        for (int i = j + 1; i < 7; i++) {
            double u = A[i][j];
#pragma unroll
            for (int k = 0; k < j; k++) u -= (L[i][k] * L[j][k]) * d[k];
            L[i][j] = u * dinv[j];
        }
    }
    if (!spd) return false;
#pragma unroll
    for (int i = 0; i < 7; i++) {
        double v = -s[28 + i];
#pragma unroll
        for (int k = 0; k < i; k++) v -= L[i][k] * y[k];
        y[i] = v;
    }
#pragma unroll
    for (int i = 6; i >= 0; i--) {
        double v = y[i] * dinv[i];
#pragma unroll
        for (int k = i + 1; k < 7; k++) v -= L[k][i] * x[k];
        x[i] = v;
    }
    if (fix_scale) x[6] = 0.0;
    return true;
}
// the denominator of the gain ratio: x . (lam x - b) + 1e-3
SO_HD double so_gain_scale(const double* s, double lam, const double* x) {
    double sc = 1e-3;
#pragma unroll
    for (int i = 0; i < 7; i++) sc += x[i] * (lam * x[i] - s[28 + i]);
    return sc;
}
SO_HD double so_accept_factor(double rho) {
    const double g = 2.0 * rho - 1.0;
    double f = 1.0 - (g * g) * g;
    f = f < 2.0 / 3.0 ? f : 2.0 / 3.0;
    return f > 1.0 / 3.0 ? f : 1.0 / 3.0;
}
// S <- (s_d s, R_d R, s_d R_d t + upsilon): Cayley rotation of a = omega / 2, s_d = 1 + sigma + sigma^2 / 2
SO_HD void so_retract(const double* model, const double* x, double* out) {
    const double a0 = x[0] / 2.0, a1 = x[1] / 2.0, a2 = x[2] / 2.0;
    const double n = (a0 * a0 + a1 * a1) + a2 * a2;
    const double inv = 1.0 / (1.0 + n), k = 1.0 - n;
    double Q[9];
    Q[0] = (k + 2.0 * (a0 * a0)) * inv;        Q[1] = (2.0 * (a0 * a1) - 2.0 * a2) * inv; Q[2] = (2.0 * (a0 * a2) + 2.0 * a1) * inv;
    Q[3] = (2.0 * (a1 * a0) + 2.0 * a2) * inv; Q[4] = (k + 2.0 * (a1 * a1)) * inv;        Q[5] = (2.0 * (a1 * a2) - 2.0 * a0) * inv;
    Q[6] = (2.0 * (a2 * a0) - 2.0 * a1) * inv; Q[7] = (2.0 * (a2 * a1) + 2.0 * a0) * inv; Q[8] = (k + 2.0 * (a2 * a2)) * inv;
    const double sd = (1.0 + x[6]) + (x[6] * x[6]) / 2.0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) out[4 * i + j] = (Q[3 * i] * model[j] + Q[3 * i + 1] * model[4 + j]) + Q[3 * i + 2] * model[8 + j];
        out[4 * i + 3] = sd * ((Q[3 * i] * model[3] + Q[3 * i + 1] * model[7]) + Q[3 * i + 2] * model[11]) + x[3 + i];
    }
    out[12] = sd * model[12];
}

#ifndef SIM3_OPT_HOST_ONLY
// =============================================================== kernel ======================================================
#define SO_STAGE 512                 // pairs kept in LDS: 12 doubles each by component (48 KiB) and a flag byte
static_assert(SO_STAGE == SLAM_SIM3_OPT_STAGE, "the header states it");

// where a candidate's pairs are read from: the LDS copy (component k of pair i at lds[k * SO_STAGE + i]: consecutive lanes on
// consecutive banks) or the global arrays
template <bool STAGED>
struct so_data {
    const double* lds;
    const double *X1, *X2, *px1, *px2, *sg;
    uint8_t* active;
    __device__ __forceinline__ void load(int i, double* p) const {
        if (STAGED) {
#pragma unroll
            for (int k = 0; k < 12; k++) p[k] = lds[k * SO_STAGE + i];
        } else {
            so_load_global(X1, X2, px1, px2, sg, i, p);
        }
    }
    static __device__ __forceinline__ void so_load_global(const double* X1, const double* X2, const double* px1, const double* px2,
                                                          const double* sg, int i, double* p) {
#pragma unroll
        for (int k = 0; k < 3; k++) { p[k] = X1[3 * (size_t)i + k]; p[3 + k] = X2[3 * (size_t)i + k]; }
        p[6] = px1[2 * (size_t)i]; p[7] = px1[2 * (size_t)i + 1];
        p[8] = px2[2 * (size_t)i]; p[9] = px2[2 * (size_t)i + 1];
        p[10] = sg ? sg[2 * (size_t)i] : 1.0; p[11] = sg ? sg[2 * (size_t)i + 1] : 1.0;
    }
};

struct so_shared {
    double part[4][SO_TERMS];        // the four waves' sums
    int cnt[4][2];
};

// The stated order: every lane arrives with the sum over its own positions; within each wave of 64 consecutive lanes the tree
// "for stride = 32, 16, ..., 1: lane l < stride adds lane l + stride to its own" (a shuffle: what lanes >= stride compute is
// never read by a lane below them), then the four wave sums as (w0 + w1) + (w2 + w3).  Every lane returns with the sums.
template <int NT>
__device__ __forceinline__ void so_block_sums(double (&acc)[NT], so_shared& sh, double* out) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int stride = 32; stride >= 1; stride >>= 1) {
#pragma unroll
        for (int k = 0; k < NT; k++) acc[k] += __shfl_down(acc[k], stride, 64);
    }
    __syncthreads();                                    // the sums of the pass before are read
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < NT; k++) sh.part[tid >> 6][k] = acc[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NT; k++) out[k] = (sh.part[0][k] + sh.part[1][k]) + (sh.part[2][k] + sh.part[3][k]);
}
// integers: any order gives the same counts.  v[0], v[1] summed over the block
__device__ __forceinline__ void so_block_counts(int a, int b, so_shared& sh, int* out) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int stride = 32; stride >= 1; stride >>= 1) { a += __shfl_down(a, stride, 64); b += __shfl_down(b, stride, 64); }
    __syncthreads();
    if ((tid & 63) == 0) { sh.cnt[tid >> 6][0] = a; sh.cnt[tid >> 6][1] = b; }
    __syncthreads();
    out[0] = (sh.cnt[0][0] + sh.cnt[1][0]) + (sh.cnt[2][0] + sh.cnt[3][0]);
    out[1] = (sh.cnt[0][1] + sh.cnt[1][1]) + (sh.cnt[2][1] + sh.cnt[3][1]);
}

template <bool STAGED>
__device__ __forceinline__ void so_linearize(const so_data<STAGED>& D, int n, const double* model, const geo_cam& cam, double delta,
                                             int fix_scale, so_shared& sh, double* sums) {
    double m[21], acc[SO_TERMS];
    so_form(model, m);
#pragma unroll
    for (int k = 0; k < SO_TERMS; k++) acc[k] = 0.0;
    for (int i = threadIdx.x; i < n; i += SO_LANES) {
        if (!D.active[i]) continue;
        double p[12];
        D.load(i, p);
        so_acc_pair(acc, m, p, cam, delta, fix_scale);
    }
    so_block_sums<SO_TERMS>(acc, sh, sums);
}
template <bool STAGED>
__device__ __forceinline__ double so_cost(const so_data<STAGED>& D, int n, const double* model, const geo_cam& cam, double delta,
                                          so_shared& sh, bool* bad_out) {
    double m[21], acc[1] = {0.0}, out[1];
    so_form(model, m);
    bool bad = false;
    for (int i = threadIdx.x; i < n; i += SO_LANES) {
        if (!D.active[i]) continue;
        double p[12];
        D.load(i, p);
        acc[0] += so_cost_pair(m, p, cam, delta, &bad);
    }
    *bad_out = __syncthreads_or(bad ? 1 : 0) != 0;
    so_block_sums<1>(acc, sh, out);
    return out[0];
}
// one stage of the schedule: `iters` iterations from `model` (overwritten); true when it ended on ten refusals
template <bool STAGED>
__device__ __forceinline__ bool so_stage(const so_data<STAGED>& D, int n, double* model, const geo_cam& cam, double delta, int iters,
                                         int fix_scale, so_shared& sh, int* accepted) {
    if (iters <= 0) return false;
    double sums[SO_TERMS], lambda = 0.0, ni = 2.0;
    for (int it = 0; it < iters; it++) {
        so_linearize(D, n, model, cam, delta, fix_scale, sh, sums);
        if (it == 0) lambda = so_lambda0(sums);
        bool took = false;
        for (int trial = 0; trial < SO_TRIALS && !took; trial++) {
            double x[7], cand[13];
            bool ok = so_solve(sums, lambda, fix_scale, x);             // uniform over the block, as everything below
            double rho = -1.0;
            if (ok) {
                so_retract(model, x, cand);
                ok = so_model_ok(cand);
            }
            if (ok) {
                bool bad;
                const double cost = so_cost(D, n, cand, cam, delta, sh, &bad);
                ok = so_finite(cost) && !bad;
                rho = (sums[35] - cost) / so_gain_scale(sums, lambda, x);
            }
            if (ok && rho > 0.0) {
#pragma unroll
                for (int k = 0; k < 13; k++) model[k] = cand[k];
                lambda *= so_accept_factor(rho);
                ni = 2.0;
                (*accepted)++;
                took = true;
            } else {
                lambda *= ni;
                ni *= 2.0;
            }
        }
        if (!took) return true;
    }
    return false;
}
// a pair stays iff both chi2 are within the gate and both depths positive at `model`; returns {staying, leaving}
template <bool STAGED>
__device__ __forceinline__ void so_classify(const so_data<STAGED>& D, int n, const double* model, const geo_cam& cam, double th2,
                                            so_shared& sh, int* counts) {
    double m[21];
    so_form(model, m);
    int stay = 0, leave = 0;
    for (int i = threadIdx.x; i < n; i += SO_LANES) {
        if (!D.active[i]) continue;
        double p[12];
        D.load(i, p);
        so_res r;
        so_residual(m, p, cam, r);
        const bool keep = so_keep(r, th2);
        D.active[i] = keep ? 1 : 0;
        stay += keep ? 1 : 0;
        leave += keep ? 0 : 1;
    }
    so_block_counts(stay, leave, sh, counts);           // (its barriers also order the flags for the next pass: a lane
}                                                       // only ever reads and writes the flags of its own positions)

template <bool STAGED>
__device__ __forceinline__ void so_run(const so_data<STAGED>& D, int n, const double* model_in, const geo_cam& cam, const so_params& prm,
                                       so_shared& sh, double* model_out, uint8_t* inlier, const uint8_t* eligible, double* chi2,
                                       int* stats) {
    const int tid = threadIdx.x;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    double in[13], model[13];
#pragma unroll
    for (int k = 0; k < 13; k++) { in[k] = model_in[k]; model[k] = in[k]; }
    int status = 0, accepted = 0, counts[2] = {0, 0}, nbad = 0;
    if (!so_model_ok(in)) {
        status = SO_REJECTED | SO_BAD_MODEL;
        so_identity(in);
    } else {
        // `eligible` holds what so_pair_ok said (written by the caller); the depths at the input model join it here
        double m[21];
        so_form(in, m);
        for (int i = tid; i < n; i += SO_LANES) {
            uint8_t a = eligible[i];
            if (a) {
                double p[12];
                D.load(i, p);
                so_res r;
                so_residual(m, p, cam, r);
                a = so_front(r) ? 1 : 0;
            }
            D.active[i] = a;
            chi2[2 * (size_t)i] = a ? 0.0 : nan;        // NaN marks "inactive from the start" until the end
        }
        for (int stage = 0; stage < 2; stage++) {
            const double delta = stage == 0 ? sqrt(prm.th2) : 0.0;
            const int iters = stage == 0 ? prm.it0 : (nbad > 0 ? prm.it_bad : prm.it_clean);
            if (so_stage(D, n, model, cam, delta, iters, prm.fix_scale, sh, &accepted)) status |= SO_STALLED;
            so_classify(D, n, model, cam, prm.th2, sh, counts);
            if (stage == 0) {
                nbad = counts[1];
                if (counts[0] < prm.min_pairs) { status |= SO_REJECTED; break; }
            }
        }
    }
    const bool rejected = (status & SO_REJECTED) != 0;
    {
        double m[21];
        so_form(model, m);
        for (int i = tid; i < n; i += SO_LANES) {
            const bool live = !(status & SO_BAD_MODEL) && chi2[2 * (size_t)i] == 0.0;          // active at the start
            double c1 = nan, c2 = nan;
            if (live && !rejected) {
                double p[12];
                D.load(i, p);
                so_res r;
                so_residual(m, p, cam, r);
                c1 = r.c1; c2 = r.c2;
            }
            const uint8_t keep = (!rejected && D.active[i]) ? 1 : 0;
            chi2[2 * (size_t)i] = c1;
            chi2[2 * (size_t)i + 1] = c2;
            inlier[i] = keep;
        }
    }
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 13; k++) model_out[k] = rejected ? in[k] : model[k];
        stats[0] = rejected ? 0 : counts[0];
        stats[1] = accepted;
        stats[2] = nbad;
        stats[3] = status;
    }
}

// grid B, one workgroup per candidate.  d_inlier doubles as the eligibility / activity flags of a candidate too large to
// stage (a lane reads and writes the entries of its own positions only), as pose_opt_kernel uses its d_inlier.
__global__ __launch_bounds__(SO_LANES) void so_optimize_kernel(const int* __restrict__ offsets, int M, const double* __restrict__ X1_all,
                                                               const double* __restrict__ X2_all, const double* __restrict__ px1_all,
                                                               const double* __restrict__ px2_all, const double* __restrict__ sigma2,
                                                               const double* __restrict__ model_in, geo_cam cam, so_params prm,
                                                               double* __restrict__ model_out, uint8_t* __restrict__ inlier,
                                                               double* __restrict__ chi2, int* __restrict__ stats,
                                                               unsigned int* __restrict__ index_errors) {
    __shared__ double s_pair[12 * SO_STAGE];
    __shared__ uint8_t s_active[SO_STAGE], s_eligible[SO_STAGE];
    __shared__ so_shared sh;
    const int b = blockIdx.x, tid = threadIdx.x;
    int first, last; bool bad;
    geo_range(offsets, b, M, &first, &last, &bad);
    if (bad && tid == 0) atomicAdd(index_errors, 1u);
    const int n = last - first;
    const double* X1 = X1_all + 3 * (size_t)first;
    const double* X2 = X2_all + 3 * (size_t)first;
    const double* p1 = px1_all + 2 * (size_t)first;
    const double* p2 = px2_all + 2 * (size_t)first;
    const double* sg = sigma2 ? sigma2 + 2 * (size_t)first : nullptr;
    if (n <= SO_STAGE) {
        for (int i = tid; i < n; i += SO_LANES) {
            double p[12];
            so_data<false>::so_load_global(X1, X2, p1, p2, sg, i, p);
#pragma unroll
            for (int k = 0; k < 12; k++) s_pair[k * SO_STAGE + i] = p[k];
            s_eligible[i] = so_pair_ok(p) ? 1 : 0;
        }
        const so_data<true> D = {s_pair, nullptr, nullptr, nullptr, nullptr, nullptr, s_active};
        so_run<true>(D, n, model_in + 13 * (size_t)b, cam, prm, sh, model_out + 13 * (size_t)b, inlier + first, s_eligible,
                     chi2 + 2 * (size_t)first, stats + 4 * b);
    } else {
        uint8_t* act = inlier + first;
        for (int i = tid; i < n; i += SO_LANES) {
            double p[12];
            so_data<false>::so_load_global(X1, X2, p1, p2, sg, i, p);
            act[i] = so_pair_ok(p) ? 1 : 0;
        }
        const so_data<false> D = {nullptr, X1, X2, p1, p2, sg, act};
        so_run<false>(D, n, model_in + 13 * (size_t)b, cam, prm, sh, model_out + 13 * (size_t)b, act, act, chi2 + 2 * (size_t)first,
                      stats + 4 * b);
    }
}

// =============================================================== entry point =================================================
extern "C" int slam_sim3_optimize_f64(slam_ctx* ctx, int64_t B, const int32_t* d_offsets, const double* d_X1, const double* d_X2,
                                      const double* d_px1, const double* d_px2, int64_t M, const double* d_sigma2, const double* d_model_in,
                                      double fx, double fy, double cx, double cy, double th2, int it0, int it_bad, int it_clean, int min_pairs,
                                      int fix_scale, double* d_model_out, uint8_t* d_inlier, double* d_chi2, int32_t* d_stats) {
    SLAM_REQUIRE(ctx, "slam_sim3_optimize_f64: null ctx");
    SLAM_REQUIRE(B >= 0 && B <= 65535 && M >= 0 && M <= (1 << 28), "bad sizes (B=%lld, M=%lld; B <= 65535)", (long long)B, (long long)M);
    SLAM_REQUIRE(th2 > 0.0 && th2 <= SO_DBL_MAX, "th2 must be positive and finite");
    SLAM_REQUIRE(it0 >= 0 && it_bad >= 0 && it_clean >= 0 && it0 <= 1000 && it_bad <= 1000 && it_clean <= 1000, "iteration counts must be in [0, 1000]");
    SLAM_REQUIRE(min_pairs >= 1, "min_pairs=%d must be at least 1", min_pairs);
    SLAM_REQUIRE(fx > 0.0 && fy > 0.0 && fx <= SO_DBL_MAX && fy <= SO_DBL_MAX && fabs(cx) <= SO_DBL_MAX && fabs(cy) <= SO_DBL_MAX,
                 "focal lengths must be positive and the intrinsics finite");
    SLAM_REQUIRE(d_offsets && d_model_in && d_model_out && d_stats && (M == 0 || (d_X1 && d_X2 && d_px1 && d_px2 && d_inlier && d_chi2)),
                 "slam_sim3_optimize_f64: null device pointer");
    if (B == 0) return SLAM_OK;
    SLAM_HIP(hipSetDevice(ctx->device));
    const geo_cam cam = {fx, fy, cx, cy};
    const so_params prm = {th2, it0, it_bad, it_clean, min_pairs, fix_scale != 0};
    if (M > 0) SLAM_HIP(hipMemsetAsync(d_inlier, 0, (size_t)M, ctx->stream));          // entries outside every candidate: 0
    so_optimize_kernel<<<(unsigned)B, SO_LANES, 0, ctx->stream>>>(d_offsets, (int)M, d_X1, d_X2, d_px1, d_px2, d_sigma2, d_model_in, cam, prm,
                                                                  d_model_out, d_inlier, d_chi2, d_stats, slam_index_error_counter(ctx));
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}
#endif  // SIM3_OPT_HOST_ONLY
