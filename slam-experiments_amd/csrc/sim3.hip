// sim3.hip — batched similarity alignment of two copies of the same map points on gfx950: ORB-SLAM's Sim3Solver (Horn's
// three-point closed form under RANSAC) for MANY loop candidates in one call, and a least-squares refit on the inliers.
// The reference has no call site: its driver prints the estimated translation beside the ground truth with no alignment
// (euroc.py:63-66), and its loop closing does not exist.
//
//   slam_sim3_threepoint_f64   the minimal solver on its own: X2 = s R X1 + t through three correspondences
//   slam_sim3_ransac_f64       H hypotheses per candidate, each scored on all correspondences in both images (pixels)
//   slam_sim3_refit_f64        Horn / Umeyama least squares over the selected correspondences, sums in a stated order
//
// All arithmetic is f64 and the file is compiled with floating-point contraction OFF (the pragma below), as pnp.hip and
// homography.hip: the winning hypothesis is solved again by the kernel that writes the result and must come out bit for bit
// as it was scored, and the host build of these routines (SIM3_HOST_ONLY, the test suite's twin) must give the device's
// bits.  For the same reason only + - * / sqrt are used: no acos / cbrt / library SVD.
//
// The closed form (Horn 1987, "Closed-form solution of absolute orientation using unit quaternions"):
//   1. centroids c1, c2; M = sum (x2 - c2)(x1 - c1)^T; d1 = sum |x1 - c1|^2;
//   2. Horn's symmetric 4x4 matrix N of the entries of M: the unit quaternion q that maximises q^T N q is the rotation that
//      maximises trace(R^T M).  N is diagonalised by cyclic Jacobi (a fixed number of sweeps, arrays indexed by unrolled
//      constants only), q is the eigenvector of the largest eigenvalue, R the rotation matrix of q / |q|.  A quaternion
//      cannot express a reflection: mirror-image point sets get the best PROPER rotation without a determinant fix, which
//      is why this route and not the SVD of M;
//   3. s = trace(R^T M) / d1 (Umeyama's least-squares scale, ORB-SLAM's asymmetric one), or 1 with fix_scale;
//   4. t = c2 - s R c1.
// The eigenvalues of N are s1 + s2 + s3', s1 - s2 - s3', -s1 + s2 - s3', -s1 - s2 + s3' (s_i the singular values of M,
// s3' = s3 sign(det M)): the two largest differ by 2 (s2 + s3'), which vanishes exactly when the best rotation is not
// unique (collinear points; a mirror image with s2 = s3).  The refit tests that gap; the minimal solver tests its two
// triangles instead, with P3P's rule.
#ifndef SIM3_HOST_ONLY               // a host build of the routines alone (the test suite's twin) defines it
#include "internal.h"
#endif
#include <math.h>
#include <stdint.h>
#include "geometry_common.h"         // sampler, Jacobi, range clamp, intrinsics, model key, dot, GEO_BIG / GEO_FLAT

#pragma clang fp contract(off)

#define S3_HD __host__ __device__ __forceinline__
// the shared sampler and intrinsics under this file's names, as its host twin calls them (three correspondences per sample)
#define s3_draw_sample geo_draw_sample<3>
typedef geo_cam s3_cam;
#define S3_GAP 1e-10                 // refit: (l1 - l2) / l1 of Horn's matrix below which the points count as collinear (sin, not sin^2)
#define S3_SWEEPS 12                 // cyclic Jacobi sweeps of the 4x4 (converged after 5 - 7 in f64; the rest are no-ops)
#define S3_REFIT_THREADS 256         // lanes of the refit's stated summation order (the host twin restates it)

// ---- Horn's closed form from the sums -----------------------------------------------------------------------------------------
S3_HD void s3_identity(double* model) {
#pragma unroll
    for (int i = 0; i < 12; i++) model[i] = (i % 5 == 0) ? 1.0 : 0.0;
    model[12] = 1.0;
}
// model [13] = row-major [R | t], s from the centroids c1, c2, M[i][j] = sum (x2 - c2)_i (x1 - c1)_j and d1 = sum |x1 - c1|^2
// (all finite).  l[2]: the two largest eigenvalues of Horn's matrix.  False (model untouched): a scale that is not finite
// and positive, or a model entry that is not finite.
S3_HD bool s3_from_sums(const double* c1, const double* c2, const double (&M)[3][3], double d1, int fix_scale, double* model, double* l) {
    double N[4][4], V[4][4];
    // Horn's S_ab = sum x1_a x2_b = M[b][a]
    const double Sxx = M[0][0], Sxy = M[1][0], Sxz = M[2][0], Syx = M[0][1], Syy = M[1][1], Syz = M[2][1], Szx = M[0][2], Szy = M[1][2], Szz = M[2][2];
    N[0][0] = (Sxx + Syy) + Szz; N[1][1] = (Sxx - Syy) - Szz; N[2][2] = (Syy - Sxx) - Szz; N[3][3] = (Szz - Sxx) - Syy;
    N[0][1] = N[1][0] = Syz - Szy; N[0][2] = N[2][0] = Szx - Sxz; N[0][3] = N[3][0] = Sxy - Syx;
    N[1][2] = N[2][1] = Sxy + Syx; N[1][3] = N[3][1] = Szx + Sxz; N[2][3] = N[3][2] = Syz + Szy;
    geo_jacobi<4, S3_SWEEPS>(N, V);
    double best = N[0][0], q[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
    int arg = 0;
#pragma unroll
    for (int j = 1; j < 4; j++) {
        const bool g = N[j][j] > best;
        best = g ? N[j][j] : best;
        arg = g ? j : arg;
#pragma unroll
        for (int k = 0; k < 4; k++) q[k] = g ? V[k][j] : q[k];
    }
    double second = -1.7976931348623157e308;
#pragma unroll
    for (int j = 0; j < 4; j++) second = (j != arg && N[j][j] > second) ? N[j][j] : second;
    l[0] = best; l[1] = second;
    const double inv = 1.0 / sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    const double w = q[0] * inv, x = q[1] * inv, y = q[2] * inv, z = q[3] * inv;
    double R[9];
    R[0] = ((w * w + x * x) - y * y) - z * z; R[1] = 2.0 * (x * y - w * z);             R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);             R[4] = ((w * w - x * x) + y * y) - z * z; R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);             R[7] = 2.0 * (y * z + w * x);             R[8] = ((w * w - x * x) - y * y) + z * z;
    const double r0 = (R[0] * M[0][0] + R[1] * M[0][1]) + R[2] * M[0][2];
    const double r1 = (R[3] * M[1][0] + R[4] * M[1][1]) + R[5] * M[1][2];
    const double r2 = (R[6] * M[2][0] + R[7] * M[2][1]) + R[8] * M[2][2];
    const double s = fix_scale ? 1.0 : ((r0 + r1) + r2) / d1;
    if (!(s > 0.0 && s < GEO_BIG)) return false;
    double T[3], chk = s;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        T[i] = c2[i] - s * ((R[3 * i] * c1[0] + R[3 * i + 1] * c1[1]) + R[3 * i + 2] * c1[2]);
        chk += ((fabs(R[3 * i]) + fabs(R[3 * i + 1])) + fabs(R[3 * i + 2])) + fabs(T[i]);
    }
    if (!(chk < GEO_BIG)) return false;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        model[4 * i] = R[3 * i]; model[4 * i + 1] = R[3 * i + 1]; model[4 * i + 2] = R[3 * i + 2]; model[4 * i + 3] = T[i];
    }
    model[12] = s;
    return true;
}

// ---- the minimal solver -------------------------------------------------------------------------------------------------------
// a triangle that is neither repeated nor collinear (pnp.hip's rule on the world points)
S3_HD bool s3_triangle(const double* P) {
    double e12[3], e13[3], e23[3], nw[3];
#pragma unroll
    for (int i = 0; i < 3; i++) { e12[i] = P[3 + i] - P[i]; e13[i] = P[6 + i] - P[i]; e23[i] = P[6 + i] - P[3 + i]; }
    const double a2 = geo_dot(e23, e23), b2 = geo_dot(e13, e13), c2 = geo_dot(e12, e12);
    geo_cross(e12, e13, nw);
    return geo_dot(nw, nw) > GEO_FLAT * (c2 * b2) && a2 > 0.0;
}
// P1, P2 [9]: three points of each set; model [13] (the identity with s = 1 when there is none)
S3_HD bool s3_threepoint(const double* P1, const double* P2, int fix_scale, double* model) {
    s3_identity(model);
    double big = 0.0;
#pragma unroll
    for (int i = 0; i < 9; i++) big += P1[i] * P1[i];
#pragma unroll
    for (int i = 0; i < 9; i++) big += P2[i] * P2[i];
    if (!(big < GEO_BIG)) return false;                           // NaN, inf, coordinates beyond 1e100
    if (!(s3_triangle(P1) && s3_triangle(P2))) return false;
    double c1[3], c2[3], a[3][3], b[3][3], M[3][3], l[2];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        c1[i] = ((P1[i] + P1[3 + i]) + P1[6 + i]) / 3.0;
        c2[i] = ((P2[i] + P2[3 + i]) + P2[6 + i]) / 3.0;
#pragma unroll
        for (int k = 0; k < 3; k++) { a[k][i] = P1[3 * k + i] - c1[i]; b[k][i] = P2[3 * k + i] - c2[i]; }
    }
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) M[i][j] = (b[0][i] * a[0][j] + b[1][i] * a[1][j]) + b[2][i] * a[2][j];
    const double d1 = (geo_dot(a[0], a[0]) + geo_dot(a[1], a[1])) + geo_dot(a[2], a[2]);
    return s3_from_sums(c1, c2, M, d1, fix_scale, model, l);
}

// ---- scoring and sampling (stated in the header) ---------------------------------------------------------------------------
// what a correspondence contributes whatever the hypothesis, c [12]: X1, X2, the projections (u1, v1), (u2, v2) of both and
// the two gates g1, g2 (0 when one of the two points is not in front of its camera: no squared error is below 0)
S3_HD void s3_stage(const double* x1, const double* x2, double sg1, double sg2, const geo_cam& cam, double chi2, double* c) {
    c[0] = x1[0]; c[1] = x1[1]; c[2] = x1[2]; c[3] = x2[0]; c[4] = x2[1]; c[5] = x2[2];
    c[6] = cam.fx * (x1[0] / x1[2]) + cam.cx; c[7] = cam.fy * (x1[1] / x1[2]) + cam.cy;
    c[8] = cam.fx * (x2[0] / x2[2]) + cam.cx; c[9] = cam.fy * (x2[1] / x2[2]) + cam.cy;
    const bool front = x1[2] > 0.0 && x2[2] > 0.0;
    c[10] = front ? chi2 * sg1 : 0.0;
    c[11] = front ? chi2 * sg2 : 0.0;
}
// a hypothesis in the form it is scored in, m [21]: A = s R (9), t (3), R (9); all zero = no model (depth 0, never an inlier)
S3_HD void s3_scoring_form(const double* model, bool ok, double* m) {
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            m[3 * i + j] = ok ? model[12] * model[4 * i + j] : 0.0;
            m[12 + 3 * i + j] = ok ? model[4 * i + j] : 0.0;
        }
        m[9 + i] = ok ? model[4 * i + 3] : 0.0;
    }
}
S3_HD bool s3_inlier(const double* m, const double* c, const geo_cam& cam) {
    const double* A = m;
    const double* t = m + 9;
    const double* R = m + 12;
    const double x = ((A[0] * c[0] + A[1] * c[1]) + A[2] * c[2]) + t[0];
    const double y = ((A[3] * c[0] + A[4] * c[1]) + A[5] * c[2]) + t[1];
    const double z = ((A[6] * c[0] + A[7] * c[1]) + A[8] * c[2]) + t[2];
    const double du2 = (cam.fx * (x / z) + cam.cx) - c[8], dv2 = (cam.fy * (y / z) + cam.cy) - c[9];
    const double y0 = c[3] - t[0], y1 = c[4] - t[1], y2 = c[5] - t[2];
    const double wx = (R[0] * y0 + R[3] * y1) + R[6] * y2;
    const double wy = (R[1] * y0 + R[4] * y1) + R[7] * y2;
    const double wz = (R[2] * y0 + R[5] * y1) + R[8] * y2;
    const double du1 = (cam.fx * (wx / wz) + cam.cx) - c[6], dv1 = (cam.fy * (wy / wz) + cam.cy) - c[7];
    return z > 0.0 && wz > 0.0 && (du2 * du2 + dv2 * dv2) < c[11] && (du1 * du1 + dv1 * dv1) < c[10];
}
// hypothesis h of a candidate of n correspondences X1 / X2 [n,3]: its sample drawn and solved
S3_HD bool s3_solve_hypothesis(const double* X1, const double* X2, int n, int fix_scale, uint64_t seed, int h, double* model) {
    int idx[3] = {0, 0, 0};
    geo_draw_sample<3>(seed, h, n, idx);
    double P1[9], P2[9];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double* p = X1 + 3 * (size_t)idx[k];
        const double* q = X2 + 3 * (size_t)idx[k];
        P1[3 * k] = p[0]; P1[3 * k + 1] = p[1]; P1[3 * k + 2] = p[2];
        P2[3 * k] = q[0]; P2[3 * k + 1] = q[1]; P2[3 * k + 2] = q[2];
    }
    return s3_threepoint(P1, P2, fix_scale, model);
}

// ---- the refit's pieces: what one lane adds per correspondence, and the model from the combined sums ------------------------
// pass 1, a [6]: the coordinate sums of both sets
S3_HD void s3_acc_points(double* a, const double* x1, const double* x2) {
    a[0] += x1[0]; a[1] += x1[1]; a[2] += x1[2]; a[3] += x2[0]; a[4] += x2[1]; a[5] += x2[2];
}
// pass 2, a [11]: M row-major (9), d1, d2 of the points centred on c [6]
S3_HD void s3_acc_centred(double* a, const double* x1, const double* x2, const double* c) {
    const double p[3] = {x1[0] - c[0], x1[1] - c[1], x1[2] - c[2]};
    const double q[3] = {x2[0] - c[3], x2[1] - c[4], x2[2] - c[5]};
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) a[3 * i + j] += q[i] * p[j];
    a[9] += geo_dot(p, p);
    a[10] += geo_dot(q, q);
}
// n selected points with centroids c [6] and centred sums a [11]; model [13] (the identity with s = 1 when not ok)
S3_HD bool s3_refit_model(int n, const double* c, const double* a, int fix_scale, double* model) {
    s3_identity(model);
    if (n < 3) return false;
    const double chk = ((geo_dot(c, c) + geo_dot(c + 3, c + 3)) + a[9]) + a[10];
    if (!(chk < GEO_BIG) || !(a[9] > 0.0 && a[10] > 0.0)) return false;        // NaN / inf / beyond 1e100; all points of a set equal
    double M[3][3], l[2], out[13];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) M[i][j] = a[3 * i + j];
    if (!s3_from_sums(c, c + 3, M, a[9], fix_scale, out, l)) return false;
    if (!(l[0] > 0.0 && (l[0] - l[1]) > S3_GAP * l[0])) return false;           // collinear: the best rotation is not unique
#pragma unroll
    for (int i = 0; i < 13; i++) model[i] = out[i];
    return true;
}

#ifndef SIM3_HOST_ONLY
// =============================================================== kernels =====================================================
#define S3_LANES 64
#define S3_THREADS 256               // hypotheses per block of the RANSAC kernel
#define S3_CHUNK 256                 // correspondences staged in LDS at a time (12 doubles each: 24 KiB)

__global__ __launch_bounds__(S3_LANES) void s3_threepoint_kernel(int S, const double* __restrict__ X1, const double* __restrict__ X2,
                                                                 int fix_scale, double* __restrict__ model, int* __restrict__ ok) {
    const int s = blockIdx.x * S3_LANES + threadIdx.x;
    if (s >= S) return;
    double P1[9], P2[9], m[13];
#pragma unroll
    for (int i = 0; i < 9; i++) { P1[i] = X1[(size_t)s * 9 + i]; P2[i] = X2[(size_t)s * 9 + i]; }
    ok[s] = s3_threepoint(P1, P2, fix_scale, m) ? 1 : 0;
#pragma unroll
    for (int i = 0; i < 13; i++) model[(size_t)s * 13 + i] = m[i];
}

// grid (ceil(H / 256), B): lane = one hypothesis of candidate blockIdx.y; the candidate's correspondences pass through LDS in
// chunks (staged once per block: the four projections of the points themselves do not depend on the hypothesis) and are
// read as broadcasts
__global__ __launch_bounds__(S3_THREADS) void s3_ransac_kernel(const int* __restrict__ offsets, int M, const double* __restrict__ X1_all,
                                                               const double* __restrict__ X2_all, const double* __restrict__ sigma2, geo_cam cam,
                                                               int H, double chi2, int fix_scale, uint64_t seed,
                                                               unsigned long long* __restrict__ keys, int* __restrict__ models) {
    __shared__ __attribute__((aligned(16))) double s_c[S3_CHUNK * 12];
    __shared__ unsigned long long s_key;
    __shared__ int s_models;
    const int b = blockIdx.y, tid = threadIdx.x, h = blockIdx.x * S3_THREADS + tid;
    int first, last; bool bad;
    geo_range(offsets, b, M, &first, &last, &bad);
    const int n = last - first;
    if (n < 3) return;                                  // block-uniform
    if (tid == 0) { s_key = 0ull; s_models = 0; }
    const double* X1 = X1_all + 3 * (size_t)first;
    const double* X2 = X2_all + 3 * (size_t)first;
    const double* sg = sigma2 ? sigma2 + 2 * (size_t)first : nullptr;
    double model[13], m[21];
    const bool ok = s3_solve_hypothesis(X1, X2, n, fix_scale, seed, min(h, H - 1), model);   // the spare lanes solve the last hypothesis again
    s3_scoring_form(model, ok, m);
    int count = 0;
    for (int base = 0; base < n; base += S3_CHUNK) {
        const int cm = min(S3_CHUNK, n - base);
        __syncthreads();                                // the chunk before is consumed (and the first time: s_key is set)
        for (int i = tid; i < cm; i += S3_THREADS) {
            double c[12];
            s3_stage(X1 + 3 * (size_t)(base + i), X2 + 3 * (size_t)(base + i), sg ? sg[2 * (size_t)(base + i)] : 1.0,
                     sg ? sg[2 * (size_t)(base + i) + 1] : 1.0, cam, chi2, c);
#pragma unroll
            for (int k = 0; k < 12; k++) s_c[12 * i + k] = c[k];
        }
        __syncthreads();
        for (int i = 0; i < cm; i++) count += s3_inlier(m, s_c + 12 * i, cam) ? 1 : 0;
    }
    if (h < H && ok) {
        atomicMax(&s_key, geo_key2(count, h));
        atomicAdd(&s_models, 1);
    }
    __syncthreads();
    if (tid == 0) {
        if (s_key) atomicMax(&keys[b], s_key);          // integer maxima and sums: the order of arrival does not matter
        if (s_models) atomicAdd(&models[b], s_models);
    }
}

// grid B: the winner of candidate b solved again (every lane the same hypothesis), its model, mask and stats written
__global__ __launch_bounds__(S3_LANES) void s3_ransac_result_kernel(const int* __restrict__ offsets, int M, const double* __restrict__ X1_all,
                                                                    const double* __restrict__ X2_all, const double* __restrict__ sigma2,
                                                                    geo_cam cam, double chi2, int fix_scale, uint64_t seed,
                                                                    const unsigned long long* __restrict__ keys, const int* __restrict__ models,
                                                                    double* __restrict__ model_out, uint8_t* __restrict__ inlier,
                                                                    int* __restrict__ stats, unsigned int* __restrict__ index_errors) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int first, last; bool bad;
    geo_range(offsets, b, M, &first, &last, &bad);
    if (bad && lane == 0) atomicAdd(index_errors, 1u);
    const int n = last - first;
    const unsigned long long key = n >= 3 ? keys[b] : 0ull;
    double model[13], m[21];
    if (!key) {
        s3_identity(model);
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 13; i++) model_out[13 * (size_t)b + i] = model[i];
            stats[4 * b] = 0; stats[4 * b + 1] = -1; stats[4 * b + 2] = -1; stats[4 * b + 3] = 0;
        }
        for (int i = lane; i < n; i += S3_LANES) inlier[first + i] = 0;
        return;
    }
    const int count = geo_key_count(key), h = geo_key2_h(key);
    const double* X1 = X1_all + 3 * (size_t)first;
    const double* X2 = X2_all + 3 * (size_t)first;
    const double* sg = sigma2 ? sigma2 + 2 * (size_t)first : nullptr;
    const bool ok = s3_solve_hypothesis(X1, X2, n, fix_scale, seed, h, model);
    s3_scoring_form(model, ok, m);
    for (int i = lane; i < n; i += S3_LANES) {
        double c[12];
        s3_stage(X1 + 3 * (size_t)i, X2 + 3 * (size_t)i, sg ? sg[2 * (size_t)i] : 1.0, sg ? sg[2 * (size_t)i + 1] : 1.0, cam, chi2, c);
        inlier[first + i] = s3_inlier(m, c, cam) ? 1 : 0;
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 13; i++) model_out[13 * (size_t)b + i] = model[i];
        stats[4 * b] = count; stats[4 * b + 1] = h; stats[4 * b + 2] = 0; stats[4 * b + 3] = models[b];
    }
}

// the lanes' partial sums combined: at each stride 128, 64, ..., 1 lane l < stride adds lane l + stride to its own
template <int K>
__device__ __forceinline__ void s3_tree(double (*s)[S3_REFIT_THREADS], const double* a, int tid) {
    __syncthreads();                                    // the values of the pass before are read
#pragma unroll
    for (int k = 0; k < K; k++) s[k][tid] = a[k];
    __syncthreads();
    for (int stride = S3_REFIT_THREADS / 2; stride >= 1; stride >>= 1) {
        if (tid < stride) {
#pragma unroll
            for (int k = 0; k < K; k++) s[k][tid] += s[k][tid + stride];
        }
        __syncthreads();
    }
}

// grid B, one block per candidate: two passes over its selected correspondences (centroids, then the centred sums), each
// in the stated order - lane l takes the positions l, l + 256, l + 512, ... of the candidate in ascending order, then the tree
__global__ __launch_bounds__(S3_REFIT_THREADS) void s3_refit_kernel(const int* __restrict__ offsets, int M, const double* __restrict__ X1_all,
                                                                    const double* __restrict__ X2_all, const uint8_t* __restrict__ mask,
                                                                    int fix_scale, double* __restrict__ model_out, int* __restrict__ stats,
                                                                    unsigned int* __restrict__ index_errors) {
    __shared__ double s_sum[11][S3_REFIT_THREADS];
    __shared__ int s_cnt[S3_REFIT_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    int first, last; bool bad;
    geo_range(offsets, b, M, &first, &last, &bad);
    if (bad && tid == 0) atomicAdd(index_errors, 1u);
    const int n = last - first;
    const double* X1 = X1_all + 3 * (size_t)first;
    const double* X2 = X2_all + 3 * (size_t)first;
    const uint8_t* sel = mask ? mask + first : nullptr;
    double a[11];
#pragma unroll
    for (int k = 0; k < 11; k++) a[k] = 0.0;
    int cnt = 0;
    for (int i = tid; i < n; i += S3_REFIT_THREADS) {
        if (sel && !sel[i]) continue;
        s3_acc_points(a, X1 + 3 * (size_t)i, X2 + 3 * (size_t)i);
        cnt++;
    }
    s_cnt[tid] = cnt;
    s3_tree<6>(s_sum, a, tid);
    for (int stride = S3_REFIT_THREADS / 2; stride >= 1; stride >>= 1) {      // (integers: any order gives the same count)
        if (tid < stride) s_cnt[tid] += s_cnt[tid + stride];
        __syncthreads();
    }
    const int used = s_cnt[0];
    double c[6];
#pragma unroll
    for (int k = 0; k < 6; k++) c[k] = s_sum[k][0] / (double)used;
#pragma unroll
    for (int k = 0; k < 11; k++) a[k] = 0.0;
    for (int i = tid; i < n; i += S3_REFIT_THREADS) {
        if (sel && !sel[i]) continue;
        s3_acc_centred(a, X1 + 3 * (size_t)i, X2 + 3 * (size_t)i, c);
    }
    s3_tree<11>(s_sum, a, tid);
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 11; k++) a[k] = s_sum[k][0];
        double model[13];
        const bool ok = s3_refit_model(used, c, a, fix_scale, model);
#pragma unroll
        for (int i = 0; i < 13; i++) model_out[13 * (size_t)b + i] = model[i];
        stats[2 * b] = used; stats[2 * b + 1] = ok ? 1 : 0;
    }
}

// =============================================================== entry points ================================================
#include "geometry_host.h"           // the checks, the vote block and the launch shapes the four estimators' entry points share

extern "C" int slam_sim3_threepoint_f64(slam_ctx* ctx, int64_t S, const double* d_X1, const double* d_X2, int fix_scale, double* d_model,
                                        int32_t* d_ok) {
    GEO_SAMPLE_SIZES(ctx, S);
    GEO_POINTERS(S, d_X1 && d_X2 && d_model && d_ok);
    SLAM_HIP(hipSetDevice(ctx->device));
    s3_threepoint_kernel<<<geo_blocks(S, S3_LANES), S3_LANES, 0, ctx->stream>>>((int)S, d_X1, d_X2, fix_scale != 0, d_model, d_ok);
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

extern "C" int slam_sim3_ransac_f64(slam_ctx* ctx, int64_t B, const int32_t* d_offsets, const double* d_X1, const double* d_X2, int64_t M,
                                    const double* d_sigma2, double fx, double fy, double cx, double cy, int H, double chi2_gate, int fix_scale,
                                    uint64_t seed, double* d_model, uint8_t* d_inlier, int32_t* d_stats) {
    GEO_RANSAC_SIZES(ctx, B, M, H);
    SLAM_REQUIRE(chi2_gate > 0.0 && fx > 0.0 && fy > 0.0, "chi2 gate and focal lengths must be positive");
    GEO_POINTERS(B, d_offsets && d_model && d_stats && (M == 0 || (d_X1 && d_X2 && d_inlier)));
    SLAM_HIP(hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> lk(ctx->call_mu);        // the workspace holds the keys and the model counts
    void* ws = nullptr;
    if (int rc = slam_workspace(ctx, geo_vote_bytes(0, B), &ws)) return rc;
    unsigned long long* keys; int* models;
    if (int rc = geo_vote_block(ctx, ws, 0, B, true, M, d_inlier, &keys, &models)) return rc;
    const geo_cam cam = {fx, fy, cx, cy};
    s3_ransac_kernel<<<geo_vote_grid(H, S3_THREADS, B), S3_THREADS, 0, ctx->stream>>>(d_offsets, (int)M, d_X1, d_X2, d_sigma2, cam, H, chi2_gate,
                                                                                      fix_scale != 0, seed, keys, models);
    SLAM_HIP(hipGetLastError());
    s3_ransac_result_kernel<<<(unsigned)B, S3_LANES, 0, ctx->stream>>>(d_offsets, (int)M, d_X1, d_X2, d_sigma2, cam, chi2_gate, fix_scale != 0, seed,
                                                                      keys, models, d_model, d_inlier, d_stats, slam_index_error_counter(ctx));
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

extern "C" int slam_sim3_refit_f64(slam_ctx* ctx, int64_t B, const int32_t* d_offsets, const double* d_X1, const double* d_X2, int64_t M,
                                   const uint8_t* d_mask, int fix_scale, double* d_model, int32_t* d_stats) {
    GEO_CANDIDATE_SIZES(ctx, B, 1 << 24, M);
    GEO_POINTERS(B, d_offsets && d_model && d_stats && (M == 0 || (d_X1 && d_X2)));
    SLAM_HIP(hipSetDevice(ctx->device));
    s3_refit_kernel<<<(unsigned)B, S3_REFIT_THREADS, 0, ctx->stream>>>(d_offsets, (int)M, d_X1, d_X2, d_mask, fix_scale != 0, d_model, d_stats,
                                                                     slam_index_error_counter(ctx));
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}
#endif  // SIM3_HOST_ONLY
