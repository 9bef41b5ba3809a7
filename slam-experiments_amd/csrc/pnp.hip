// pnp.hip — batched absolute pose from 2D-3D correspondences on gfx950: cv2.solvePnPRansac (SOLVEPNP_P3P) for MANY
// candidates in one call.  The reference has no call site (the nearest is _reinitialize_from_keyframe, frontend.py:223-229,
// which drops the map because it has no such estimate).
//
//   slam_pnp_p3p_f64      the minimal solver on its own: every pose that sees three world points along three bearings
//   slam_pnp_ransac_f64   H hypotheses per candidate, every solution scored on all correspondences (reprojection in pixels)
//
// All arithmetic is f64 and the file is compiled with floating-point contraction OFF (the pragma below), as two_view.hip: the
// winning hypothesis is solved again by the kernel that writes the result and must come out bit for bit as it was scored, and
// the host build of these routines (PNP_HOST_ONLY, the test suite's twin) must give the device's bits.  For the same reason
// the solver uses + - * / sqrt only: no acos / cos / cbrt / pow, whose library versions differ between hosts and the device.
//
// The solver (Grunert's elimination, the quartic built by polynomial arithmetic instead of hand-expanded coefficients):
//   1. unit bearings f1 f2 f3, their cosines ca = f2.f3, cb = f1.f3, cg = f1.f2, squared world distances a2 = |X2 - X3|^2,
//      b2 = |X1 - X3|^2, c2 = |X1 - X2|^2.  With depths s1, s2 = u s1, s3 = v s1 the law of cosines gives three equations;
//      the difference of two of them is linear in u:  u = N(v) / D(v),  N = (1 + K) - 2 K cb v + (K - 1) v^2,  K = (a2 - c2) / b2,
//      D = 2 (cg - ca v);
//   2. substituted into the third:  N^2 + D^2 (1 - q (1 + v^2 - 2 cb v)) - 2 cg N D = 0,  q = c2 / b2: a quartic in v;
//   3. its real roots, ascending: the roots of each derivative bracket the roots of the one below it (degree 1 up to 4),
//      every bracket closed by a safeguarded Newton iteration - bounded loops, no recursion (the scheme of tv_real_roots, here
//      on register arrays that only unrolled constants index);
//   4. per root v > 0 with u > 0: s1 = sqrt(b2 / (1 + v^2 - 2 cb v)), then up to three Newton steps on the three law-of-cosines
//      equations themselves in (s1, s2, s3) (the expanded coefficients lose digits the equations still have; a step is kept
//      only if it lowers the residual);
//   5. R from two orthonormal frames (Gram-Schmidt on the world triangle and on the camera-frame triangle s_i f_i: orthonormal
//      to rounding whatever the root's accuracy), t from the centroids.
// One sample per lane, everything in registers: no run-time-indexed array, so nothing goes to scratch.
#ifndef PNP_HOST_ONLY                // a host build of the routines alone (the test suite's twin) defines it
#include "internal.h"
#endif
#include <math.h>
#include <stdint.h>
#include "geometry_common.h"         // sampler, range clamp, intrinsics, model key, three-vectors, GEO_BIG / GEO_FLAT

#pragma clang fp contract(off)

#define PNP_HD __host__ __device__ __forceinline__
// the shared sampler and intrinsics under this file's names, as its host twin calls them (three correspondences per sample)
#define pnp_draw_sample geo_draw_sample<3>
typedef geo_cam pnp_cam;
#define PNP_POLISH_STEPS 3

// ---- real roots of a quartic ------------------------------------------------------------------------------------------------
template <int N>
PNP_HD double pnp_horner(const double* c, double x) {      // N coefficients, ascending
    double r = c[N - 1];
#pragma unroll
    for (int i = N - 2; i >= 0; i--) r = r * x + c[i];
    return r;
}
PNP_HD bool pnp_neg(double v) { return v < 0.0; }
// the root of p (N coefficients; dp its derivative) in (lo, hi), where p is negative at lo iff neg_lo and changes sign: Newton
// steps kept inside the bracket, bisection when one leaves it or gains too little
template <int N>
PNP_HD double pnp_close(const double* p, const double* dp, double lo, double hi, bool neg_lo) {
    double x = 0.5 * (lo + hi), dxold = fabs(hi - lo), dx = dxold;
    double f = pnp_horner<N>(p, x), df = pnp_horner<N - 1>(dp, x);
    for (int it = 0; it < 200; it++) {
        const double lo_side = neg_lo ? lo : hi, hi_side = neg_lo ? hi : lo;      // f < 0 at lo_side, f >= 0 at hi_side
        const bool out = ((x - hi_side) * df - f) * ((x - lo_side) * df - f) > 0.0;
        double xn;
        if (out || !(fabs(2.0 * f) <= fabs(dxold * df))) {
            dxold = dx;
            dx = 0.5 * (hi - lo);
            xn = lo + dx;
            if (xn == lo || xn == hi) return x;
        } else {
            dxold = dx;
            dx = f / df;
            xn = x - dx;
            if (xn == x) return x;
            if (!(xn > lo && xn < hi)) { dx = 0.5 * (hi - lo); xn = lo + dx; if (xn == lo || xn == hi) return x; }
        }
        x = xn;
        f = pnp_horner<N>(p, x);
        df = pnp_horner<N - 1>(dp, x);
        if (f == 0.0) return x;
        if (pnp_neg(f) == neg_lo) lo = x; else hi = x;
    }
    return x;
}
// the real roots of p (degree N - 1, leading coefficient non-zero) from the m ascending real roots crit[] of its derivative
// (m <= N - 2; none: any break point will do); out[] ascending, returns the count
template <int N>
PNP_HD int pnp_level(const double* p, const double* dp, const double* crit, int m, double* out) {
    constexpr int deg = N - 1;
    const bool none = m == 0;
    const int mm = none ? 1 : m;
    const bool neg_pinf = pnp_neg(p[N - 1]), neg_ninf = (deg & 1) ? !neg_pinf : neg_pinf;
    int found = 0;
    double prev = 0.0;
    bool neg_prev = neg_ninf;
#pragma unroll
    for (int i = 0; i < deg; i++) {
        if (i > mm) continue;
        const bool last = i == mm;
        const double t = (last || none) ? 0.0 : crit[i < deg - 1 ? i : deg - 2];
        const bool neg_t = last ? neg_pinf : pnp_neg(pnp_horner<N>(p, t));
        if (neg_t != neg_prev && found < deg) {
            double lo = prev, hi = t;
            bool ok = true;
            if (i == 0) {                                        // (-inf, t): walk left until the sign is the one at -inf
                double step = 1.0 + fabs(t);
                lo = t - step;
                int guard = 0;
                while (pnp_neg(pnp_horner<N>(p, lo)) != neg_ninf && guard++ < 1100) { step *= 2.0; lo = t - step; }
                ok = guard < 1100 && isfinite(lo);
            } else if (last) {                                   // (prev, +inf)
                double step = 1.0 + fabs(prev);
                hi = prev + step;
                int guard = 0;
                while (pnp_neg(pnp_horner<N>(p, hi)) != neg_pinf && guard++ < 1100) { step *= 2.0; hi = prev + step; }
                ok = guard < 1100 && isfinite(hi);
            }
            if (ok) {
                const double r = pnp_close<N>(p, dp, lo, hi, neg_prev);
#pragma unroll
                for (int k = 0; k < deg; k++)
                    if (k == found) out[k] = r;
                found++;
            }
        }
        prev = t;
        neg_prev = neg_t;
    }
    return found;
}
PNP_HD int pnp_quartic_roots(const double* p, double* r) {      // p[5] ascending; r[4] ascending, returns the count
    const double chk = (((p[0] + p[1]) + p[2]) + p[3]) + p[4];
    if (!(fabs(p[4]) > 0.0) || !isfinite(chk)) return 0;
    const double d1[4] = {p[1], 2.0 * p[2], 3.0 * p[3], 4.0 * p[4]};
    const double d2[3] = {d1[1], 2.0 * d1[2], 3.0 * d1[3]};
    const double d3[2] = {d2[1], 2.0 * d2[2]};
    const double r3[1] = {-d3[0] / d3[1]};                      // the linear one (d3[1] = 24 p[4], non-zero)
    double r2[2] = {0.0, 0.0}, r1[3] = {0.0, 0.0, 0.0};
    const int m2 = pnp_level<3>(d2, d3, r3, 1, r2);
    const int m1 = pnp_level<4>(d1, d2, r2, m2, r1);
    return pnp_level<5>(p, d1, r1, m1, r);
}

// ---- the minimal solver -------------------------------------------------------------------------------------------------------
// orthonormal frame of the triangle (p1, p2, p3): e1 along p2 - p1, e3 its normal, e2 = e3 x e1
PNP_HD void pnp_frame(const double* p1, const double* p2, const double* p3, double* e1, double* e2, double* e3) {
    double d[3];
#pragma unroll
    for (int i = 0; i < 3; i++) { e1[i] = p2[i] - p1[i]; d[i] = p3[i] - p1[i]; }
    geo_cross(e1, d, e3);
    geo_unit(e1);
    geo_unit(e3);
    geo_cross(e3, e1, e2);
}
// residuals of the three law-of-cosines equations at depths s; returns |F|^2
PNP_HD double pnp_residual(const double* s, double ca, double cb, double cg, double a2, double b2, double c2, double* F) {
    F[0] = ((s[1] * s[1] + s[2] * s[2]) - 2.0 * (s[1] * s[2]) * ca) - a2;
    F[1] = ((s[0] * s[0] + s[2] * s[2]) - 2.0 * (s[0] * s[2]) * cb) - b2;
    F[2] = ((s[0] * s[0] + s[1] * s[1]) - 2.0 * (s[0] * s[1]) * cg) - c2;
    return (F[0] * F[0] + F[1] * F[1]) + F[2] * F[2];
}
// X [9]: three world points; x [6]: their normalised image points; pose [48]: up to four [R|t] (row-major 3x4, X_cam = R X + t),
// ascending in v = s3 / s1, unused slots zero; returns the number of solutions
PNP_HD int pnp_p3p(const double* X, const double* x, double* pose) {
#pragma unroll
    for (int i = 0; i < 48; i++) pose[i] = 0.0;
    double big = 0.0;
#pragma unroll
    for (int i = 0; i < 9; i++) big += X[i] * X[i];
#pragma unroll
    for (int i = 0; i < 6; i++) big += x[i] * x[i];
    if (!(big < GEO_BIG)) return 0;                              // NaN, inf, coordinates beyond 1e100
    double f[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        f[k][0] = x[2 * k]; f[k][1] = x[2 * k + 1]; f[k][2] = 1.0;
        geo_unit(f[k]);
    }
    double e12[3], e13[3], e23[3], nw[3];
#pragma unroll
    for (int i = 0; i < 3; i++) { e12[i] = X[3 + i] - X[i]; e13[i] = X[6 + i] - X[i]; e23[i] = X[6 + i] - X[3 + i]; }
    const double a2 = geo_dot(e23, e23), b2 = geo_dot(e13, e13), c2 = geo_dot(e12, e12);
    geo_cross(e12, e13, nw);
    if (!(geo_dot(nw, nw) > GEO_FLAT * (c2 * b2)) || !(a2 > 0.0)) return 0;          // repeated or collinear world points
    const double ca = geo_dot(f[1], f[2]), cb = geo_dot(f[0], f[2]), cg = geo_dot(f[0], f[1]);
    {
        double c01[3], c02[3], c12[3];
        geo_cross(f[0], f[1], c01); geo_cross(f[0], f[2], c02); geo_cross(f[1], f[2], c12);
        if (!(geo_dot(c01, c01) > GEO_FLAT && geo_dot(c02, c02) > GEO_FLAT && geo_dot(c12, c12) > GEO_FLAT)) return 0;   // repeated image points
    }
    const double K = (a2 - c2) / b2, q = c2 / b2;
    const double Np[3] = {1.0 + K, -2.0 * (K * cb), K - 1.0};
    const double Dp[2] = {2.0 * cg, -2.0 * ca};
    const double Wp[3] = {1.0 - q, 2.0 * (q * cb), -q};
    double NN[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, DD[3] = {0.0, 0.0, 0.0}, ND[4] = {0.0, 0.0, 0.0, 0.0}, P[5];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) NN[i + j] += Np[i] * Np[j];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) DD[i + j] += Dp[i] * Dp[j];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) ND[i + j] += Np[i] * Dp[j];
#pragma unroll
    for (int i = 0; i < 5; i++) P[i] = NN[i] - (i < 4 ? 2.0 * (cg * ND[i]) : 0.0);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) P[i + j] += DD[i] * Wp[j];
    double vs[4] = {0.0, 0.0, 0.0, 0.0};
    const int nr = pnp_quartic_roots(P, vs);
    double Xc[3], w1[3], w2[3], w3[3];
#pragma unroll
    for (int i = 0; i < 3; i++) Xc[i] = ((X[i] + X[3 + i]) + X[6 + i]) / 3.0;
    pnp_frame(X, X + 3, X + 6, w1, w2, w3);
    int kept = 0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        if (r >= nr) continue;
        const double v = vs[r];
        if (!(v > 0.0)) continue;
        const double u = pnp_horner<3>(Np, v) / pnp_horner<2>(Dp, v);
        const double den = (1.0 + v * v) - 2.0 * (cb * v);
        double s[3], F[3];
        s[0] = sqrt(b2 / den); s[1] = u * s[0]; s[2] = v * s[0];
        if (!(u > 0.0) || !isfinite((s[0] + s[1]) + s[2])) continue;
        double n2 = pnp_residual(s, ca, cb, cg, a2, b2, c2, F);
        for (int it = 0; it < PNP_POLISH_STEPS; it++) {
            // J = dF/ds (zero diagonal), solved by its adjugate
            const double j01 = 2.0 * (s[1] - s[2] * ca), j02 = 2.0 * (s[2] - s[1] * ca);
            const double j10 = 2.0 * (s[0] - s[2] * cb), j12 = 2.0 * (s[2] - s[0] * cb);
            const double j20 = 2.0 * (s[0] - s[1] * cg), j21 = 2.0 * (s[1] - s[0] * cg);
            const double det = j01 * (j12 * j20) + j02 * (j10 * j21);
            const double d0 = (((-(j12 * j21)) * F[0] + (j02 * j21) * F[1]) + (j01 * j12) * F[2]) / det;
            const double d1 = (((j12 * j20) * F[0] + (-(j02 * j20)) * F[1]) + (j02 * j10) * F[2]) / det;
            const double d2 = (((j10 * j21) * F[0] + (j01 * j20) * F[1]) + (-(j01 * j10)) * F[2]) / det;
            const double sn[3] = {s[0] - d0, s[1] - d1, s[2] - d2};
            double Fn[3];
            const double m2 = pnp_residual(sn, ca, cb, cg, a2, b2, c2, Fn);
            if (!(m2 < n2)) break;                               // (also a NaN step)
#pragma unroll
            for (int i = 0; i < 3; i++) { s[i] = sn[i]; F[i] = Fn[i]; }
            n2 = m2;
        }
        if (!(s[0] > 0.0 && s[1] > 0.0 && s[2] > 0.0)) continue;
        double Y[3][3], Yc[3], c1[3], c2v[3], c3[3], T[12];
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
            for (int i = 0; i < 3; i++) Y[k][i] = s[k] * f[k][i];
#pragma unroll
        for (int i = 0; i < 3; i++) Yc[i] = ((Y[0][i] + Y[1][i]) + Y[2][i]) / 3.0;
        pnp_frame(Y[0], Y[1], Y[2], c1, c2v, c3);
        double chk = 0.0;
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int j = 0; j < 3; j++) T[4 * i + j] = (c1[i] * w1[j] + c2v[i] * w2[j]) + c3[i] * w3[j];
            T[4 * i + 3] = Yc[i] - ((T[4 * i] * Xc[0] + T[4 * i + 1] * Xc[1]) + T[4 * i + 2] * Xc[2]);
        }
#pragma unroll
        for (int i = 0; i < 12; i++) chk += T[i];
        if (!isfinite(chk)) continue;
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k == kept) {
#pragma unroll
                for (int i = 0; i < 12; i++) pose[12 * k + i] = T[i];
            }
        kept++;
    }
    return kept;
}

// ---- scoring and sampling (stated in the header) ---------------------------------------------------------------------------
PNP_HD bool pnp_inlier(const double* T, double X, double Y, double Z, double u, double v, const geo_cam& cam, double thr2) {
    const double xc = ((T[0] * X + T[1] * Y) + T[2] * Z) + T[3];
    const double yc = ((T[4] * X + T[5] * Y) + T[6] * Z) + T[7];
    const double zc = ((T[8] * X + T[9] * Y) + T[10] * Z) + T[11];
    const double du = (cam.fx * (xc / zc) + cam.cx) - u, dv = (cam.fy * (yc / zc) + cam.cy) - v;
    return zc > 0.0 && (du * du + dv * dv) < thr2;
}
// hypothesis h of a candidate of n correspondences X [n,3] / px [n,2]: its sample drawn, normalised and solved
PNP_HD int pnp_solve_hypothesis(const double* X, const double* px, int n, const geo_cam& cam, uint64_t seed, int h, double* pose) {
    int idx[3] = {0, 0, 0};
    geo_draw_sample<3>(seed, h, n, idx);
    double P[9], x[6];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double* p = X + 3 * (size_t)idx[k];
        const double* m = px + 2 * (size_t)idx[k];
        P[3 * k] = p[0]; P[3 * k + 1] = p[1]; P[3 * k + 2] = p[2];
        x[2 * k] = (m[0] - cam.cx) / cam.fx; x[2 * k + 1] = (m[1] - cam.cy) / cam.fy;
    }
    return pnp_p3p(P, x, pose);
}

#ifndef PNP_HOST_ONLY
// =============================================================== kernels =====================================================
#define PNP_LANES 64
#define PNP_THREADS 256              // hypotheses per block of the RANSAC kernel
#define PNP_CHUNK 256                // correspondences staged in LDS at a time (5 doubles each: 10 KiB)

__global__ __launch_bounds__(PNP_LANES) void pnp_p3p_kernel(int S, const double* __restrict__ X, const double* __restrict__ x,
                                                            double* __restrict__ pose, int* __restrict__ nsol) {
    const int s = blockIdx.x * PNP_LANES + threadIdx.x;
    if (s >= S) return;
    double P[9], m[6], T[48];
#pragma unroll
    for (int i = 0; i < 9; i++) P[i] = X[(size_t)s * 9 + i];
#pragma unroll
    for (int i = 0; i < 6; i++) m[i] = x[(size_t)s * 6 + i];
    nsol[s] = pnp_p3p(P, m, T);
#pragma unroll
    for (int i = 0; i < 48; i++) pose[(size_t)s * 48 + i] = T[i];
}

// grid (ceil(H / 256), B): lane = one hypothesis of candidate blockIdx.y; the candidate's correspondences pass through LDS in
// chunks and are read as broadcasts (a wave's 64 hypotheses score the same correspondence at the same time)
__global__ __launch_bounds__(PNP_THREADS) void pnp_ransac_kernel(const int* __restrict__ offsets, int M, const double* __restrict__ X_all,
                                                                 const double* __restrict__ px_all, geo_cam cam, int H, double thr2,
                                                                 uint64_t seed, unsigned long long* __restrict__ keys,
                                                                 int* __restrict__ models) {
    __shared__ double s_pt[PNP_CHUNK * 5];
    __shared__ unsigned long long s_key;
    __shared__ int s_models;
    const int b = blockIdx.y, tid = threadIdx.x, h = blockIdx.x * PNP_THREADS + tid;
    int first, last; bool bad;
    geo_range(offsets, b, M, &first, &last, &bad);
    const int n = last - first;
    if (n < 3) return;                                  // block-uniform
    if (tid == 0) { s_key = 0ull; s_models = 0; }
    const double* X = X_all + 3 * (size_t)first;
    const double* px = px_all + 2 * (size_t)first;
    double T[48];
    const int ns = pnp_solve_hypothesis(X, px, n, cam, seed, min(h, H - 1), T);     // the spare lanes solve the last hypothesis again
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    for (int base = 0; base < n; base += PNP_CHUNK) {
        const int m = min(PNP_CHUNK, n - base);
        __syncthreads();                                // the chunk before is consumed (and the first time: s_key is set)
        for (int i = tid; i < m; i += PNP_THREADS) {
            const double* p = X + 3 * (size_t)(base + i);
            const double* q = px + 2 * (size_t)(base + i);
            s_pt[5 * i] = p[0]; s_pt[5 * i + 1] = p[1]; s_pt[5 * i + 2] = p[2]; s_pt[5 * i + 3] = q[0]; s_pt[5 * i + 4] = q[1];
        }
        __syncthreads();
        for (int i = 0; i < m; i++) {                   // an unused slot is a zero pose: depth 0, never an inlier
            const double x = s_pt[5 * i], y = s_pt[5 * i + 1], z = s_pt[5 * i + 2], u = s_pt[5 * i + 3], v = s_pt[5 * i + 4];
            c0 += pnp_inlier(T, x, y, z, u, v, cam, thr2) ? 1 : 0;
            c1 += pnp_inlier(T + 12, x, y, z, u, v, cam, thr2) ? 1 : 0;
            c2 += pnp_inlier(T + 24, x, y, z, u, v, cam, thr2) ? 1 : 0;
            c3 += pnp_inlier(T + 36, x, y, z, u, v, cam, thr2) ? 1 : 0;
        }
    }
    unsigned long long best = 0ull;
    const int cnt[4] = {c0, c1, c2, c3};
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const unsigned long long k = r < ns ? geo_key3(cnt[r], h, r) : 0ull;
        best = k > best ? k : best;
    }
    if (h < H) {
        if (best) atomicMax(&s_key, best);
        if (ns) atomicAdd(&s_models, ns);
    }
    __syncthreads();
    if (tid == 0) {
        if (s_key) atomicMax(&keys[b], s_key);          // integer maxima and sums: the order of arrival does not matter
        if (s_models) atomicAdd(&models[b], s_models);
    }
}

// grid B: the winner of candidate b solved again (every lane the same hypothesis), its pose, mask and stats written
__global__ __launch_bounds__(PNP_LANES) void pnp_ransac_result_kernel(const int* __restrict__ offsets, int M, const double* __restrict__ X_all,
                                                                      const double* __restrict__ px_all, geo_cam cam, double thr2, uint64_t seed,
                                                                      const unsigned long long* __restrict__ keys,
                                                                      const int* __restrict__ models, double* __restrict__ pose_out,
                                                                      uint8_t* __restrict__ inlier, int* __restrict__ stats,
                                                                      unsigned int* __restrict__ index_errors) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int first, last; bool bad;
    geo_range(offsets, b, M, &first, &last, &bad);
    if (bad && lane == 0) atomicAdd(index_errors, 1u);
    const int n = last - first;
    const unsigned long long key = n >= 3 ? keys[b] : 0ull;
    if (!key) {
        if (lane < 12) pose_out[12 * b + lane] = (lane % 5 == 0) ? 1.0 : 0.0;
        for (int i = lane; i < n; i += PNP_LANES) inlier[first + i] = 0;
        if (lane == 0) { stats[4 * b] = 0; stats[4 * b + 1] = -1; stats[4 * b + 2] = -1; stats[4 * b + 3] = 0; }
        return;
    }
    // geo_key3 unpacked in place, not through geo_key_count / geo_key3_h / geo_key3_sub: with the accessors this kernel's
    // instruction stream changes (6658 -> 6626 instructions), every other result kernel's does not
    const int count = (int)(key >> 32), h = GEO_H_MAX - (int)((key >> 4) & 0xFFFFFFFull), sol = 15 - (int)(key & 15);
    const double* X = X_all + 3 * (size_t)first;
    const double* px = px_all + 2 * (size_t)first;
    double T4[48], T[12];
    pnp_solve_hypothesis(X, px, n, cam, seed, h, T4);
#pragma unroll
    for (int i = 0; i < 12; i++) T[i] = sol == 0 ? T4[i] : sol == 1 ? T4[12 + i] : sol == 2 ? T4[24 + i] : T4[36 + i];
    for (int i = lane; i < n; i += PNP_LANES)
        inlier[first + i] = pnp_inlier(T, X[3 * (size_t)i], X[3 * (size_t)i + 1], X[3 * (size_t)i + 2], px[2 * (size_t)i], px[2 * (size_t)i + 1],
                                       cam, thr2) ? 1 : 0;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 12; i++) pose_out[12 * b + i] = T[i];
        stats[4 * b] = count; stats[4 * b + 1] = h; stats[4 * b + 2] = sol; stats[4 * b + 3] = models[b];
    }
}

// =============================================================== entry points ================================================
#include "geometry_host.h"           // the checks, the vote block and the launch shapes the four estimators' entry points share

extern "C" int slam_pnp_p3p_f64(slam_ctx* ctx, int64_t S, const double* d_X, const double* d_x, double* d_pose, int32_t* d_nsol) {
    GEO_SAMPLE_SIZES(ctx, S);
    GEO_POINTERS(S, d_X && d_x && d_pose && d_nsol);
    SLAM_HIP(hipSetDevice(ctx->device));
    pnp_p3p_kernel<<<geo_blocks(S, PNP_LANES), PNP_LANES, 0, ctx->stream>>>((int)S, d_X, d_x, d_pose, d_nsol);
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

extern "C" int slam_pnp_ransac_f64(slam_ctx* ctx, int64_t B, const int32_t* d_offsets, const double* d_X, const double* d_px, int64_t M,
                                   double fx, double fy, double cx, double cy, int H, double threshold_px, uint64_t seed, double* d_pose,
                                   uint8_t* d_inlier, int32_t* d_stats) {
    GEO_RANSAC_SIZES(ctx, B, M, H);
    SLAM_REQUIRE(threshold_px > 0.0 && fx > 0.0 && fy > 0.0, "threshold and focal lengths must be positive");
    GEO_POINTERS(B, d_offsets && d_pose && d_stats && (M == 0 || (d_X && d_px && d_inlier)));
    SLAM_HIP(hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> lk(ctx->call_mu);        // the workspace holds the keys and the model counts
    void* ws = nullptr;
    if (int rc = slam_workspace(ctx, geo_vote_bytes(0, B), &ws)) return rc;
    unsigned long long* keys; int* models;
    if (int rc = geo_vote_block(ctx, ws, 0, B, true, M, d_inlier, &keys, &models)) return rc;
    const geo_cam cam = {fx, fy, cx, cy};
    const double thr2 = threshold_px * threshold_px;
    pnp_ransac_kernel<<<geo_vote_grid(H, PNP_THREADS, B), PNP_THREADS, 0, ctx->stream>>>(d_offsets, (int)M, d_X, d_px, cam, H, thr2, seed, keys,
                                                                                         models);
    SLAM_HIP(hipGetLastError());
    pnp_ransac_result_kernel<<<(unsigned)B, PNP_LANES, 0, ctx->stream>>>(d_offsets, (int)M, d_X, d_px, cam, thr2, seed, keys, models, d_pose,
                                                                       d_inlier, d_stats, slam_index_error_counter(ctx));
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}
#endif  // PNP_HOST_ONLY
