// ba_common.h — the device code that the dense (ba_schur.hip) and the sparse (ba_sparse.hip) bundle adjustment share: the
// one-observation linearisation, the fixed-order block sum, the damped 3x3 inverse of a point block and the pose update.
//
// This header carries NO floating-point contraction pragma, on purpose: the arithmetic of its functions takes the contraction
// state of the file that includes it, at the place where it is included.  The two files differ.  ba_schur.hip compiles with
// the compiler's default (a * b + c may become one fma): its one-launch kernel is the benchmarked one, and its results are
// held to a plain-C statement of the same loop within a tolerance.  ba_sparse.hip sets `#pragma clang fp contract(off)` BEFORE it includes this
// header: its blocks are held against the numpy statement within a bound that counts one rounding per operation.  Giving
// either file the other's state changes its bits, so neither is "fixed" to match.
//
// Not here, because they are different arithmetic by design: pose_opt.hip (explicit fma(), the translation summed separately
// in po_apply_update), reproj.hip (its own project), pose_graph.hip (an update with a series below 1e-4 rad).
#pragma once
#include <math.h>

#define BA_THREADS 256   // every workgroup of both files; ba_block_sum assumes its four waves

struct ba_cam { double fx, fy, cx, cy; };

// one observation linearised: residual e, robust weight w and cost rho, the 2x6 pose Jacobian (rotation first) and the 2x3
// point Jacobian, at pose P (3x4 row-major, any address space) and point p
struct ba_lin { double e0, e1, w, rho, jp[2][6], jq[2][3]; };

__device__ __forceinline__ void ba_linearise(const double* P, const double* p, const double2 m, const ba_cam& cam, const double delta,
                                             ba_lin& q) {
    const double X = P[0] * p[0] + P[1] * p[1] + P[2] * p[2] + P[3];
    const double Y = P[4] * p[0] + P[5] * p[1] + P[6] * p[2] + P[7];
    const double Z = P[8] * p[0] + P[9] * p[1] + P[10] * p[2] + P[11];
    q.e0 = m.x - (cam.fx * X + cam.cx * Z) / Z;      // frontend.py:275-277
    q.e1 = m.y - (cam.fy * Y + cam.cy * Z) / Z;
    const double Zinv = 1.0 / (Z + 1e-18), Zinv2 = Zinv * Zinv;  // frontend.py:284-291
    q.jp[0][0] = cam.fx * X * Y * Zinv2; q.jp[0][1] = -cam.fx - cam.fx * X * X * Zinv2; q.jp[0][2] = cam.fx * Y * Zinv;
    q.jp[0][3] = -cam.fx * Zinv; q.jp[0][4] = 0.0; q.jp[0][5] = cam.fx * X * Zinv2;
    q.jp[1][0] = cam.fy + cam.fy * Y * Y * Zinv2; q.jp[1][1] = -cam.fy * X * Y * Zinv2; q.jp[1][2] = -cam.fy * X * Zinv;
    q.jp[1][3] = 0.0; q.jp[1][4] = -cam.fy * Zinv; q.jp[1][5] = cam.fy * Y * Zinv2;
    const double A[2][3] = {{cam.fx * Zinv, 0.0, -cam.fx * X * Zinv2}, {0.0, cam.fy * Zinv, -cam.fy * Y * Zinv2}};
#pragma unroll
    for (int c = 0; c < 3; c++) {
        q.jq[0][c] = -(A[0][0] * P[c] + A[0][2] * P[8 + c]);
        q.jq[1][c] = -(A[1][1] * P[4 + c] + A[1][2] * P[8 + c]);
    }
    const double c2 = q.e0 * q.e0 + q.e1 * q.e1;
    q.w = 1.0; q.rho = c2;
    if (delta > 0.0) {
        const double en = sqrt(c2);
        if (en > delta) { q.w = delta / en; q.rho = 2.0 * delta * en - delta * delta; }
    }
}

__device__ __forceinline__ double ba_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// block-wide fixed-order sum of NT per-thread accumulators into out[NT] (shared): the xor tree inside a wave, the four waves
// in order; all threads return after it
template <int NT>
__device__ __forceinline__ void ba_block_sum(const double (&acc)[NT], double (*sw)[NT], double* out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NT; i++) {
        const double s = ba_wave_sum(acc[i]);
        if (lane == 0) sw[wave][i] = s;
    }
    __syncthreads();
    if (threadIdx.x < NT) out[threadIdx.x] = ((sw[0][threadIdx.x] + sw[1][threadIdx.x]) + sw[2][threadIdx.x]) + sw[3][threadIdx.x];
    __syncthreads();
}

// symmetric 3x3 inverse of H + lam I by cofactors, H as its packed upper triangle (the identity for a point nobody observes)
__device__ __forceinline__ void ba_damped_inverse(const double (&h)[6], const double lam, const bool seen, double (&e)[9]) {
    double m00 = h[0] + lam, m01 = h[1], m02 = h[2], m11 = h[3] + lam, m12 = h[4], m22 = h[5] + lam;
    if (!seen) { m00 = m11 = m22 = 1.0; m01 = m02 = m12 = 0.0; }
    const double c00 = m11 * m22 - m12 * m12, c01 = m02 * m12 - m01 * m22, c02 = m01 * m12 - m02 * m11;
    const double det = m00 * c00 + m01 * c01 + m02 * c02;
    const double id = 1.0 / det;
    e[0] = c00 * id; e[1] = c01 * id; e[2] = c02 * id;
    e[3] = e[1]; e[4] = (m00 * m22 - m02 * m02) * id; e[5] = (m01 * m02 - m00 * m12) * id;
    e[6] = e[2]; e[7] = e[5]; e[8] = (m00 * m11 - m01 * m01) * id;
}

// exp([w, v]) * T for a 3x4 row-major pose (rotation first): the update the Jacobian of frontend.py:288-291 is the derivative for
__device__ __forceinline__ void ba_apply_update(const double* dx, const double* T, double* Tn) {
    const double wx = dx[0], wy = dx[1], wz = dx[2];
    const double th2 = wx * wx + wy * wy + wz * wz, th = sqrt(th2);
    double a, b, c;  // sin(th)/th, (1-cos)/th^2, (th-sin)/th^3
    if (th < 1e-10) { a = 1.0; b = 0.5; c = 1.0 / 6.0; }
    else {
        double sn, cs;
        sincos(th, &sn, &cs);
        a = sn / th; b = (1.0 - cs) / th2; c = (th - sn) / (th2 * th);
    }
    const double W[9] = {0, -wz, wy, wz, 0, -wx, -wy, wx, 0};
    double W2[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) W2[i * 3 + j] = W[i * 3] * W[j] + W[i * 3 + 1] * W[3 + j] + W[i * 3 + 2] * W[6 + j];
    double R[9], V[9];
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const double I = (i % 4 == 0) ? 1.0 : 0.0;
        R[i] = I + a * W[i] + b * W2[i];
        V[i] = I + b * W[i] + c * W2[i];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 4; j++) Tn[i * 4 + j] = R[i * 3] * T[j] + R[i * 3 + 1] * T[4 + j] + R[i * 3 + 2] * T[8 + j];
        Tn[i * 4 + 3] += V[i * 3] * dx[3] + V[i * 3 + 1] * dx[4] + V[i * 3 + 2] * dx[5];
    }
}
