// pose_lm.h - the model-independent parts of the one-launch pose refinements: the pose update, the damped 6x6 solve and the
// fixed-order block sums of pose_opt.hip (two residuals per edge, unit information) and pose_stereo.hip (the stereo / weighted
// edges of stereo_edge.h).  The text is pose_opt.hip's, moved; it carries no contraction pragma and both files include it
// under the compiler's default, before any pragma of their own.  The Levenberg-Marquardt round they both run is
// pose_lm_round.inc, which takes the contraction state of each file instead.
#pragma once
#include <math.h>


#define PO_THREADS 256
#define PO_TERMS 28   // 21 (upper H) + 6 (b) + 1 (robust chi2 of the active edges)
#define PO_RED_STRIDE (PO_THREADS / 2 + 8)   // doubles per term in the reduction buffer: padded, so the 16-value reads of
                                             // thread (term, segment) fall on different LDS banks for different terms

// exp([w, v]) * T for a 3x4 row-major pose (rotation first, g2o SE3Quat::exp ordering)
__device__ __forceinline__ void po_apply_update(const double* dx, const double* T, double* Tn) {
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
    double t[3];
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = V[i * 3] * dx[3] + V[i * 3 + 1] * dx[4] + V[i * 3 + 2] * dx[5];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 4; j++)
            Tn[i * 4 + j] = R[i * 3] * T[j] + R[i * 3 + 1] * T[4 + j] + R[i * 3 + 2] * T[8 + j];
        Tn[i * 4 + 3] += t[i];
    }
}

// solve (H + lam I) x = -b by LDL^T (six reciprocals, no square roots: this runs on one lane, so the length of
// the dependent f64 chain is what it costs); H given as packed upper triangle s[0..20]; false if not SPD
__device__ __forceinline__ bool po_solve(const double* s, const double* b, double lam, double* x) {
    double A[36];
    int t = 0;
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = i; j < 6; j++) { A[i * 6 + j] = A[j * 6 + i] = s[t++]; }
#pragma unroll
    for (int i = 0; i < 6; i++) A[i * 6 + i] += lam;
    double L[36], d[6], dinv[6];
    bool spd = true;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double v = A[j * 6 + j];
#pragma unroll
        for (int k = 0; k < j; k++) v -= L[j * 6 + k] * L[j * 6 + k] * d[k];
        spd = spd && (v > 0.0) && isfinite(v);
        d[j] = v;
        dinv[j] = 1.0 / v;
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double u = A[i * 6 + j];
#pragma unroll
            for (int k = 0; k < j; k++) u -= L[i * 6 + k] * L[j * 6 + k] * d[k];
            L[i * 6 + j] = u * dinv[j];
        }
    }
    if (!spd) return false;
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double v = -b[i];
#pragma unroll
        for (int k = 0; k < i; k++) v -= L[i * 6 + k] * y[k];
        y[i] = v;
    }
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        double v = y[i] * dinv[i];
#pragma unroll
        for (int k = i + 1; k < 6; k++) v -= L[k * 6 + i] * x[k];
        x[i] = v;
    }
    return true;
}

// sum over the block of `nterms` per-thread values each (acc[0..nterms)), run-to-run identical: adjacent lanes are paired
// by a DPP swap, the even lane of each pair parks the pair's sum in LDS (128 values per term), thread (term, segment) adds
// its 16 values in a rotated but fixed order (bank-conflict free through the padded term stride; the rotation depends on the segment only, so a term
// rounds the same whatever its index), then one thread per term adds the 8 partials.  Three barriers; every thread returns
// with the sums in out[0..nterms).
__device__ __forceinline__ double po_swap_adjacent(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)b, 0xB1, 0xF, 0xF, true);          // quad_perm [1,0,3,2]
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), 0xB1, 0xF, 0xF, true);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
template <int NT>
__device__ __forceinline__ void po_block_sums(double (&acc)[NT], double* red, double* part, double* out) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < NT; i++) acc[i] += po_swap_adjacent(acc[i]);
    if (!(tid & 1)) {
#pragma unroll
        for (int i = 0; i < NT; i++) red[i * PO_RED_STRIDE + (tid >> 1)] = acc[i];
    }
    __syncthreads();
    if (tid < NT * 8) {
        const double* r = red + (tid >> 3) * PO_RED_STRIDE + (tid & 7) * 16;
        double sum = 0.0;
#pragma unroll
        for (int k = 0; k < 16; k++) sum += r[(k + (tid & 7)) & 15];
        part[tid] = sum;
    }
    __syncthreads();
    if (tid < NT) {
        const double* q = part + tid * 8;
        out[tid] = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
    }
    __syncthreads();
}
