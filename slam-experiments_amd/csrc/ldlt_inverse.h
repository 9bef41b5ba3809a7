// ldlt_inverse.h — inverse of a small SPD block by LDL^T: the block-Jacobi preconditioner of graph_lm.h.  On its own, with no
// other include, because the host twin of the test suite compiles it with a plain C++ compiler through sim3_graph.hip.
#pragma once
#include <math.h>

#pragma clang fp contract(off)

#ifdef __HIPCC__
#define LDLT_HD __device__ __forceinline__
#else
#define LDLT_HD inline
#endif

// inverse of the SPD NxN A (full storage, row-major), as po_solve of pose_opt.hip; false (and the identity) if not SPD
template <int N>
LDLT_HD bool ldlt_inverse(const double* A, double* Inv) {
    double L[N * N], d[N], dinv[N];
    bool spd = true;
#pragma unroll
    for (int j = 0; j < N; j++) {
        double v = A[j * N + j];
#pragma unroll
        for (int k = 0; k < j; k++) v -= L[j * N + k] * L[j * N + k] * d[k];
        spd = spd && (v > 0.0) && isfinite(v);
        d[j] = v;
        dinv[j] = 1.0 / v;
#pragma unroll
        for (int i = j + 1; i < N; i++) {
            double u = A[i * N + j];
#pragma unroll
            for (int k = 0; k < j; k++) u -= L[i * N + k] * L[j * N + k] * d[k];
            L[i * N + j] = u * dinv[j];
        }
    }
#pragma unroll
    for (int c = 0; c < N; c++) {          // column c of the inverse; the lower triangle is mirrored from the upper one
        double y[N], x[N];
#pragma unroll
        for (int i = 0; i < N; i++) {
            double v = (i == c) ? 1.0 : 0.0;
#pragma unroll
            for (int k = 0; k < i; k++) v -= L[i * N + k] * y[k];
            y[i] = v;
        }
#pragma unroll
        for (int i = N - 1; i >= 0; i--) {
            double v = y[i] * dinv[i];
#pragma unroll
            for (int k = i + 1; k < N; k++) v -= L[k * N + i] * x[k];
            x[i] = v;
        }
#pragma unroll
        for (int i = 0; i < N; i++)
            if (i <= c) { Inv[i * N + c] = spd ? x[i] : (i == c ? 1.0 : 0.0); Inv[c * N + i] = Inv[i * N + c]; }
    }
    return spd;
}
