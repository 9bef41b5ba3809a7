// geometry_common.h — the one copy of what the four batched RANSAC estimators (two_view.hip, pnp.hip, homography.hip, sim3.hip)
// share: the counter-based sampler, cyclic Jacobi, DLT triangulation and the cheirality test, a candidate's clamped slice
// of the offsets, the intrinsics, the key of a scored model, and three-vector helpers.
//
// Contraction is OFF here as in every includer, and only + - * / sqrt are used: a result is a pure function of its inputs
// whatever it is inlined into, on the device and in the host twins alike.  The twins (two_view_twin.cpp, pnp_twin.cpp,
// hg_twin.cpp, sim3_twin.cpp of the test suite) include a kernel file under plain g++ with __host__, __device__ and
// __forceinline__ defined away and no HIP header, so nothing here may need internal.h, and the one routine that needs a
// device function (geo_range) is for hipcc alone.
#pragma once
#include <math.h>
#include <stdint.h>

#pragma clang fp contract(off)

#define GEO_HD __host__ __device__ __forceinline__
#define GEO_H_MAX (1 << 20)          // hypotheses per candidate, the width of a key's hypothesis field
#define GEO_BIG 1e200                // data whose squares sum to this or more (or to NaN) has no model
#define GEO_FLAT 1e-20               // sin^2 of the smallest angle of a triangle / between two bearings that is still solved

struct geo_cam { double fx, fy, cx, cy; };

// ---- three-vectors (pnp, homography, sim3 and two_view had these operation for operation) ----------------------------------
GEO_HD double geo_dot(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
GEO_HD void geo_cross(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
GEO_HD void geo_unit(double* a) {
    const double inv = 1.0 / sqrt(geo_dot(a, a));
    a[0] *= inv; a[1] *= inv; a[2] *= inv;
}

// ---- sampling (stated in include/slamhip.h at slam_tv_essential_ransac_f64) ---------------------------------------------------
GEO_HD uint64_t geo_splitmix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
GEO_HD uint64_t geo_draw_word(uint64_t seed, uint64_t h, uint64_t d) {
    return geo_splitmix(geo_splitmix(seed ^ (h * 0xD1B54A32D192ED03ull)) ^ (d * 0x8CB92BA72F3D8DD7ull));
}
// the K distinct indices of hypothesis h among n >= K
template <int K>
GEO_HD void geo_draw_sample(uint64_t seed, int h, int n, int* idx) {
    uint64_t d = 0;
#pragma unroll
    for (int k = 0; k < K; k++) {
        int i;
        bool dup;
        do {
            i = (int)(((geo_draw_word(seed, (uint64_t)h, d++) >> 32) * (uint64_t)n) >> 32);
            dup = false;
#pragma unroll
            for (int j = 0; j < K; j++) dup = dup || (j < k && idx[j] == i);
        } while (dup);
        idx[k] = i;
    }
}

#ifdef __HIPCC__                     // the kernels' alone (device min / max): a host twin takes one candidate and no offsets
// candidate b's slice of the concatenated arrays, never outside [0, M)
__device__ __forceinline__ void geo_range(const int* offsets, int b, int M, int* first, int* last, bool* bad) {
    const int lo = offsets[b], hi = offsets[b + 1];
    *first = min(max(lo, 0), M);
    *last = min(max(hi, *first), M);
    *bad = *first != lo || *last != hi;
}
#endif

// ---- the key of a scored model: more inliers first, then the lower hypothesis (then the lower root / solution); 0 = no model --
GEO_HD unsigned long long geo_key3(int count, int h, int sub) {
    return ((unsigned long long)(unsigned)count << 32) | ((unsigned long long)(GEO_H_MAX - h) << 4) | (unsigned long long)(15 - sub);
}
GEO_HD int geo_key_count(unsigned long long key) { return (int)(key >> 32); }      // of either layout
GEO_HD int geo_key3_h(unsigned long long key) { return GEO_H_MAX - (int)((key >> 4) & 0xFFFFFFFull); }
GEO_HD int geo_key3_sub(unsigned long long key) { return 15 - (int)(key & 15); }
GEO_HD unsigned long long geo_key2(int count, int h) {
    return ((unsigned long long)(unsigned)count << 32) | (unsigned long long)(GEO_H_MAX - h);
}
GEO_HD int geo_key2_h(unsigned long long key) { return GEO_H_MAX - (int)(key & 0xFFFFFFFFull); }

// ---- small symmetric eigenproblems (cyclic Jacobi, fixed sweep count: deterministic) ------------------------------------------
// A symmetric, overwritten by its diagonal form; V its eigenvectors by columns
template <int N, int SWEEPS>
GEO_HD void geo_jacobi(double (&A)[N][N], double (&V)[N][N]) {
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = 0; j < N; j++) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < SWEEPS; sweep++) {
#pragma unroll
        for (int p = 0; p < N - 1; p++)
#pragma unroll
            for (int q = p + 1; q < N; q++) {
                const double apq = A[p][q];
                if (apq == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                A[p][p] -= t * apq;
                A[q][q] += t * apq;
                A[p][q] = A[q][p] = 0.0;
#pragma unroll
                for (int k = 0; k < N; k++) {
                    if (k != p && k != q) {
                        const double akp = A[k][p], akq = A[k][q];
                        A[k][p] = A[p][k] = c * akp - s * akq;
                        A[k][q] = A[q][k] = s * akp + c * akq;
                    }
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    }
}

// DLT triangulation of one point (cv2.triangulatePoints): v = unit eigenvector of the smallest eigenvalue of A^T A, v[3] >= 0
GEO_HD void geo_triangulate_point(const double* P1, const double* P2, double a, double b, double c, double d, double* v) {
    double A[4][4], S[4][4], V[4][4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        A[0][j] = a * P1[8 + j] - P1[j];
        A[1][j] = b * P1[8 + j] - P1[4 + j];
        A[2][j] = c * P2[8 + j] - P2[j];
        A[3][j] = d * P2[8 + j] - P2[4 + j];
    }
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = i; j < 4; j++) S[i][j] = S[j][i] = ((A[0][i] * A[0][j] + A[1][i] * A[1][j]) + A[2][i] * A[2][j]) + A[3][i] * A[3][j];
    geo_jacobi<4, 10>(S, V);
    double best = S[0][0];
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = V[k][0];
#pragma unroll
    for (int j = 1; j < 4; j++)
        if (S[j][j] < best) {
            best = S[j][j];
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = V[k][j];
        }
    const double inv = 1.0 / sqrt(((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + v[3] * v[3]);
    const double sg = v[3] < 0.0 ? -inv : inv;
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] *= sg;
}

// good under the pose T [12] = [R | t]: depth in (0, dist) in both cameras (cv2.recoverPose)
GEO_HD bool geo_cheirality(const double* T, double a, double b, double c, double d, double dist) {
    const double P1[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    double v[4];
    geo_triangulate_point(P1, T, a, b, c, d, v);
    const double X = v[0] / v[3], Y = v[1] / v[3], Z = v[2] / v[3];
    const double Z2 = ((T[8] * X + T[9] * Y) + T[10] * Z) + T[11];
    return Z > 0.0 && Z < dist && Z2 > 0.0 && Z2 < dist;
}
