// proj_point.h - the per-point gates of SearchByProjection: camera coordinates, pixel, range, view angle
// and the predicted pyramid level of one map point under one pose.  The same text runs in pm_scan_kernel and on the host
// (tests/proj_match_twin.cpp builds it with a plain C++ compiler): f64, contraction off, the operations in the order written.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define PP_HD __host__ __device__ __forceinline__
#else
#define PP_HD inline
#endif

#define PP_LEVELS_MAX 16

struct pp_camera {
    double fx, fy, cx, cy;
    double min_x, max_x, min_y, max_y;
    double cos2_limit;
    double scale[PP_LEVELS_MAX], scale2[PP_LEVELS_MAX];
    int n_levels;
    int pad;
};

// status: 0 = searched, 1 = not in front of the camera, 2 = outside the bounds, 3 = outside the scale-invariance range,
// 4 = seen from too far off its normal.  What a failed gate never computed stays NaN (u, v) or -1 (lp).
struct pp_result {
    double u, v, r;
    int status, lp;
};

#pragma clang fp contract(off)
// A: world -> camera, 3x4 row-major; Ow: the camera centre; X: the point; range: {dmin2, dmax2} or null; normal: the unit
// viewing normal or null; level: the level the point was last seen at, or null (read only when range is null).  m_lo2, m_hi2:
// the margins of the range gate (Fuse: 0.8^2 and 1.2^2, fuse_point.h); times 1.0 is exact, and the level is predicted from the
// range as it stands.
PP_HD pp_result pp_gates(const pp_camera& c, const double* A, const double* Ow, double th, const double* X, const double* range,
                         const double* normal, const int32_t* level, double m_lo2 = 1.0, double m_hi2 = 1.0) {
    pp_result o;
    o.u = o.v = o.r = __builtin_nan("");
    o.lp = -1;
    const double xc = ((A[0] * X[0] + A[1] * X[1]) + A[2] * X[2]) + A[3];
    const double yc = ((A[4] * X[0] + A[5] * X[1]) + A[6] * X[2]) + A[7];
    const double zc = ((A[8] * X[0] + A[9] * X[1]) + A[10] * X[2]) + A[11];
    o.status = 1;
    if (!(zc > 0.0)) return o;
    const double iz = 1.0 / zc;
    const double u = c.fx * (xc * iz) + c.cx, v = c.fy * (yc * iz) + c.cy;
    o.u = u;
    o.v = v;
    o.status = 2;
    if (!(c.min_x <= u && u < c.max_x && c.min_y <= v && v < c.max_y)) return o;
    double d2 = 0.0;
    if (range) {
        d2 = (xc * xc + yc * yc) + zc * zc;
        o.status = 3;
        if (d2 < m_lo2 * range[0] || d2 > m_hi2 * range[1]) return o;
    }
    if (normal) {
        const double p0 = X[0] - Ow[0], p1 = X[1] - Ow[1], p2 = X[2] - Ow[2];
        const double dot = (p0 * normal[0] + p1 * normal[1]) + p2 * normal[2];
        const double po2n = (p0 * p0 + p1 * p1) + p2 * p2;
        o.status = 4;
        if (!(dot > 0.0) || dot * dot < c.cos2_limit * po2n) return o;
    }
    int lp = 0;
    if (range) {
        for (int l = 0; l + 1 < c.n_levels; l++) lp += c.scale2[l] * d2 < range[1] ? 1 : 0;
    } else if (level) {
        lp = *level < 0 ? 0 : (*level > c.n_levels - 1 ? c.n_levels - 1 : *level);
    }
    o.status = 0;
    o.lp = lp;
    o.r = th * c.scale[lp];
    return o;
}
