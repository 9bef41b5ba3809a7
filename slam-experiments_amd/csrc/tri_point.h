// tri_point.h - the per-candidate gates of SearchForTriangulation and the per-match geometry of CreateNewMapPoints (DESIGN.md
// 4m): the epipolar line of a side-1 pixel, the epipole and line gates of a side-2 pixel, and parallax, DLT, depths,
// reprojection and scale consistency of one match with the new point's normal and distance range.  The same text runs in
// tri_match.hip and on the host (tests/tri_match_twin.cpp builds it with a plain C++ compiler): f64, contraction off, only
// + - * / sqrt, the operations in the order written.
#pragma once
#include "geometry_common.h"

#define TP_LEVELS_MAX 16

#pragma clang fp contract(off)

// ---- A: the gates of one candidate -------------------------------------------------------------------------------------------
struct tp_line {
    double a, b, c;
};

// the line F12^T x1 of the side-1 pixel (x1, y1) in image 2; F row-major [9]
GEO_HD tp_line tp_epiline(const double* F, double x1, double y1) {
    tp_line l;
    l.a = (x1 * F[0] + y1 * F[3]) + F[6];
    l.b = (x1 * F[1] + y1 * F[4]) + F[7];
    l.c = (x1 * F[2] + y1 * F[5]) + F[8];
    return l;
}

// false iff the side-2 pixel lies closer to the epipole (ex, ey) than sqrt(lim) (lim = epipole_r2 * scale[level]); a NaN
// epipole rejects nothing
GEO_HD bool tp_off_epipole(double ex, double ey, double x2, double y2, double lim) {
    const double dx = ex - x2, dy = ey - y2;
    return !((dx * dx + dy * dy) < lim);
}

// CheckDistEpipolarLine without the division: strict, and false for a degenerate line or a NaN (lim = chi2 * sigma2[level])
GEO_HD bool tp_on_line(const tp_line& l, double x2, double y2, double lim) {
    const double num = (l.a * x2 + l.b * y2) + l.c, den = l.a * l.a + l.b * l.b;
    return den > 0.0 && num * num < lim * den;
}

// ---- B: the geometry of one match --------------------------------------------------------------------------------------------
struct tp_params {
    double fx, fy, cx, cy;
    double cos_max, chi2_px, ratio_factor;
    double line_lim[TP_LEVELS_MAX], epi_lim[TP_LEVELS_MAX];     // chi2 * sigma2[l] and epipole_r2 * scale[l], made on the host
    double scale[TP_LEVELS_MAX], sigma2[TP_LEVELS_MAX];
    int n_levels, th_low;
};

// status: 0 = created, 2 = parallax, 3 = at infinity, 4 / 5 = not in front of camera 1 / 2, 6 / 7 = reprojection error in image
// 1 / 2, 8 = scale inconsistent (1 = no match is the caller's).  X, normal and range are NaN wherever status != 0.
struct tp_point {
    double X[3], normal[3], range[2];
    int status;
};

GEO_HD int tp_level(int l, int n_levels) { return l < 0 ? 0 : (l > n_levels - 1 ? n_levels - 1 : l); }

// squared reprojection error of X under T (world -> camera, 3x4 row-major) against the pixel (x, y); *z receives the depth
GEO_HD double tp_reproject(const tp_params& c, const double* A, const double* X, double x, double y, double* z) {
    const double xc = ((A[0] * X[0] + A[1] * X[1]) + A[2] * X[2]) + A[3];
    const double yc = ((A[4] * X[0] + A[5] * X[1]) + A[6] * X[2]) + A[7];
    const double zc = ((A[8] * X[0] + A[9] * X[1]) + A[10] * X[2]) + A[11];
    *z = zc;
    const double iz = 1.0 / zc;
    const double u = c.fx * (xc * iz) + c.cx, v = c.fy * (yc * iz) + c.cy;
    const double du = u - x, dv = v - y;
    return du * du + dv * dv;
}

// T1, T2: world -> camera [12]; O1, O2: the camera centres; (x1, y1) / (x2, y2): level-0 pixels; l1, l2: pyramid levels
GEO_HD tp_point tp_triangulate(const tp_params& c, const double* T1, const double* T2, const double* O1, const double* O2, double x1,
                               double y1, double x2, double y2, int l1, int l2) {
    tp_point o;
    const double nan = __builtin_nan("");
    o.X[0] = o.X[1] = o.X[2] = o.normal[0] = o.normal[1] = o.normal[2] = o.range[0] = o.range[1] = nan;
    l1 = tp_level(l1, c.n_levels);
    l2 = tp_level(l2, c.n_levels);
    const double a1 = (x1 - c.cx) / c.fx, b1 = (y1 - c.cy) / c.fy, a2 = (x2 - c.cx) / c.fx, b2 = (y2 - c.cy) / c.fy;
    double r1[3], r2[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {                       // R^T xn with xn = (a, b, 1)
        r1[k] = (T1[k] * a1 + T1[4 + k] * b1) + T1[8 + k];
        r2[k] = (T2[k] * a2 + T2[4 + k] * b2) + T2[8 + k];
    }
    const double dot = geo_dot(r1, r2), n1 = geo_dot(r1, r1), n2 = geo_dot(r2, r2);
    o.status = 2;
    if (!(dot > 0.0 && dot * dot < (c.cos_max * c.cos_max) * (n1 * n2))) return o;
    double v[4];
    geo_triangulate_point(T1, T2, a1, b1, a2, b2, v);
    o.status = 3;
    if (!(v[3] > 0.0)) return o;
    const double X[3] = {v[0] / v[3], v[1] / v[3], v[2] / v[3]};
    if (!(X[0] - X[0] == 0.0 && X[1] - X[1] == 0.0 && X[2] - X[2] == 0.0)) return o;
    double z1, z2;
    const double e1 = tp_reproject(c, T1, X, x1, y1, &z1), e2 = tp_reproject(c, T2, X, x2, y2, &z2);
    o.status = 4;
    if (!(z1 > 0.0)) return o;
    o.status = 5;
    if (!(z2 > 0.0)) return o;
    o.status = 6;
    if (e1 > c.chi2_px * c.sigma2[l1]) return o;
    o.status = 7;
    if (e2 > c.chi2_px * c.sigma2[l2]) return o;
    const double p1[3] = {X[0] - O1[0], X[1] - O1[1], X[2] - O1[2]}, p2[3] = {X[0] - O2[0], X[1] - O2[1], X[2] - O2[2]};
    const double dist1 = sqrt(geo_dot(p1, p1)), dist2 = sqrt(geo_dot(p2, p2));
    o.status = 8;
    if (dist1 == 0.0 || dist2 == 0.0) return o;
    const double ratio_dist = dist2 / dist1, ratio_octave = c.scale[l1] / c.scale[l2];
    if (ratio_dist * c.ratio_factor < ratio_octave || ratio_dist > ratio_octave * c.ratio_factor) return o;
    double nr[3] = {p1[0] / dist1 + p2[0] / dist2, p1[1] / dist1 + p2[1] / dist2, p1[2] / dist1 + p2[2] / dist2};
    geo_unit(nr);
    const double dmax = dist1 * c.scale[l1], dmin = dmax / c.scale[c.n_levels - 1];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        o.X[k] = X[k];
        o.normal[k] = nr[k];
    }
    o.range[0] = dmin * dmin;
    o.range[1] = dmax * dmax;
    o.status = 0;
    return o;
}
