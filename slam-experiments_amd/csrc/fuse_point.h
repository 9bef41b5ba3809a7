// fuse_point.h - the per-point and per-candidate arithmetic of ORBmatcher::Fuse and of the refresh of a map point from its
// observations: the gates of proj_point.h with the distance-invariance margins, the reprojection gate of one
// candidate row, the median of one row of the observation distance table by counting, and the normal and distance range of
// MapPoint::UpdateNormalAndDepth.  The same text runs in fuse.hip and on the host (tests/fuse_twin.cpp builds it with a plain
// C++ compiler): integers and f64, contraction off, only + - * / sqrt, the operations in the order written.
#pragma once
#include "geometry_common.h"
#include "proj_point.h"

#define FP_OBS_MAX 256              // observations of one map point
#define FP_LEVELS_MAX PP_LEVELS_MAX

#pragma clang fp contract(off)

// ---- A: the search ------------------------------------------------------------------------------------------------------------
// statuses 1 - 4 of pp_gates with the range gate d2 < m_lo2 dmin2 || d2 > m_hi2 dmax2; the level is predicted from dmax2 itself
GEO_HD pp_result fp_gates(const pp_camera& c, const double* A, const double* Ow, double th, const double* X, const double* range,
                          const double* normal, const int32_t* level, double m_lo2, double m_hi2) {
    return pp_gates(c, A, Ow, th, X, range, normal, level, m_lo2, m_hi2);
}

// the reprojection gate of the frame row at pixel (xj, yj) for the projection (u, v): false iff e2 > lim with lim =
// chi2 * sigma2[level_j], formed once on the host.  A NaN rejects nothing.
GEO_HD bool fp_candidate(double u, double v, float xj, float yj, double lim) {
    const double ex = u - (double)xj, ey = v - (double)yj;
    const double e2 = ex * ex + ey * ey;
    return !(e2 > lim);
}

// ---- B: the refresh -----------------------------------------------------------------------------------------------------------
// The element of rank (n - 1) / 2 (0-based, ascending) of the n distances dist(0) .. dist(n - 1), each an integer in [0, 256]:
// the smallest value v with at least rank + 1 distances <= v.  Nine passes of counting; no order among equal elements exists.
template <class DIST>
GEO_HD int fp_median(int n, const DIST& dist) {
    const int need = (n - 1) / 2 + 1;
    int lo = 0, hi = 256;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        int c = 0;
        for (int k = 0; k < n; k++) c += dist(k) <= mid ? 1 : 0;
        if (c >= need) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// the word of observation i in the choice of the representative descriptor: the smallest (median, i) wins
GEO_HD uint32_t fp_choice_key(int median, int i) { return ((uint32_t)median << 8) | (uint32_t)i; }

// one observation's share of the normal: t[0..2] = (X - O) / |X - O|, t[3] = |X - O|
GEO_HD void fp_view(const double* X, const double* O, double* t) {
    const double p[3] = {X[0] - O[0], X[1] - O[1], X[2] - O[2]};
    const double len = sqrt(geo_dot(p, p));
    t[0] = p[0] / len;
    t[1] = p[1] / len;
    t[2] = p[2] / len;
    t[3] = len;
}

// s: the views' sum in list order (s = t_0, then s += t_k); dist, level: of the reference observation.  normal = unit(s),
// range = (dmin^2, dmax^2) with dmax = dist * scale[l], dmin = dmax / scale[n_levels - 1]; all NaN unless the normal is finite.
GEO_HD void fp_normal_range(const double* s, double dist, int level, const double* scale, int n_levels, double* normal, double* range) {
    const double nan = __builtin_nan("");
    double nr[3] = {s[0], s[1], s[2]};
    geo_unit(nr);
    const int l = level < 0 ? 0 : (level > n_levels - 1 ? n_levels - 1 : level);
    const double dmax = dist * scale[l], dmin = dmax / scale[n_levels - 1];
    const bool ok = nr[0] - nr[0] == 0.0 && nr[1] - nr[1] == 0.0 && nr[2] - nr[2] == 0.0;
    normal[0] = ok ? nr[0] : nan;
    normal[1] = ok ? nr[1] : nan;
    normal[2] = ok ? nr[2] : nan;
    range[0] = ok ? dmin * dmin : nan;
    range[1] = ok ? dmax * dmax : nan;
}
