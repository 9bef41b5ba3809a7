// stereo_point.h - the per-row arithmetic of stereo matching (ORB-SLAM's Frame::ComputeStereoMatches): the level-0
// pixel of a keypoint, the row band and the candidate gates, the centre of the SAD slide, the SAD itself over a patch pointer
// and a pitch, the running best of the slide, the parabola and the disparity.  The same text runs in the kernels of stereo.hip
// and on the host (tests/stereo_twin.cpp builds it with a plain C++ compiler): integers, one f32 product, and f64 with
// contraction off in the order written; floor, ceil and the division are exact or correctly rounded on both builds, so both give
// the same bits.
#pragma once
#pragma clang fp contract(off)
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <math.h>

#ifdef __HIPCC__
#define ST_HD __host__ __device__ __forceinline__
#else
#define ST_HD inline
#endif

#define ST_MATCHED 0
#define ST_NO_CANDIDATE 1
#define ST_ORB_DISTANCE 2
#define ST_WINDOW 3
#define ST_SLIDE_BORDER 4
#define ST_DISPARITY 5
#define ST_MEDIAN 6
#define ST_PENDING 255          // between the search and the SAD launch only: never in a result
#define ST_NO_DIST 256          // orb_dist of a row without a candidate
#define ST_HALF_MAX 15          // largest w and Ls (SLAM_STEREO_HALF_MAX)

// the one NaN every party writes: the bits of numpy's nan
ST_HD double st_nan() {
    const uint64_t b = 0x7ff8000000000000ull;
    double d;
    memcpy(&d, &b, 8);
    return d;
}

// level-0 pixel of a level coordinate: the single f32 product of OrbResult.xy, promoted
ST_HD double st_level0(int x, float scale) {
    const float p = (float)x * scale;
    return (double)p;
}

// the row band of a right row: every trunc(vL) in [lo, hi] = [floor(vR - r), ceil(vR + r)], r = 2 scale[lR], may hold its match
ST_HD void st_band(double vR, float scale_r, int* lo, int* hi) {
    const double r = 2.0 * (double)scale_r;
    *lo = (int)floor(vR - r);
    *hi = (int)ceil(vR + r);
}

// step 1: is the right row (band, level, uR) a candidate of the left row (tv = trunc(vL), lL, [min_u, max_u])
ST_HD bool st_candidate(int tv, int lL, double min_u, double max_u, int lo, int hi, int lR, double uR) {
    return lo <= tv && tv <= hi && lR >= lL - 1 && lR <= lL + 1 && uR >= min_u && uR <= max_u;
}

// step 3: the centre of the slide on level lL
ST_HD int st_c0(double uR, float scale_l) { return (int)floor(uR / (double)scale_l + 0.5); }

// ORB-SLAM's column test, and the left patch and the rows y +- w inside the level
ST_HD bool st_window_ok(int x, int y, int c0, int w, int Ls, int level_w, int level_h) {
    return c0 - Ls - w >= 0 && c0 + Ls + w + 1 < level_w && x - w >= 0 && x + w < level_w && y - w >= 0 && y + w < level_h;
}

// The pixels q = first, first + step, ... of the (2w+1)^2 window (row-major) of sum |(L(dy,dx) - L(0,0)) - (R(dy,dx) - R(0,0))|;
// pl and pr point at the two centres.  (first, step) = (0, 1) is the whole SAD; the kernel gives each lane (lane, 64) and adds.
ST_HD int st_sad(const uint8_t* pl, ptrdiff_t pitch_l, const uint8_t* pr, ptrdiff_t pitch_r, int w, int first, int step) {
    const int side = 2 * w + 1, n = side * side;
    const int cl = (int)pl[0], cr = (int)pr[0];
    int s = 0;
    for (int q = first; q < n; q += step) {
        const int dy = q / side - w, dx = q % side - w;
        const int d = ((int)pl[dy * pitch_l + dx] - cl) - ((int)pr[dy * pitch_r + dx] - cr);
        s += d < 0 ? -d : d;
    }
    return s;
}

// the slide: SADs pushed in ascending inc; keeps the smallest (SAD, inc) and its two neighbours (d1 is not meaningful when the
// best is the first inc pushed, d3 when it is the last: those are the slide border)
struct st_slide {
    int best, inc, d1, d3, prev, wait;
};

ST_HD st_slide st_slide_start() {
    st_slide s;
    s.best = INT32_MAX;
    s.inc = s.d1 = s.d3 = s.prev = s.wait = 0;
    return s;
}

ST_HD void st_slide_push(st_slide* s, int inc, int sad) {
    if (s->wait) {
        s->d3 = sad;
        s->wait = 0;
    }
    if (sad < s->best) {
        s->best = sad;
        s->inc = inc;
        s->d1 = s->prev;
        s->wait = 1;
    }
    s->prev = sad;
}

// step 4: d2 is the minimum, so den >= 0 and |delta| <= 1/2
ST_HD double st_parabola(int d1, int d2, int d3) {
    const int den = d1 + d3 - 2 * d2;
    if (den == 0) return 0.0;
    return (double)(d1 - d3) / (double)(2 * den);
}

struct st_depth {
    double u_right, depth;
    int status;                 // ST_MATCHED or ST_DISPARITY
};

// step 5
ST_HD st_depth st_disparity(double uL, float scale_l, int c0, int inc, double delta, double bf, double min_d, double max_d) {
    st_depth o;
    double u_right = (double)scale_l * ((double)(c0 + inc) + delta);
    double disp = uL - u_right;
    if (!(disp >= min_d && disp < max_d)) {
        o.u_right = o.depth = st_nan();
        o.status = ST_DISPARITY;
        return o;
    }
    if (disp <= 0.0) {
        disp = 0.01;
        u_right = uL - 0.01;
    }
    o.u_right = u_right;
    o.depth = bf / disp;
    o.status = ST_MATCHED;
    return o;
}

// step 6: kept when 10 SAD < 21 m
ST_HD bool st_median_keeps(int sad, int m) { return 10 * sad < 21 * m; }
