// proj_search.h - what the searches by projection share outside their scan kernels (proj_match.hip: SearchByProjection,
// fuse.hip: Fuse): the limits, the pair record, the parameters, the frames and points as the kernels take
// them, the cell of a coordinate, and the argument checks of the entry points.  One copy: both files include it.
#pragma once
#include "match_finish.h"
#include "proj_point.h"

#define PM_ROWS_MAX MF_ROWS_MAX
#define PM_PAIRS_MAX MF_PAIRS_MAX
#define PM_SCAN_LANES 64            // points of one scan workgroup: one wave
#define PM_ROW_THREADS 256          // threads of the per-row kernels of the grid step
#define PM_CELLS_MAX (1ll << 30)    // cells of one grid

struct pm_pair {
    mf_pair m;
    double A[12], Ow[3], th;
};

static_assert(sizeof(pm_pair) == 176, "the pair table is laid out by the host");

struct pm_params {
    pp_camera cam;
    double ratio;
    int th_high, level_rule, lo, hi;
};

struct pm_frames {
    const uint4* desc;              // descriptors in grid order
    const int* cells;               // cell ids in grid order
    const int* order;               // the row (local to its image) at each grid position
    const float2* xy;               // pixels in grid order
    const int* meta;                // level in grid order, -1 for a taken row
    const int* level;               // levels in row order
    const uint8_t* bins;            // orientation bins in row order, or null
    int gw, gh;
    double cell;
};

struct pm_points {
    const double* xyz;
    const uint4* desc;
    const double* range;            // (dmin2, dmax2) per point, or null
    const double* normal;           // or null
    const int* level;               // or null
    const uint8_t* bins;            // or null
};

// the grid column (or row) of a coordinate: monotone in x, clamped into the grid, 0 for a NaN
__device__ __forceinline__ int pm_cell_of(double x, double cell, int g) { return (int)fmin(fmax(floor(x / cell), 0.0), (double)(g - 1)); }

// ------------------------------------------------------------------------------------------------- argument checks (host)
static int pm_check_grid(int W, int H, int cell, const char* who, int* gw, int* gh) {
    SLAM_REQUIRE(W > 0 && H > 0, "%s: the image is %d x %d", who, W, H);
    SLAM_REQUIRE(cell > 0, "%s: cell=%d is not positive", who, cell);
    *gw = (W + cell - 1) / cell;
    *gh = (H + cell - 1) / cell;
    SLAM_REQUIRE((int64_t)*gw * *gh <= PM_CELLS_MAX, "%s: %d x %d cells are more than 2^30", who, *gw, *gh);
    return SLAM_OK;
}

static int pm_check_params(const slam_proj_params* p, const char* who, bool search, pm_params* out) {
    SLAM_REQUIRE(p, "%s: null parameters", who);
    SLAM_REQUIRE(p->n_levels >= 1 && p->n_levels <= PP_LEVELS_MAX, "%s: n_levels=%d outside [1, %d]", who, p->n_levels, PP_LEVELS_MAX);
    SLAM_REQUIRE(p->h_scale && p->h_scale2, "%s: null scale tables", who);
    SLAM_REQUIRE(!search || p->lo <= p->hi, "%s: the level offsets (%d, %d) descend", who, p->lo, p->hi);
    SLAM_REQUIRE(!search || p->ratio == p->ratio, "%s: ratio is not a number", who);
    memset(out, 0, sizeof(*out));
    pp_camera& c = out->cam;
    c.fx = p->fx, c.fy = p->fy, c.cx = p->cx, c.cy = p->cy;
    c.min_x = p->min_x, c.max_x = p->max_x, c.min_y = p->min_y, c.max_y = p->max_y;
    c.cos2_limit = p->cos2_limit;
    c.n_levels = p->n_levels;
    for (int l = 0; l < PP_LEVELS_MAX; l++) {
        c.scale[l] = l < p->n_levels ? p->h_scale[l] : 0.0;
        c.scale2[l] = l < p->n_levels ? p->h_scale2[l] : 0.0;
    }
    out->ratio = p->ratio;
    out->th_high = p->th_high;
    out->level_rule = p->level_rule;
    out->lo = p->lo;
    out->hi = p->hi;
    return SLAM_OK;
}

static int pm_check_points(const slam_proj_points* s, const char* who, pm_points* out) {
    SLAM_REQUIRE(s, "%s: null point sets", who);
    if (int rc = mf_check_offsets(s->h_offsets, s->B, who, "point set")) return rc;
    SLAM_REQUIRE(s->h_offsets[s->B] == 0 || s->d_xyz, "%s: null positions", who);
    SLAM_REQUIRE(((uintptr_t)s->d_desc & 15) == 0, "%s: descriptor pointers must be 16-byte aligned", who);
    out->xyz = s->d_xyz;
    out->desc = (const uint4*)s->d_desc;
    out->range = s->d_range;
    out->normal = s->d_normal;
    out->level = s->d_level;
    out->bins = s->d_bins;
    return SLAM_OK;
}

// a frame set of a search (points: the point sets searched in it, for their descriptors)
static int pm_check_frames(const slam_proj_frames* frames, const slam_proj_points* pts, const char* who, pm_frames* s2) {
    if (int rc = mf_check_offsets(frames->h_offsets, frames->B, who, "frame")) return rc;
    if (int rc = pm_check_grid(frames->W, frames->H, frames->cell, who, &s2->gw, &s2->gh)) return rc;
    SLAM_REQUIRE(frames->h_offsets[frames->B] == 0 ||
                     (frames->d_desc && frames->d_cells && frames->d_order && frames->d_xy && frames->d_meta && frames->d_level),
                 "%s: null device pointer in a frame set", who);
    SLAM_REQUIRE(((uintptr_t)frames->d_desc & 15) == 0 && ((uintptr_t)frames->d_xy & 7) == 0, "%s: misaligned frame set", who);
    SLAM_REQUIRE(pts->h_offsets[pts->B] == 0 || pts->d_desc, "%s: null point descriptors", who);
    s2->desc = (const uint4*)frames->d_desc;
    s2->cells = frames->d_cells;
    s2->order = frames->d_order;
    s2->xy = (const float2*)frames->d_xy;
    s2->meta = frames->d_meta;
    s2->level = frames->d_level;
    s2->bins = frames->d_bins;
    s2->cell = (double)frames->cell;
    return SLAM_OK;
}
