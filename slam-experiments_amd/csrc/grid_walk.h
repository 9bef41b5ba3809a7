// grid_walk.h - the scan of a search by projection in shareable form: the walk over the grid rows a point's
// window touches, as a template over the test a row inside the window still has to pass and over what is kept of the keys
// dist << 23 | row.  fuse.hip (Fuse) is built on it.  The walk's text exists twice: pm_scan_kernel of proj_match.hip
// (SearchByProjection) carries the text it was lifted from.  Built on this template, with either form of the Hamming distance,
// pm_scan_kernel was timed against itself and missed one line of the rule it was held to (has the figures;
// profiles/pair_scan_time_ab.log all of them).  Everything else the two files share is in proj_search.h, the pair of a scan
// workgroup in match_finish.h.
#pragma once
#include "proj_search.h"

// The Hamming distance of the eight words q and the row (a, b), in plain C++.  It stays beside bf_hamming256 (bf_common.h): on
// the v_bcnt chain fz_refresh_kernel took 372.8 us against 336.3 for 1000 points of 256 observations, and fz_scan_kernel 19.0
// against 18.8 for one pair of 2000 points (profiles/pair_scan_time_ab.log, session 1).
__device__ __forceinline__ u32 gw_hamming(const u32* q, const uint4& a, const uint4& b) {
    return (u32)(((__popc(q[0] ^ a.x) + __popc(q[1] ^ a.y)) + (__popc(q[2] ^ a.z) + __popc(q[3] ^ a.w))) +
                 ((__popc(q[4] ^ b.x) + __popc(q[5] ^ b.y)) + (__popc(q[6] ^ b.z) + __popc(q[7] ^ b.w))));
}

// The rows of the pair's frame strictly inside the window of radius r about (u, v) whose level lies in [l0, l1] and which pass
// gate(pixel, level): take(dist << 23 | row) for each, the distance to descriptor i of desc1.  The run of cells of one grid row
// is one contiguous segment, found by two binary searches.
template <class GATE, class TAKE>
__device__ __forceinline__ void pm_walk(const pm_frames& s2, const mf_pair& pr, const uint4* desc1, int i, double u, double v, double r, int l0,
                                        int l1, const GATE& gate, const TAKE& take) {
    // the grid may only remove rows that are out of window: the cell of a coordinate is monotone in it, and the window's
    // ends are pushed out by far more than the rounding of x - u in the test below can move them
    const double pad_u = 1e-9 * (fabs(u) + r), pad_v = 1e-9 * (fabs(v) + r);
    const int cx0 = pm_cell_of((u - r) - pad_u, s2.cell, s2.gw), cx1 = pm_cell_of((u + r) + pad_u, s2.cell, s2.gw);
    const int cy0 = pm_cell_of((v - r) - pad_v, s2.cell, s2.gh), cy1 = pm_cell_of((v + r) + pad_v, s2.cell, s2.gh);
    const int* cells2 = s2.cells + pr.base2;
    const int* order2 = s2.order + pr.base2;
    const int* meta2 = s2.meta + pr.base2;
    const float2* xy2 = s2.xy + pr.base2;
    const uint4* rows2 = s2.desc + 2 * pr.base2;
    u32 q[8];
    bf_load_query(desc1, i, q);
    for (int cy = cy0; cy <= cy1; cy++) {
        // the two ends of the run of cells [cx0, cx1] of this grid row, searched side by side: one load latency a step, not two
        const u32 c0 = (u32)(cy * s2.gw + cx0), c1 = (u32)(cy * s2.gw + cx1);
        int j0 = 0, h0 = pr.n2, j1 = 0, h1 = pr.n2;
        while (j0 < h0 || j1 < h1) {
            const int m0 = (j0 + h0) >> 1, m1 = (j1 + h1) >> 1;
            const u32 x0 = (u32)cells2[min(m0, pr.n2 - 1)], x1 = (u32)cells2[min(m1, pr.n2 - 1)];
            if (j0 < h0) {
                if (x0 < c0) j0 = m0 + 1;
                else h0 = m0;
            }
            if (j1 < h1) {
                if (x1 <= c1) j1 = m1 + 1;
                else h1 = m1;
            }
        }
        for (int j = j0; j < j1; j += 4) {          // the pixels and levels of four rows requested before the first test
            float2 p[4];
            int m[4];
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int jj = min(j + t, j1 - 1);
                p[t] = xy2[jj];
                m[t] = meta2[jj];
            }
#pragma unroll
            for (int t = 0; t < 4; t++) {
                if (!(j + t < j1 && m[t] >= l0 && m[t] <= l1 && fabs((double)p[t].x - u) < r && fabs((double)p[t].y - v) < r)) continue;
                if (!gate(p[t], m[t])) continue;
                const uint4 a = rows2[2 * (size_t)(j + t)], b = rows2[2 * (size_t)(j + t) + 1];     // (only a row inside the window)
                const u32 d = gw_hamming(q, a, b);
                take((d << SLAM_KEY_IDX_BITS) | (u32)order2[j + t]);
            }
        }
    }
}
