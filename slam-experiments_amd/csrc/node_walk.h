// node_walk.h - the scan of a search inside one vocabulary node in shareable form: the walk over the segment
// a node has in a pair's grouped side-2 list, as a template over what is done with each row's distance.  The twin of the grid
// walk of grid_walk.h.  bow_match.hip (SearchByBoW) is built on it.  The walk's text exists twice: tm_scan_kernel of
// tri_match.hip (SearchForTriangulation) keeps its own copy, with its gates in front of the top-2 update.  Built on this
// template - its gates as the functor - it computes the same bits, but in the session that timed this form of the walk it
// missed two of its eight lines of the rule it was held to (profiles/pair_scan_time_ab.log).
#pragma once
#include "match_finish.h"

// The rows [seg.x, seg.y) of the grouped side-2 list (order2, rows2) - a node's segment, its two ends by mf_bound<false> and
// mf_bound<true> -, walked four rows ahead: take(distance of the row to q, its side-2 row, whether it lies inside the segment)
// for each, in segment order.  The rows behind the tail of the last four repeat the segment's last row and are handed over as
// outside.  The two searches and the load of q stay with the caller, and the ends come as one int2, because of what was
// measured: with q loaded in front of the searches, or with the ends as two int arguments (the row loads come out in another
// schedule), SearchByBoW took 2 to 9 % longer over 256 pairs (profiles/pair_scan_time_ab.log, sessions 1 and 3).
template <class TAKE>
__device__ __forceinline__ void nw_walk(const int* order2, const uint4* rows2, int2 seg, const u32 (&q)[8], const TAKE& take) {
    const int j0 = seg.x, j1 = seg.y;
    for (int j = j0; j < j1; j += 4) {                  // four rows requested before the first distance is formed
        uint4 a[4], b[4];
        int r[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int jj = min(j + u, j1 - 1);
            a[u] = rows2[2 * (size_t)jj];
            b[u] = rows2[2 * (size_t)jj + 1];
            r[u] = order2[jj];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) take(bf_hamming256(q, a[u], b[u]), r[u], j + u < j1);
    }
}
