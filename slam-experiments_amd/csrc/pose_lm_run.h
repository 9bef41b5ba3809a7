// pose_lm_run.h - what the speculative Levenberg-Marquardt round of the one-launch pose refinements needs around it, one copy for
// pose_opt.hip (two residuals per edge, unit information) and pose_stereo.hip (the stereo / weighted edges of stereo_edge.h):
// the shared-memory block of the round and the offsets clamp at the top of both kernels.  The round itself is
// pose_lm_round.inc, which both files include into their po_run / ps_run.  No floating-point arithmetic here.
#pragma once
#ifndef PO_THREADS
#error "include pose_lm.h first, before any contraction pragma of the file"
#endif

#define PO_SPEC 9                  // trials 1..9 of an iteration, evaluated together after trial 0 was turned down
#define PO_TRIALS (PO_SPEC + 1)    // maxTrialsAfterFailure of g2o's Levenberg-Marquardt: ten trials per iteration

struct po_lm_shared {
    double red[PO_TERMS * PO_RED_STRIDE];
    double part[PO_TERMS * 8];
    double sums[2][PO_TERMS];                       // the evaluation at the current pose / at the candidate: swapped, not copied
    double T0[12], Tcur[12];
    double pose[2][PO_TRIALS * 12];                 // the candidates of an iteration; the buffers alternate, so an accepted
                                                    // candidate stays where it is and becomes the current pose by pointer
    double scale_k[PO_TRIALS], cost_k[PO_SPEC];
    int solved_k[PO_TRIALS];
};

// Frame b of a batch: its edges are [first, first + count) of the concatenated arrays of `total` edges.  A table
// that is not ascending or leaves [0, total] is the caller's bug; it is reported (slam_index_errors) and the frame shrinks to
// what lies inside, never a wild access.
struct po_range { int first, count; };
__device__ __forceinline__ po_range po_frame_range(const int* __restrict__ offsets, int b, int total, unsigned int* index_errors) {
    const int lo = offsets[b], hi = offsets[b + 1];
    const int first = min(max(lo, 0), total), last = min(max(hi, first), total);
    if ((first != lo || last != hi) && threadIdx.x == 0) atomicAdd(index_errors, 1u);
    return {first, last - first};
}
