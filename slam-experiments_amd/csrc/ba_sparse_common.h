// ba_sparse_common.h - what the two files of the sparse bundle adjustment share besides ba_common.h: ba_sparse.hip (every phase,
// two residuals per observation, unit information) and ba_stereo.hip (the stereo / weighted forms of the phases that read a
// measurement; the phases themselves are the templates of ba_sparse_phases.h).  No arithmetic here, so the contraction state
// of the including file does not matter.
#pragma once
#include "internal.h"
#include "ba_common.h"

#define BAS_WAVES (BA_THREADS / 64)
#define BAS_ALIGNED16(p) ((((uintptr_t)(p)) & 15) == 0)

// the slice [a0, a1) of a pose's list; a slice that does not lie in the table is taken as empty, and false comes back
__device__ __forceinline__ bool bas_pose_range(const int* __restrict__ ps_ptr, int k, int O, int& a0, int& a1) {
    a0 = ps_ptr[k]; a1 = ps_ptr[k + 1];
    if (a0 < 0 || a1 < a0 || a1 > O) { a0 = a1 = 0; return false; }
    return true;
}

static inline int bas_blocks(int64_t n) { return (int)((n + BA_THREADS - 1) / BA_THREADS); }

// defined in ba_sparse.hip
int bas_sizes(const char* who, int64_t K, int64_t L, int64_t O, int64_t E, int64_t P);
void bas_finish_launch(hipStream_t st, const double* part, int n, double* out, const double* Hpp, const uint8_t* fixed, int K, const double* Hll,
                       int L);
