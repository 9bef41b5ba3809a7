// bf_mx_common.h — what the two matrix-core top-2 kernels share: bf_top2_mx_kernel (bf_mx.hip, 16x16x128 tiles) and
// bf_top2_mx32_kernel (bf_mx32.hip, 32x32x64 tiles).  One copy of the +-1 FP4 expand map, the pair union, the exchange limit
// and the stage geometry; the planner, the routing and the launch stay in bf_mx.hip, which launches either kernel (and the
// 32x32x64 kernel's sibling that is fed from a prepared image of the train set).
#pragma once
#include "internal.h"
#include "bf_common.h"

#define SLAM_MX_STAGE 128        // train rows per LDS stage: 16 KiB expanded, two stages per block
#define SLAM_MX_BOUND_LIMIT 0x7F000000u   // bound[] of these kernels holds keys below this; at or above (the idle pattern): nobody has published
// Early bound exchanges: bit k set = the workers of a query block also exchange after the stage at whose end a block has scanned
// 128 k rows since launch (k < 32).  Until its first exchange with news in it a worker knows only its own rows, and nearly every
// tile of its first chunk takes the update path; the rule is in the file header of bf_mx.hip, the measured choice in DESIGN.md 3c.
#define SLAM_MX_EARLY 0x16u      // after 128, 256 and 512 rows
#define SLAM_MX_RESIDENT 4       // blocks of either kernel a CU holds at once (the plan describe counts on it; launches ask)

// The phase probe (tools/mx_phase_probe.py): an experiment build (-DSLAM_MX_PROBE) in which every wave of either kernel sums the
// shader clock over the phases of its life (pacc, plast: the kernel's locals) and leaves the sums in a buffer of the tool's.
// The shipped build executes no stamp.
// phases: 0 prologue, 1 chunk start, 2 quiet scan, 3 update paths, 4 stage end (unions, early exchange), 5 stage barrier
// (arrival to release), 6 epilogue, 7 stage head (the ticket's draw and its wait)
#ifdef SLAM_MX_PROBE
#define MX_STAMP(ph) do { const unsigned long long now_ = __builtin_readcyclecounter(); pacc[ph] += now_ - plast; plast = now_; } while (0)
#else
#define MX_STAMP(ph) do {} while (0)
#endif

typedef int mx_v8i __attribute__((ext_vector_type(8)));

// 32 descriptor bits -> 32 FP4 elements (-1.0 for a set bit, +1.0 for a clear one: the bit is the sign bit as it stands): nibble
// n of word w = bit 4n + w.  The query rows go through this form; the kernels' staging has the same map as one shift and one
// v_and_or_b32 per word (mx_expand_op): a change of the map changes both.
__device__ __forceinline__ uint4 mx_expand(u32 x) {
    uint4 r;
    r.x = ((x << 3) & 0x88888888u) | 0x22222222u;
    r.y = ((x << 2) & 0x88888888u) | 0x22222222u;
    r.z = ((x << 1) & 0x88888888u) | 0x22222222u;
    r.w = (x & 0x88888888u) | 0x22222222u;
    return r;
}

// mx_expand with one v_and_or_b32 per output word.  A VOP3 instruction of gfx950 reads at most one scalar or literal operand,
// so the compiler, given both masks as constants, splits each into an AND and an OR: the OR mask (fill = 0x22222222) is held
// in a VGPR by the caller.
__device__ __forceinline__ uint4 mx_expand_op(u32 v, u32 fill) {
    uint4 r;
    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(r.x) : "v"(v << 3), "s"(0x88888888u), "v"(fill));
    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(r.y) : "v"(v << 2), "s"(0x88888888u), "v"(fill));
    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(r.z) : "v"(v << 1), "s"(0x88888888u), "v"(fill));
    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(r.w) : "v"(v), "s"(0x88888888u), "v"(fill));
    return r;
}

// top-2 of two top-2 pairs whose keys are distinct rows (or none)
__device__ __forceinline__ void mx_unite(u32& b1, u32& b2, u32 c1, u32 c2) {
    const u32 n2 = min(max(b1, c1), min(b2, c2));
    b1 = min(b1, c1);
    b2 = n2;
}

// The threshold x that a key g read from bound[] allows from row c0 on (x is exclusive: a row passes when its distance is below
// x).  Another worker's key excludes ties only when ITS row is below c0 - the row is tested, not inferred from the ticket order:
// a worker can publish from a later chunk before a slower one reads the bound for an earlier chunk.
__device__ __forceinline__ u32 mx_bound_x(u32 g, int c0) {
    return g < SLAM_MX_BOUND_LIMIT ? (g >> SLAM_KEY_IDX_BITS) + ((g & SLAM_KEY_IDX_MASK) < (u32)c0 ? 0u : 1u)
                                   : SLAM_KEY_NONE >> SLAM_KEY_IDX_BITS;
}

// Both kernels take the same arguments: grid = (query blocks, workers), 256 threads; see bf_mx.hip.
__global__ void bf_top2_mx32_kernel(const uint4* __restrict__ q, int N, const uint4* __restrict__ t, const int* __restrict__ tbl,
                                    bf_state st, int train_base, int2* __restrict__ out_idx, int2* __restrict__ out_dist,
                                    uint4* __restrict__ keep, int nchunks, bf_select sel);
// The 32x32x64 search fed from the prepared image of the train set (bf_mx32.hip): t is the image, not the compact rows.
__global__ void bf_mx32_image_top2_kernel(const uint4* __restrict__ q, int N, const uint4* __restrict__ t, const int* __restrict__ tbl,
                                          bf_state st, int train_base, int2* __restrict__ out_idx, int2* __restrict__ out_dist,
                                          uint4* __restrict__ keep, int nchunks, bf_select sel);
// The image: M compact rows -> `rows` expanded rows of 128 bytes (rows = M rounded up to whole stages), one thread per half row.
__global__ void bf_mx_image_kernel(const u32* __restrict__ t, int M, uint4* __restrict__ img, int rows);
#define SLAM_MX_IMAGE_ROW_BYTES 128   // an expanded row: 8 source words x 16 bytes
