// bf_common.h - device helpers and merge state shared by the Hamming searches of libslamhip.so: the top-2 search
// (bf_hamming.hip) and the top-k search (bf_topk.hip).  Not part of the C ABI.
#pragma once
#include "internal.h"

typedef uint32_t u32;

#define SLAM_TILE_ROWS 256          // train rows per LDS tile (8 KiB)
#define SLAM_COLD_ROWS 128          // rows folded in unfiltered at a cold chunk start (make_plan; slam_bf_set_tuning [6])
#define SLAM_GROUP_PAIRS 16         // (train rows) x (queries per lane) covered by one filter test
#define SLAM_KEY_IDX_BITS 23
#define SLAM_KEY_IDX_MASK 0x7FFFFFu
#define SLAM_KEY_NONE 0xFFFFFFFFu
#define SLAM_ACC_BIAS 0x80000000u
#define SLAM_BOUND_IDLE 0x7F7F7F7Fu  // bound[] between launches (one byte pattern: restored by memset as well)

// D = popcount(x) + acc in ONE instruction.  Written as asm because hipcc
// re-associates __builtin_popcount(x)+acc chains into bcnt(x,0)+v_add3 (20
// instead of 16 VALU ops per pair).
__device__ __forceinline__ u32 bcnt_acc(u32 x, u32 acc) {
    u32 d;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(d) : "v"(x), "v"(acc));
    return d;
}
__device__ __forceinline__ u32 umed3(u32 a, u32 b, u32 c) { return max(min(a, b), min(max(a, b), c)); }

// LDS byte address of a __shared__ object, and a 16-byte LDS read at address + constant (becomes the offset: field)
__device__ __forceinline__ u32 lds_addr(const uint4* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (u32)(uintptr_t)(const __attribute__((address_space(3))) uint4*)p;
#else
    return 0;
#endif
}
__device__ __forceinline__ uint4 lds_read16(u32 addr, int byte_offset) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(3))) const uint4 lds_u4;
    return *(lds_u4*)(uintptr_t)(addr + byte_offset);
#else
    return make_uint4(0, 0, 0, 0);
#endif
}

// distances of one train row (a = words 0-3, b = words 4-7) to the lane's R queries, biased:
// acc[r] = 2^31 - th[r] + d  =>  d < th[r]  <=>  acc[r] < 2^31 (sign bit clear)
//
// R = 1 issues the row as ONE block: the eight v_xor first (each overwrites its train word, which is dead afterwards,
// so no extra registers), then the eight accumulating v_bcnt, with the wave's PRIORITY raised for the v_bcnt half.
//
// Why the priority (round 3, tools/ubench/cycles.hip, profiles/r03_ubench_cycles.log - all in measured shader cycles,
// s_memtime against s_memrealtime, in-kernel clock 2.35-2.39 GHz): a gfx950 SIMD executes a wave64 VALU instruction
// in 4 cycles and can run TWO at once when they come from different waves and at least one of them is a "simple" op
// (v_xor/and/or/add/mov ...): a stream of v_xor from 8 waves costs 2.08 cycles per instruction, a stream of v_bcnt
// 4.05 - but four waves of pure v_xor next to four waves of pure v_bcnt cost 2.17 per instruction TOGETHER when the
// v_bcnt waves have the higher priority (2.65 with equal priorities, 3.6 when the v_xor waves have it).  v_bcnt can
// only use one of the two issue slots; whoever is served first takes that slot, so a v_xor served first blocks the
// v_bcnt of the next wave for 4 cycles while the second slot idles.  Arbitration is by priority, then age: with equal
// priorities the oldest wave is served first whatever it holds, and every bare loop of this row measured 3.7-4.0 cycles
// per instruction (59-64 per row; the round-2 kernel: 54.9, its waves drift apart at waits and branches).  With
// s_setprio 2 in front of the v_bcnt half and s_setprio 0 in front of the v_xor half, a wave in its v_bcnt half is
// served first and the v_xor of the other waves fill the second slot: the same bare loop runs at 2.24 cycles per
// instruction (35.8 per row), and this kernel went from 1.514 to 1.24-1.26 ms at 64k x 64k (profiles/r03_ab_setprio.log).
// The priority stays raised through the LDS reads and the filter that follow the row (placing s_setprio 0 right
// behind the last v_bcnt measured 2 % slower at 64k x 64k) and is dropped when the scan ends.
template <int R>
__device__ __forceinline__ void row_acc(const u32 (&q)[R][8], uint4 a, uint4 b, const u32 (&init)[R],
                                        u32 (&acc)[R]) {
    if constexpr (R == 1) {
        asm volatile("s_setprio 0\n\t"
            "v_xor_b32 %1, %9, %1\n\tv_xor_b32 %2, %10, %2\n\tv_xor_b32 %3, %11, %3\n\tv_xor_b32 %4, %12, %4\n\t"
            "v_xor_b32 %5, %13, %5\n\tv_xor_b32 %6, %14, %6\n\tv_xor_b32 %7, %15, %7\n\tv_xor_b32 %8, %16, %8\n\t"
            "s_setprio 2\n\t"
            "v_bcnt_u32_b32 %0, %1, %17\n\tv_bcnt_u32_b32 %0, %2, %0\n\tv_bcnt_u32_b32 %0, %3, %0\n\t"
            "v_bcnt_u32_b32 %0, %4, %0\n\tv_bcnt_u32_b32 %0, %5, %0\n\tv_bcnt_u32_b32 %0, %6, %0\n\t"
            "v_bcnt_u32_b32 %0, %7, %0\n\tv_bcnt_u32_b32 %0, %8, %0"
            : "=v"(acc[0]), "+v"(a.x), "+v"(a.y), "+v"(a.z), "+v"(a.w), "+v"(b.x), "+v"(b.y), "+v"(b.z), "+v"(b.w)
            : "v"(q[0][0]), "v"(q[0][1]), "v"(q[0][2]), "v"(q[0][3]), "v"(q[0][4]), "v"(q[0][5]), "v"(q[0][6]),
              "v"(q[0][7]), "v"(init[0]));
        return;
    }
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = bcnt_acc(q[r][0] ^ a.x, init[r]);
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = bcnt_acc(q[r][1] ^ a.y, acc[r]);
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = bcnt_acc(q[r][2] ^ a.z, acc[r]);
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = bcnt_acc(q[r][3] ^ a.w, acc[r]);
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = bcnt_acc(q[r][4] ^ b.x, acc[r]);
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = bcnt_acc(q[r][5] ^ b.y, acc[r]);
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = bcnt_acc(q[r][6] ^ b.z, acc[r]);
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = bcnt_acc(q[r][7] ^ b.w, acc[r]);
}

// Exchange the 2nd-best distance of the lane's queries with the blocks scanning other train chunks.
// bound[q] only ever holds the 2nd-best distance over some subset of the train rows, i.e. an upper
// bound of the final 2nd-best distance g: rows with d > g can be dropped, rows with d == g must stay
// (they may win the tie on index), hence the "+ 1".  The load may be stale; that only loosens it.
// (Measured and dropped: issuing the load at one share point and consuming it at the next, so that a wave never
// sits on the round trip, makes every applied bound one segment staler - 64k x 64k 1528 -> 1551 us,
// 8192 x 65536 212 -> 222 us, 2000 x 2000 21 -> 33 us.)
// gk[r] keeps the last bound seen (an upper bound of the final 2nd-best distance for good: bound[] only decreases
// during a launch); the epilogue uses it to skip merges that cannot matter, without another round trip.
// (Forms measured against each other in round 4, profiles/r04_ab_queue.log "share_bound forms": the returning atomic waited for
// on the spot, round 3's load + no-return atomic, and this one with and without the "nothing before a 2nd neighbour" rule - all
// within 1 % of each other; this is the one whose writes are known to be complete.)
template <int R>
__device__ __forceinline__ void share_bound(u32* __restrict__ bound, int qbase, int N, const u32 (&b2)[R],
                                            u32 (&init)[R], u32 (&gk)[R], u32 (&pend)[R]) {
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int qi = qbase + r * 64;
        if (qi < N) {
            const u32 own = b2[r] >> SLAM_KEY_IDX_BITS;
            // The bound is READ with a relaxed agent-scope load.  A lane whose own 2nd-best beats it publishes it with an
            // atomic minimum in the RETURNING form, whose value nobody waits for here: it is parked in pend[] and consumed
            // at the lane's next exchange or in front of the arrival ticket (vector-memory operations return in issue
            // order, so by then it has long arrived).  Returning on purpose: every write to bound[] is then known to have
            // been performed at the memory side before the block's ticket is drawn, so none can land behind the last
            // arriver's reset (a no-return atomic is only known to have been sent).
            asm volatile("" ::"v"(pend[r]));
            const u32 g = __hip_atomic_load(&bound[qi], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // Nothing is published while the lane has no 2nd neighbour yet (own = 511): a block that starts must still see
            // "nobody has published" (SLAM_BOUND_IDLE) then.
            if (own < g && own <= 256u) pend[r] = atomicMin(&bound[qi], own);
            gk[r] = g;
            init[r] = SLAM_ACC_BIAS - min(own, g + 1);
        }
    }
}

// Per-query merge state shared by the blocks of one launch (device memory owned by the ctx).
// Invariant between launches: best[] = ~0, bound[] = 0x7F7F7F7F, arrivals[] = 0, cursor[] = 0; the last block
// of every query block restores it after decoding, so no memset or merge kernel runs per call.
struct bf_state {
    unsigned long long* best;   // [N]  (1st key << 32 | 2nd key), keys = dist << 23 | train row, ~0 = none
    u32* bound;                 // [N]  upper bound of the final 2nd-best distance (share_bound)
    u32* arrivals;              // [query blocks]  how many chunk blocks have merged their result
    u32* cursor;                // [4 x query blocks] x SLAM_CURSOR_STRIDE  queue plans: the next chunk ticket of each query wave (0
                                // between launches), every cursor on a 128-byte line of its own: returning atomics on one line
                                // serialise at the memory side (with the 128 cursors of the 1/8 shard packed into four lines a
                                // 256-row chunk cost 168 us where one block per chunk took 157: profiles/r04_ab_queue.log)
};

// the context's merge state for up to N queries (bf_hamming.hip; allocated on first use, idle between searches)
int bf_state_get(slam_ctx* ctx, int64_t N, bf_state* out);
