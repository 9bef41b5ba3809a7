// bf_common.h - device helpers and merge state shared by the Hamming searches of libslamhip.so: the top-2 searches
// (bf_hamming.hip, bf_mx.hip) and the top-k, radius and window searches (bf_topk.hip, bf_radius.hip, bf_window.hip).  Not
// part of the C ABI.
#pragma once
#include "internal.h"
#include <vector>

typedef uint32_t u32;

#define SLAM_TILE_ROWS 256          // train rows per LDS tile (8 KiB)
#define SLAM_COLD_ROWS 128          // rows folded in unfiltered at a cold chunk start (make_plan; slam_bf_set_tuning [6])
#define SLAM_GROUP_PAIRS 16         // (train rows) x (queries per lane) covered by one filter test
#define SLAM_KEY_IDX_BITS 23
#define SLAM_KEY_IDX_MASK 0x7FFFFFu
#define SLAM_KEY_NONE 0xFFFFFFFFu
#define SLAM_ACC_BIAS 0x80000000u
#define SLAM_BOUND_IDLE 0x7F7F7F7Fu  // bound[] between launches (one byte pattern: restored by memset as well)
#define SLAM_CURSOR_STRIDE 32       // u32 words between the cursors of two query waves (one 128-byte line each)

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

// ---- pieces the one-query-per-lane searches share (bf_topk.hip, bf_radius.hip, bf_window.hip) -------------------------

// query row qi (two uint4) into the lane's eight registers
__device__ __forceinline__ void bf_load_query(const uint4* q, int qi, u32 (&qr)[8]) {
    const uint4 x = q[2 * (size_t)qi], y = q[2 * (size_t)qi + 1];
    qr[0] = x.x; qr[1] = x.y; qr[2] = x.z; qr[3] = x.w;
    qr[4] = y.x; qr[5] = y.y; qr[6] = y.z; qr[7] = y.w;
}

// the Hamming distance of the eight words q to the row (a, b): one accumulating v_bcnt per word
__device__ __forceinline__ u32 bf_hamming256(const u32 (&q)[8], uint4 a, uint4 b) {
    u32 d = bcnt_acc(q[0] ^ a.x, 0);
    d = bcnt_acc(q[1] ^ a.y, d);
    d = bcnt_acc(q[2] ^ a.z, d);
    d = bcnt_acc(q[3] ^ a.w, d);
    d = bcnt_acc(q[4] ^ b.x, d);
    d = bcnt_acc(q[5] ^ b.y, d);
    d = bcnt_acc(q[6] ^ b.z, d);
    return bcnt_acc(q[7] ^ b.w, d);
}

// One group of U rows of the LDS tile tp from row j, read rolling one row ahead through one LDS address + immediate
// offsets (bf_top2_block): a0 / c0 hold row j on entry and row j + U on return.
template <int U>
__device__ __forceinline__ void bf_group_acc(const u32 (&qr)[1][8], const uint4* tp, int j, uint4& a0, uint4& c0,
                                             const u32 (&ini)[1], u32 (&acc)[U][1]) {
    u32 base = lds_addr(tp + 2 * j);
#pragma unroll
    for (int u = 0; u < U; u += 2) {
        const uint4 a1 = lds_read16(base, (2 * u + 2) * 16), c1 = lds_read16(base, (2 * u + 3) * 16);
        row_acc<1>(qr, a0, c0, ini, acc[u]);
        asm volatile("" : "+v"(base) : "v"(acc[u][0]));
        a0 = lds_read16(base, (2 * u + 4) * 16);
        c0 = lds_read16(base, (2 * u + 5) * 16);
        row_acc<1>(qr, a1, c1, ini, acc[u + 1]);
        asm volatile("" : "+v"(base) : "v"(acc[u + 1][0]));
    }
}

// a packed key dist << 23 | row as its row (+ base) and its distance; SLAM_KEY_NONE as "no match"
__device__ __forceinline__ int bf_key_idx(u32 key, int base) {
    return key == SLAM_KEY_NONE ? SLAM_NO_MATCH_IDX : (int)(key & SLAM_KEY_IDX_MASK) + base;
}
__device__ __forceinline__ int bf_key_dist(u32 key) {
    return key == SLAM_KEY_NONE ? SLAM_NO_MATCH_DIST : (int)(key >> SLAM_KEY_IDX_BITS);
}

// exclusive scan of one value per thread over a 256-thread block (lds4: four words of LDS); *total = the block's sum
template <typename T>
__device__ __forceinline__ T bf_block_excl_scan(T v, T* lds4, T* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
    if (lane == 63) lds4[wave] = x;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        before += w < wave ? lds4[w] : 0;
        all += lds4[w];
    }
    __syncthreads();
    *total = all;
    return before + x - v;
}

// A wave's own LDS operations complete in order, so waiting for them is all the hand-off between its lanes needs.
__device__ __forceinline__ void bf_wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

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

// Selection fused into the decode (round 4): the last arriver of a query block has (k1, k2) of its queries
// in hand, so the selections that need NO reduction over the queries - "has a neighbour" (bf.match, feature_matchers.py:39,44)
// and the Lowe ratio test - are made there: one flag per query, and how many each wave kept (a plain store per wave: nothing
// to zero beforehand, the host adds them up).  A search + ratio test on resident rows is ONE launch instead of two.
struct bf_select {
    uint8_t* keep;        // [N] 1 = kept; null = no selection
    int* wave_kept;       // [ceil(N / 64)] rows kept in each group of 64 consecutive queries (device or pinned host memory)
    double param;         // mode 2: the ratio
    int mode;             // 0 = keep every query that has a neighbour, 2 = Lowe ratio: dist0 < param * dist1 (needs two neighbours)
    unsigned epoch;       // what the last arriver of query block x stores into done[x] once its results are visible to the host
    unsigned* done;       // pinned host memory, or null: the caller synchronises the stream instead of polling (slam_wait_done)
};

// ---- epilogue of the top-2 searches (bf_top2_kernel, bf_top2_mx_kernel): merge, then the last arriver of this query block decodes
// Lane `lane` of wave (tid >> 6) holds the top-2 (b1, b2) of the queries qbase + r * 64 (r < R); gk / pend: what the exchanges
// left (share_bound / share_union); S_e: blocks that arrive for each query block; s_last: a __shared__ word of the caller.
// (The arguments N_e ... od_e arrive in vector registers where the caller parked them in front of its scan.)
template <int R, bool QUEUE>
__device__ __forceinline__ void bf_top2_epilogue(const bf_state st, const int bx, const int tid, const int lane, const int qbase,
                                                 const bool merging, const bool leader, const u32 (&b1)[R], const u32 (&b2)[R],
                                                 const u32 (&gk)[R], const u32 (&pend)[R], const int N_e, const int S_e,
                                                 const int base_e, int2* const oi_e, int2* const od_e, const bf_select sel,
                                                 u32& s_last) {
    __builtin_amdgcn_s_setprio(0);   // the scan raised it (row_acc); merges and tickets run at the default priority
    // Merge into best[q] = (1st key << 32 | 2nd key) with TWO 32-bit atomic minima instead of a 64-bit CAS loop: the 1st
    // key goes into the high half with a returning atomicMin; whichever of (what was there, mine) lost, or my 2nd key if
    // that is smaller, goes into the low half.  Every key is distinct, so: the high half ends as the smallest key m; m is
    // never pushed into the low half (its holder pushes min(loser, own 2nd), both > m; everybody else pushes keys > m);
    // and the second smallest key s always is (if s is somebody's 1st key it either loses against m directly or is
    // displaced by m later, and the displacing thread pushes it; if it is the 2nd key of m's holder, that thread pushes
    // it).  One round trip, no retries when the 16-64 chunk blocks of a query finish together - the CAS loop paid a
    // load plus one round trip per lost race (epilogue of a 4096 x 4096 block: 6.6 us mean, profiles/r02_block_timeline.log).
    // gk >= the final 2nd-best distance (share_bound): a block whose best row is farther than that cannot contribute and
    // skips the atomics without looking (rows AT that distance may still win the tie on index).
    if (merging) {
    // (merge form of the exchange: a lane whose pair has not changed since its last fold has nothing left to merge)
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int qi = qbase + r * 64;
        if (qi < N_e && b1[r] != SLAM_KEY_NONE && (b1[r] >> SLAM_KEY_IDX_BITS) <= gk[r] &&
            (b2[r] != pend[r] || b2[r] == SLAM_KEY_NONE)) {       // (a lone row: b2 is none, and so was it at the last fold)
            u32* half = (u32*)&st.best[qi];
            const u32 o1 = atomicMin(half + 1, b1[r]);
            const u32 loser = o1 == b1[r] ? SLAM_KEY_NONE : max(o1, b1[r]);
            const u32 push = min(loser, b2[r]);
            if (push != SLAM_KEY_NONE) {
                // returning form on purpose: "the value is back" means the minimum has been taken at the memory side, which is
                // what the arrival ticket below relies on (a no-return atomic is only known to have been sent)
                const u32 o2 = atomicMin(half, push);
                asm volatile("" ::"v"(o2));
            }
        }
    }
    } else {
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int qi = qbase + r * 64;
        if (qi < N_e && b1[r] != SLAM_KEY_NONE && (b1[r] >> SLAM_KEY_IDX_BITS) <= gk[r]) {
            u32* half = (u32*)&st.best[qi];                       // little endian: [0] = 2nd key, [1] = 1st key
            const u32 o1 = atomicMin(half + 1, b1[r]);
            const u32 push = min(max(o1, b1[r]), b2[r]);
            if (leader) {
                // leaders leave the 2nd key of everything merged so far as the bound (an upper bound of the final one:
                // the low half only ever holds keys other than the smallest)
                const u32 k2 = min(atomicMin(half, push), push);
                if ((k2 >> SLAM_KEY_IDX_BITS) < gk[r]) {           // returning form, like every write to bound[] (share_bound)
                    const u32 ob = atomicMin(&st.bound[qi], k2 >> SLAM_KEY_IDX_BITS);
                    asm volatile("" ::"v"(ob));
                }
            } else if (push != SLAM_KEY_NONE) {
                // returning form on purpose: "the value is back" means the minimum has been taken at the memory side, which is
                // what the arrival ticket below relies on (a no-return atomic is only known to have been sent)
                const u32 o2 = atomicMin(half, push);
                asm volatile("" ::"v"(o2));
            }
        }
    }
    }
    // Arrival ticket.  Everything a block contributes travels in agent-scope INTEGER atomics in the RETURNING form
    // (global_atomic_umin ... sc0: the merges above, every write to bound[] in share_bound / share_union), and what is relied
    // on is this, no more:
    //   (1) a returned value means the read-modify-write has been performed at the point all XCDs share - an agent-scope
    //       atomic is never satisfied from an XCD's own L2 (the guide measures that for float atomics, "Global float atomics";
    //       for the integer minima used here it is what 140 000 + 46 000 fuzzed searches and the state soaks of rounds 3 / 4
    //       show, and what makes cross-XCD merges come out right at all), and nothing of it stays dirty in an L2;
    //   (2) every wave waits for all its returns (s_waitcnt vmcnt(0): vector-memory operations return in issue order), then
    //       the block barrier, then ONE lane's relaxed agent-scope ticket - the guide's hand-off table, first row: "an
    //       agent-scope atomic add ... after every storing wave's vmcnt(0) wait ... the workgroup whose add came last, told by
    //       the value its add returned";
    //   (3) the block that draws the last ticket passes a barrier and TAKES the slots with returning 8-byte atomic exchanges
    //       (which also put them back to idle): agent-scope atomics on BOTH sides of the hand-off - the guide's "{8-B agent
    //       atomics both sides}" form - so no load is involved that an L1 or an XCD's L2 could serve, and no acquire fence is
    //       needed (round 3 read the slots with sc1 loads behind a buffer_inv sc1: 4096 x 4096 16.2 -> 15.6 us without it, other
    //       sizes equal; profiles/r04_ab_queue.log "swap").
    // The G16 counter recipe has an agent-scope RELEASE fence (buffer_wbl2 sc1) in front of the ticket; it writes back dirty L2
    // lines, of which this hand-off has none, and cost 1.7 us on the critical path of every block: 4096 x 4096 18.4 -> 16.7 us,
    // 2000 x 2000 10.7 -> 9.4 us, the 1/8 shard 159.9 -> 154.8 us without it (profiles/r03_ab_cold_start.log).
    // tests/test_isa_handoff_cpu.py holds every build to (1)-(3) on the disassembly (return forms, wait and barrier in front
    // of the ticket, returning exchanges behind it; profiles/r04_isa_handoff_excerpt.txt), and every search leaves the
    // whole state idle, which the GPU tests assert on the state itself (slam_bf_state_dirty).  Placement-independent: nothing
    // relies on which XCD a block runs on.
    if (!merging) {
#pragma unroll
        for (int r = 0; r < R; r++) asm volatile("" ::"v"(pend[r]));   // the parked returns of share_bound
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        const u32 ticket = __hip_atomic_fetch_add(&st.arrivals[bx], 1u, __ATOMIC_RELAXED,
                                                  __HIP_MEMORY_SCOPE_AGENT);
        s_last = ticket == (u32)S_e - 1 ? 1u : 0u;
        asm volatile("" ::"s"(ticket));                 // (the ticket is back: its value was just used)
    }
    __syncthreads();
    if (!s_last) return;
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int qi = qbase + r * 64;
        int kept = 0;
        if (qi < N_e) {
            // every contribution was made by an agent-scope atomic; it is taken - and the slot put back to idle for the next
            // launch - by one more (all other blocks are done with these queries)
            const unsigned long long v = __hip_atomic_exchange(&st.best[qi], ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const u32 k1 = (u32)(v >> 32), k2 = (u32)v;
            int2 oi, od;
            oi.x = k1 == SLAM_KEY_NONE ? SLAM_NO_MATCH_IDX : (int)(k1 & SLAM_KEY_IDX_MASK) + base_e;
            od.x = k1 == SLAM_KEY_NONE ? SLAM_NO_MATCH_DIST : (int)(k1 >> SLAM_KEY_IDX_BITS);
            oi.y = k2 == SLAM_KEY_NONE ? SLAM_NO_MATCH_IDX : (int)(k2 & SLAM_KEY_IDX_MASK) + base_e;
            od.y = k2 == SLAM_KEY_NONE ? SLAM_NO_MATCH_DIST : (int)(k2 >> SLAM_KEY_IDX_BITS);
            oi_e[qi] = oi;
            od_e[qi] = od;
            if (sel.keep) {
                // (double) comparisons of integers <= 256: exact, and the same arithmetic as filter_keep_kernel
                const bool k = oi.x >= 0 && (sel.mode == 0 || (oi.y >= 0 && (double)od.x < sel.param * (double)od.y));
                sel.keep[qi] = k ? 1 : 0;
                kept = k ? 1 : 0;
            }
            if (!merging) __hip_atomic_store(&st.bound[qi], SLAM_BOUND_IDLE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (sel.keep && qi - lane < N_e) {                   // (wave-uniform: the group's first query exists)
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) kept += __shfl_xor(kept, off, 64);
            if (lane == 0) sel.wave_kept[qi >> 6] = kept;
        }
    }
    if (tid == 0) __hip_atomic_store(&st.arrivals[bx], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (QUEUE && tid < 4)   // every worker of this query block has arrived, so nobody draws a ticket any more
        __hip_atomic_store(&st.cursor[(size_t)(4 * bx + tid) * SLAM_CURSOR_STRIDE], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (__builtin_expect(sel.done != nullptr, 0)) {   // (laid out behind the common path: tests/test_isa_handoff_cpu.py reads the text in order)
        // A host thread polls done[bx] instead of synchronising the stream (frame-sized calls: 4 us less per call,
        // tools/ubench/sync_vs_poll.hip).  Every thread makes its own result stores visible at system scope, the block meets,
        // one lane releases the flag.  The state restores above need no such care: the next launch is ordered behind this
        // one by the stream.
        __threadfence_system();
        __syncthreads();
        if (tid == 0) __hip_atomic_store(&sel.done[bx], sel.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// the chunk boundary table on the device (bf_hamming.hip: a ring of recent tables, uploaded only when it changes)
int bf_table_get(slam_ctx* ctx, const std::vector<int>& tbl, const int** d_tbl);
// the matrix-core search of one pass (bf_mx.hip): whether N x M runs there (engine, knobs, where the rows lie), and the launch
bool bf_mx_route(slam_ctx* ctx, int64_t N, int64_t M, bool rows_on_host);
int bf_mx_pass(slam_ctx* ctx, const void* d_query, int64_t N, const void* d_train, int64_t M, int64_t train_base, int32_t* d_idx,
               int32_t* d_dist, void* d_keep, const bf_select& sel, int* qblocks_out);
