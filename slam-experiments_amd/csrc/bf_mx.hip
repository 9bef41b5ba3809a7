// bf_mx.hip — the top-2 Hamming search of large searches on the MATRIX cores of gfx950 (MI355X), as a dot product of
// +-1 vectors in FP4.  Same results as bf_top2_kernel (bf_hamming.hip), bit for bit; see DESIGN.md §3c.
//
//   * encoding: descriptor bit 1 -> FP4 (E2M1) -1.0 (nibble 0xA), bit 0 -> +1.0 (nibble 0x2): the bit lands in the nibble's sign
//     bit as it stands (a product of two +-1 values does not change when both signs flip, so no NOT).  For 256-bit rows a, b:
//         hamming(a, b) = (256 - <a+-, b+->) / 2
//     Every product is +-1 and every partial sum an integer of magnitude <= 256 + 1022 (the threshold rides in the
//     accumulator, below): the f32 accumulator is exact.  Which bit goes to which K position does not matter as long as
//     both operands use the same map: mx_expand spreads bit 4n + w of a 32-bit word to nibble n of output word w (one
//     shift and one v_and_or per output word).
//   * v_mfma_scale_f32_16x16x128_f8f6f4 with FP4 on both sides (cbsz:4 blgp:4, scale 2^0): D[16 train rows][16 queries]
//     over K = 128 bits; two of them per 256-bit pair.  A wave holds 64 queries as the B operands of four 16-query tiles
//     (2 K-halves x 4 VGPRs each: 32 VGPRs, expanded once from the 32-byte rows); per 16 train rows it issues 8 MFMAs.
//   * train rows reach the A operand through an LDS stage shared by the block's four waves: the block loads 128 compact
//     rows (4 KiB, one 16-byte load per thread), expands them (7 VALU per word) straight into the operand order - group
//     of 16 rows = [K-half][lane] x 16 bytes, so a lane's operand is one conflict-free ds_read_b128 - double buffered,
//     one barrier per stage.  The compact train set (2 MiB at 65536 rows) stays what sits in the L2s.
//   * selection: the accumulator starts at C = 2 e - 256 (e: the lane's inclusive threshold distance for the tile's query), so
//     D >= 0 <=> distance <= e.  Lane (lane & 15, lane >> 4) of tile t holds query 16 t + (lane & 15) against rows
//     4 (lane >> 4) + r: the 16 results of a group fold as bit patterns with v_max3_i32 (exact integers: the sign of the signed
//     maximum says "some D >= 0") into one compare and one branch; the update (laid out as unlikely) runs per tile, only for
//     tiles whose own maximum passes, and is the VALU kernel's on packed keys (dist << 23 | row: med3 / min); a key is
//     (e << 23 | row) - (D << 22), exact modulo 2^32 for every lane of a fired tile, also a lane whose e is -1.  The
//     accumulators and C live in VGPRs (the Makefile's -amdgpu-mfma-vgpr-form for this file): no AGPR round trip.  Each lane
//     keeps the top-2 of ITS rows; the four lanes of a query are united (two xor shuffles) at each chunk start and early
//     exchange, for the bound exchange, and at the end, where lane l takes query 64 wave + l - the layout of bf_top2_kernel's
//     epilogue, shared.
//   * distance ties stay out of the update path where they cannot win.  e only ever falls, to one of:
//       - dist(own 2nd-best) - 1 after a fire, dist(2nd-best of the query's four lanes) - 1 at a chunk start and at an early
//         exchange (not at a stage end): a worker's chunks ascend (tickets), and so do stages, groups and a lane's rows, hence
//         every row the lane has still to see has a higher index than every row in those pairs;
//       - dist(g) - (row(g) < c0 ? 1 : 0) for the key g read from bound[] at the start of the chunk that begins at row c0.
//         bound[] holds the 2nd-best KEY some worker of the query block has published (this kernel's own exchange: bound[] is
//         only read and written by the blocks of one launch, so the encoding is private to it; keys below 0x7F000000 only - at
//         or above, the idle pattern 0x7F7F7F7F included, reads as "nobody has published" - and the epilogue is handed a
//         distance or the idle pattern as before).  The row is TESTED: a worker can finish a later chunk and publish from it
//         before a slower one reads the bound for an earlier chunk, and a tie against such a key can win.
//       - the same, with the first row of the stage to come in place of c0, at the early exchanges (SLAM_MX_EARLY): after the
//         stage at whose end the block has scanned 128, 256 or 512 rows since launch, unless a chunk start follows anyway.  Until
//         then a worker knows only its own rows.  That stage start is the first row the lane has still to see.
//     Why this is exact: a candidate is dropped only if some known 2nd-best key K has dist(K) < dist, or dist(K) == dist and
//     row(K) < row.  Its key then exceeds K, and K is at least the final 2nd key, so the candidate is not in the final top-2.
//     (The code keeps x = e + 1, which is what a key's distance field gives without a subtract and never goes below 0.)
//     tests/test_mx_ties_cpu.py restates these rules in numpy and drives them over adversarial schedules.
//   * row gates: a tile that takes the update path keys and merges, of a lane's four rows, only those at which SOME lane of the
//     tile passes (one compare and one wave-uniform branch per row; on random rows fewer than two of the four).  Why this is
//     exact: a skipped row has D < 0, a distance at or above x, in every lane of the tile, so by the rules above it is not in
//     the final top-2 - the argument that lets a group that does not fire skip all of its rows.  Fewer losing rows now enter a
//     lane's pair, so its 2nd-best key, x, the united pairs and the published keys can be larger than without the gates; they
//     are still keys of real rows, hence valid bounds, and the final tables do not move (tests/test_mx_rowgate_cpu.py asserts
//     both).  The test for rows past the chunk runs only in the groups that the unrolled trips of whole groups leave over.
//     Open: where nearly every row passes (a worker's first stages, and so the short searches at the corners of bf_mx_auto) the
//     four gates are pure cost, 1-3 % there; skipping them until the first exchange with news in it has not been tried.
//   * staging: the load address is a scalar row base plus the thread's fixed offset, the rows are tested against the chunk end
//     only in a stage that is not whole, and each expanded word is one shift and one v_and_or_b32 (28 per thread and stage).
//   * the scan loop overlaps a wave's own serial chain with its MFMAs (DESIGN.md 3c "Operand reads and staging behind the MFMAs"):
//       - operand reads: whole groups run in trips; inside a trip the A operands rotate through three register quads - the first
//         K-half of group g + 1 is read before the MFMAs of group g, its second K-half into the quad that g's four first-half
//         MFMAs free - so the LDS latency of a group's operands runs behind the MFMAs and the fold of the group before it.  The
//         last group of a trip reads nothing ahead, so no read leaves the stage's own buffer or comes before its barrier.
//       - staging: a stage that another follows (always a whole stage) runs as ONE trip of eight groups, and its groups 4-7 each
//         expand and store one of the thread's four source words of the next stage between their second-half MFMAs, in issue
//         slots the pipe-paced MFMAs leave empty.  The other buffer is free from the barrier that opened the stage; the thread's
//         16 source bytes are ONE load at the trip's start, so its latency runs behind groups 0-3 and the stage has one vector
//         memory instruction and one wait where word-by-word loads had four (the kernel is bound by instruction issue: DESIGN.md
//         3c "Where a wave's life goes").  A chunk's first stage is stored at the chunk start as before; a chunk's last stage
//         runs trips of four and stores nothing.
//       - registers (all 128 that four waves per SIMD leave; amdgpu_waves_per_eu holds the allocator to them): the third
//         operand quad is paid for by x, which is no longer kept (threshold_x reads it back from the accumulator start in the
//         update path), and the lane's query and the group's row base, recomputed where used; the staged row is held from the
//         trip's start to the group that expands its last word.
//   * plan: the queue plan of bf_top2_kernel<1, true, true> with tickets drawn per BLOCK: grid = (query blocks, workers),
//     the workers of a query block draw chunks of the boundary table by ticket, exchange the 2nd-best key through
//     bound[] at every chunk, merge with the two returning atomic minima and the last arriver decodes (bf_common.h).
#include "internal.h"
#include <vector>
#include <atomic>
#include <type_traits>

#include "bf_common.h"
#include "bf_mx_common.h"   // the stage geometry, the expand map, the pair union: shared with bf_mx32.hip

#define SLAM_MX_UNROLL 4         // groups of 16 rows per trip of the scan loop

// The phase probe (tools/mx_phase_probe.py; MX_STAMP and the phases are in bf_mx_common.h): this kernel's buffer
#ifdef SLAM_MX_PROBE
__device__ unsigned long long* g_mx_probe = nullptr;
extern "C" __attribute__((visibility("default"))) int slam_exp_set_mx_probe(void* p) {
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_mx_probe), &p, sizeof(p));
}
#endif

typedef float mx_v4f __attribute__((ext_vector_type(4)));

// c + A B over one K-half: A = 16 train rows, B = 16 queries, FP4 on both sides (format code 4), scales 2^0 (E8M0 127)
__device__ __forceinline__ mx_v4f mx_dot(uint4 a, uint4 b, mx_v4f c) {
    const mx_v8i av = {(int)a.x, (int)a.y, (int)a.z, (int)a.w, 0, 0, 0, 0};
    const mx_v8i bv = {(int)b.x, (int)b.y, (int)b.z, (int)b.w, 0, 0, 0, 0};
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bv, c, 4, 4, 0, 127, 0, 127);
}

__device__ __forceinline__ u32 mx_pick(const u32 (&v)[4], int i) {
    return i == 0 ? v[0] : (i == 1 ? v[1] : (i == 2 ? v[2] : v[3]));
}

// grid = (query blocks, workers).  Block (x, y) works for query block (x + y) mod grid.x: the workers of a query block are
// spread over the XCDs, as in the VALU queue plan.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void bf_top2_mx_kernel(const uint4* __restrict__ q, int N, const uint4* __restrict__ t,
                                                         const int* __restrict__ tbl, bf_state st, int train_base,
                                                         int2* __restrict__ out_idx, int2* __restrict__ out_dist,
                                                         uint4* __restrict__ keep, int nchunks, bf_select sel) {
    __shared__ uint4 tile[2][SLAM_MX_STAGE * 8];
    __shared__ u32 s_ticket, s_last;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int kg = lane >> 4, col = lane & 15;
#ifdef SLAM_MX_PROBE
    unsigned long long pacc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, plast = __builtin_readcyclecounter();
#endif
    const u32 lanek = (u32)(4 * kg - (1 << SLAM_KEY_IDX_BITS));  // the lane's first row in a group of 16, less the 2^23 a key built from x owes
    const int bx = ((int)blockIdx.x + (int)blockIdx.y) % (int)gridDim.x;
    // the lane's query in the epilogue and in the bound exchange: worked out afresh at each of them (the empty asm hides that the
    // value repeats), or it and the addresses built on it hold registers through the scan
    auto lane_query = [&]() -> int {
        int v = tid;
        asm volatile("" : "+v"(v));
        return bx * 256 + v;
    };

    // the wave's 64 queries as B operands: tile tt, K-half h = words 4 h + (lane >> 4) of query 64 wave + 16 tt + (lane & 15)
    uint4 qb[4][2];
    const u32* qw = (const u32*)q;
#pragma unroll
    for (int tt = 0; tt < 4; tt++) {
        int qi = bx * 256 + wave * 64 + tt * 16 + col;
        qi = qi < N ? qi : N - 1;                                // tail columns compute a duplicate and are never stored
#pragma unroll
        for (int h = 0; h < 2; h++) qb[tt][h] = mx_expand(qw[(size_t)qi * 8 + h * 4 + kg]);
    }
    if (const int qbase = lane_query(); keep && blockIdx.y == 0 && qbase < N) {   // the caller wants the query rows left in device memory
        keep[2 * (size_t)qbase] = q[2 * (size_t)qbase];
        keep[2 * (size_t)qbase + 1] = q[2 * (size_t)qbase + 1];
    }

    // per tile: the lane's own top-2 over its rows and the EXCLUSIVE threshold distance x (a row passes when its distance is below
    // x; x - 1 is the inclusive threshold e of the file header), kept as what a key's distance field gives without a subtract.
    // The accumulator starts at 2 (x - 1) - 256.  x only ever falls.
    // x is not kept: it is read back from the accumulator start where a tile's threshold moves (threshold_x), which is rare.
    u32 b1[4], b2[4];
    mx_v4f cth[4];
    auto set_threshold = [&](int tt, u32 x) {
        const float c = (float)(2 * (int)x - 258);
        cth[tt] = mx_v4f{c, c, c, c};
    };
    auto threshold_x = [&](int tt) -> u32 { return (u32)((int)cth[tt][0] + 258) >> 1; };
#pragma unroll
    for (int tt = 0; tt < 4; tt++) {
        b1[tt] = b2[tt] = SLAM_KEY_NONE;
        set_threshold(tt, SLAM_KEY_NONE >> SLAM_KEY_IDX_BITS);   // 511: everything passes
    }
    // the top-2 of one tile's query over the rows of all four lanes that hold it (ds_bpermute: it issues beside the VALU, which
    // is what bounds this kernel; the v_permlane16/32_swap form costs two copies and a wait per swap there and measured slower)
    auto unite_tile = [&](int tt, u32& u1, u32& u2) {
        u1 = b1[tt];
        u2 = b2[tt];
#pragma unroll
        for (int off = 16; off <= 32; off <<= 1) {
            const u32 c1 = (u32)__shfl_xor((int)u1, off, 64), c2 = (u32)__shfl_xor((int)u2, off, 64);
            mx_unite(u1, u2, c1, c2);
        }
    };
    auto unite_lanes = [&](u32 (&u1)[4], u32 (&u2)[4]) {
#pragma unroll
        for (int tt = 0; tt < 4; tt++) unite_tile(tt, u1[tt], u2[tt]);
    };
    // Exchange with the other workers of this query block through bound[], at the start of the chunk that begins at row c0 (lane
    // l speaks for query 64 wave + l).  This kernel's own form of share_bound (bf_common.h): bound[] holds the 2nd-best KEY, see
    // the file header; the relaxed load, the parked returning minimum (pend) and "nothing before a 2nd neighbour" are as there.
    u32 gkey = SLAM_BOUND_IDLE, pend[1] = {0u};
    auto exchange = [&](int c0) {
        u32 u1[4], u2[4];
        unite_lanes(u1, u2);
        if (const int qbase = lane_query(); qbase < N) {
            const u32 own = mx_pick(u2, kg);
            asm volatile("" ::"v"(pend[0]));
            const u32 g = __hip_atomic_load(&st.bound[qbase], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (own < g && own < SLAM_MX_BOUND_LIMIT) pend[0] = atomicMin(&st.bound[qbase], own);
            gkey = g;
        }
#pragma unroll
        for (int tt = 0; tt < 4; tt++) {
            // the united pair comes from this worker's earlier chunks, rows below c0: ties against it lose.  Another worker's
            // key excludes ties only when ITS row is below c0 - the row is tested, not inferred from the ticket order: a worker
            // can publish from a later chunk before a slower one reads the bound for an earlier chunk
            const u32 g = (u32)__shfl((int)gkey, tt * 16 + col, 64);
            const u32 gx = mx_bound_x(g, c0);
            set_threshold(tt, min(threshold_x(tt), min(gx, u2[tt] >> SLAM_KEY_IDX_BITS)));
        }
    };

    // staging: thread tid carries half (tid & 1) of row (tid >> 1) of a stage, i.e. the source words 4 h .. 4 h + 3, which
    // become the operand words of lanes 16 g + (row & 15), g = 0..3, of K-half h in the row's group of 16
    const int srow = tid >> 1, sh = tid & 1;
    // The load address is a wave-uniform row base (scalar side) plus the thread's fixed offset, and rows are tested against the
    // chunk end only in a stage that is not whole: the table's chunks are whole stages except at the end of the train set.
    auto load_stage = [&](int s, int c1) -> uint4 {
        const uint4* ts = t + 2 * (size_t)s;
        if (s + SLAM_MX_STAGE <= c1) return ts[(u32)tid];
        return s + srow < c1 ? ts[(u32)tid] : make_uint4(0, 0, 0, 0);
    };
    // mx_expand with one v_and_or_b32 per output word (mx_expand_op, bf_mx_common.h): the OR mask is held in a VGPR here
    const u32 fill = 0x22222222u;
    auto expand = [&](u32 v) -> uint4 { return mx_expand_op(v, fill); };
    uint4* const dst0 = tile[0] + (srow >> 4) * 128 + sh * 64 + (srow & 15);
    auto store_stage = [&](int b, uint4 v) {
        uint4* dst = dst0 + b * (SLAM_MX_STAGE * 8);
        dst[0] = expand(v.x);
        dst[16] = expand(v.y);
        dst[32] = expand(v.z);
        dst[48] = expand(v.w);
    };

    u32* const cursor = st.cursor + (size_t)(4 * bx) * SLAM_CURSOR_STRIDE;
    if (tid == 0) s_ticket = __hip_atomic_fetch_add(cursor, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    int ci = __builtin_amdgcn_readfirstlane((int)s_ticket);
    int scanned = 0;                                             // wave-uniform: the rows this block has scanned since launch
    MX_STAMP(0);
    while (ci < nchunks) {
        const int c0 = tbl[ci], c1 = tbl[ci + 1];
        const uint4 first = load_stage(c0, c1);
        exchange(c0);
        store_stage(0, first);
        __syncthreads();
        MX_STAMP(1);
        int buf = 0;
        for (int s0 = c0; s0 < c1; s0 += SLAM_MX_STAGE) {
            const int s1 = s0 + SLAM_MX_STAGE;
            const bool more = s1 < c1;
            // the next ticket is drawn while the chunk's last stage is scanned; read behind the stage's barrier
            if (!more && tid == 0) s_ticket = __hip_atomic_fetch_add(cursor, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            MX_STAMP(7);
            const int ng = __builtin_amdgcn_readfirstlane(min(SLAM_MX_STAGE / 16, (c1 - s0 + 15) >> 4));
            const uint4* tp = tile[buf];
            auto dots0 = [&](const uint4& a, mx_v4f (&acc)[4]) {
#pragma unroll
                for (int tt = 0; tt < 4; tt++) acc[tt] = mx_dot(a, qb[tt][0], cth[tt]);
            };
            // fold the 16 results of group g and, where some lane passes, take the update path
            auto fold = [&](int g, mx_v4f (&acc)[4], auto rag) {
                // the results are exact integers in f32 (never -0): "any D >= 0" is the sign of the signed maximum of the bit
                // patterns - eight three-input maxima, nothing to canonicalise
                int p[4];
#pragma unroll
                for (int tt = 0; tt < 4; tt++)
                    p[tt] = max(max(__float_as_int(acc[tt][0]), __float_as_int(acc[tt][1])), __float_as_int(acc[tt][2]));
                int m = max(max(p[0], __float_as_int(acc[0][3])), p[1]);
                m = max(max(m, __float_as_int(acc[1][3])), p[2]);
                m = max(max(m, __float_as_int(acc[2][3])), p[3]);
                m = max(m, __float_as_int(acc[3][3]));
                if (__builtin_expect(__ballot(m >= 0) != 0ull, 0)) {
                    MX_STAMP(2);
                    // D = dot + 2 e - 256, so the distance (256 - dot) / 2 is e - D / 2 (D is even).  Only the tiles that hold a
                    // candidate are updated (wave-uniform branches on the tile's own maximum), and only those get a new
                    // threshold: below the lane's own 2nd-best, whose row is below every row the lane has still to see
                    // (the group's first row is taken from the scalar side here: as a per-lane value it would be carried, and
                    // advanced, through every group that does not fire)
                    // (and kept there: folded into lanek it would be one more register per group of an unrolled trip)
                    int row0 = s0 + g * 16;
                    asm("" : "+s"(row0));
                    const u32 rowk = (u32)row0 + lanek;
#pragma unroll
                    for (int tt = 0; tt < 4; tt++) {
                        if (__ballot(max(p[tt], __float_as_int(acc[tt][3])) >= 0) == 0ull) continue;
                        // key = (e - D / 2) << 23 | row with e = x - 1: base + r + (-D << 22), exact modulo 2^32 also for x = 0
                        const u32 xt = threshold_x(tt);
                        const u32 base = (xt << SLAM_KEY_IDX_BITS) + rowk;
                        // row gates: of a lane's four rows only those at which SOME lane of the tile passes are keyed and merged
                        // (wave-uniform branches); see "row gates" in the file header
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            if (__ballot(__float_as_int(acc[tt][r]) >= 0) == 0ull) continue;
                            u32 key = base + (u32)r + ((u32)(int)(-acc[tt][r]) << (SLAM_KEY_IDX_BITS - 1));
                            if constexpr (decltype(rag)::value)   // the rows past the end of a short stage never enter
                                key = (int)rowk + r < c1 - (1 << SLAM_KEY_IDX_BITS) ? key : SLAM_KEY_NONE;
                            b2[tt] = umed3(b1[tt], b2[tt], key);
                            b1[tt] = min(b1[tt], key);
                        }
                        set_threshold(tt, min(xt, b2[tt] >> SLAM_KEY_IDX_BITS));
                    }
                    MX_STAMP(3);
                }
            };
            auto group = [&](int g, auto rag) {
                const uint4 a0 = tp[g * 128 + lane], a1 = tp[g * 128 + 64 + lane];
                mx_v4f acc[4];
                dots0(a0, acc);
#pragma unroll
                for (int tt = 0; tt < 4; tt++) acc[tt] = mx_dot(a1, qb[tt][1], acc[tt]);
                fold(g, acc, rag);
            };
            // A trip of NG whole groups from group g0 on.  The A operands rotate through three quads: the first K-half of group
            // g + 1 is read before the MFMAs of group g, its second K-half once g's four first-half MFMAs have issued (into the
            // quad they free), so a group's operand reads run behind the MFMAs and the fold of the group before it.  The last
            // group of a trip reads nothing ahead: a trip stays inside its own stage buffer.  The barriers keep this order, or
            // the registers of four waves per SIMD run out.
            // With `shadow`, the trip's last four groups also expand and store one source word each of the NEXT stage (into
            // buffer buf ^ 1, free since the barrier that opened this stage) between their second-half MFMAs, in issue slots the
            // pipe-paced MFMAs leave empty.
            auto trip = [&](int g0, auto ngc, auto shadow) {
                constexpr int NG = decltype(ngc)::value;
                constexpr bool SH = decltype(shadow)::value;
                const uint4* ap = tp + g0 * 128 + lane;
                uint4* const dst = dst0 + (buf ^ 1) * (SLAM_MX_STAGE * 8);
                // the thread's 16 bytes of the next stage, one load at the trip's start: its latency runs behind groups 0-3, and
                // groups 4-7 expand a word each.  Were the next stage not whole, the rows past the chunk end would read its last
                // row instead (what such a row holds never matters, the scan tests its index); the planner's tails make every
                // short stage a chunk of its own, so this only keeps the load inside the train set whatever the table
                u32 nx[4] = {0, 0, 0, 0};
                if (SH) {
                    const uint4 x = (t + 2 * (size_t)s1)[2 * min(srow, c1 - 1 - s1) + sh];
                    nx[0] = x.x; nx[1] = x.y; nx[2] = x.z; nx[3] = x.w;
                }
                uint4 a0 = ap[0], a1 = ap[64];
#pragma unroll
                for (int k = 0; k < NG; k++) {
                    uint4 a0n = a0, a1n = a1;
                    mx_v4f acc[4];
                    if (k + 1 < NG) a0n = ap[(k + 1) * 128];
                    const u32 v = nx[SH && k >= NG - 4 ? k - (NG - 4) : 0];
                    __builtin_amdgcn_sched_barrier(0);
                    dots0(a0, acc);
                    __builtin_amdgcn_sched_barrier(0);
                    if (SH && k >= NG - 4) {
                        const int j = k - (NG - 4);
                        uint4 e;
                        acc[0] = mx_dot(a1, qb[0][1], acc[0]);
                        __builtin_amdgcn_sched_barrier(0);
                        asm volatile("v_lshlrev_b32 %0, 3, %1\n\tv_and_or_b32 %0, %0, %2, %3" : "=v"(e.x) : "v"(v), "s"(0x88888888u), "v"(fill));
                        asm volatile("v_lshlrev_b32 %0, 2, %1" : "=v"(e.y) : "v"(v));
                        __builtin_amdgcn_sched_barrier(0);
                        acc[1] = mx_dot(a1, qb[1][1], acc[1]);
                        __builtin_amdgcn_sched_barrier(0);
                        asm volatile("v_and_or_b32 %0, %1, %2, %3" : "=v"(e.y) : "v"(e.y), "s"(0x88888888u), "v"(fill));
                        asm volatile("v_lshlrev_b32 %0, 1, %1\n\tv_and_or_b32 %0, %0, %2, %3" : "=v"(e.z) : "v"(v), "s"(0x88888888u), "v"(fill));
                        __builtin_amdgcn_sched_barrier(0);
                        acc[2] = mx_dot(a1, qb[2][1], acc[2]);
                        __builtin_amdgcn_sched_barrier(0);
                        asm volatile("v_and_or_b32 %0, %1, %2, %3" : "=v"(e.w) : "v"(v), "s"(0x88888888u), "v"(fill));
                        dst[16 * j] = e;
                        if (k + 1 < NG) a1n = ap[(k + 1) * 128 + 64];
                        __builtin_amdgcn_sched_barrier(0);
                        acc[3] = mx_dot(a1, qb[3][1], acc[3]);
                    } else {
                        if (k + 1 < NG) a1n = ap[(k + 1) * 128 + 64];
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int tt = 0; tt < 4; tt++) acc[tt] = mx_dot(a1, qb[tt][1], acc[tt]);
                    }
                    fold(g0 + k, acc, std::false_type{});
                    __builtin_amdgcn_sched_barrier(0);
                    a0 = a0n;
                    a1 = a1n;
                }
            };
            // The trips take whole groups only.  A whole stage that another follows runs as one trip of eight with the next
            // stage's staging in its shadow; every other stage runs trips of SLAM_MX_UNROLL and stages at its end.  What the
            // trips leave of a stage runs in the loop below, with the test for rows past the chunk: up to seven groups, the
            // whole ones among them too (correct there, only slower), and only in a short stage - the last stage of the train set.
            const int nwhole = __builtin_amdgcn_readfirstlane(min(SLAM_MX_STAGE / 16, (c1 - s0) >> 4));
            int g = 0;
            if (more) {                                          // then this stage is whole
                trip(0, std::integral_constant<int, SLAM_MX_STAGE / 16>{}, std::true_type{});
                g = SLAM_MX_STAGE / 16;
            }
            for (; g + SLAM_MX_UNROLL <= nwhole; g += SLAM_MX_UNROLL) trip(g, std::integral_constant<int, SLAM_MX_UNROLL>{}, std::false_type{});
            for (; g < ng; g++) group(g, std::true_type{});
            MX_STAMP(2);
            // No union of a query's four lanes here: a stage ends with each lane's threshold at its own 2nd-best.  The united
            // threshold spared 5 % of the fired tiles and cost four LDS round trips in front of the barrier in 27 % of the
            // tile-stages (tools/mx_fire_model.py; DESIGN.md 3c "The stage tail"); the exchanges and the epilogue still unite.
            // an early exchange (SLAM_MX_EARLY): per wave, no barrier; every row still to come is at or above s1.  Not after a
            // chunk's last stage: the chunk-start exchange follows anyway
            scanned += min(s1, c1) - s0;
            if (more && scanned < 32 * SLAM_MX_STAGE && (SLAM_MX_EARLY >> (scanned / SLAM_MX_STAGE) & 1u)) exchange(s1);
            MX_STAMP(4);
            __syncthreads();
            MX_STAMP(5);
            buf ^= 1;
        }
        ci = __builtin_amdgcn_readfirstlane((int)s_ticket);
    }

    u32 u1[4], u2[4];
    unite_lanes(u1, u2);
    const u32 f1[1] = {mx_pick(u1, kg)}, f2[1] = {mx_pick(u2, kg)};
    // the epilogue's skip test takes a DISTANCE that bounds the final 2nd-best one, or the idle pattern when there is none
    const u32 gk[1] = {gkey < SLAM_MX_BOUND_LIMIT ? gkey >> SLAM_KEY_IDX_BITS : SLAM_BOUND_IDLE};
    bf_top2_epilogue<1, true>(st, bx, tid, lane, lane_query(), false, false, f1, f2, gk, pend, N, (int)gridDim.y, train_base, out_idx,
                              out_dist, sel, s_last);
#ifdef SLAM_MX_PROBE
    MX_STAMP(6);
    if (g_mx_probe && lane == 0) {
        unsigned long long* o = g_mx_probe + ((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 4 + wave) * 8;
        for (int i = 0; i < 8; i++) o[i] = pacc[i];
    }
#endif
}

// ---- host side -----------------------------------------------------------

struct bf_mx_plan {
    int qblocks;     // grid.x: query blocks of 256 rows
    int workers;     // grid.y: worker blocks per query block, drawing the chunks of the table by ticket
    int chunk;       // rows of a uniform chunk (a multiple of the stage)
    int S;           // chunks in the table
    int tail;        // shrinking chunks at the end of the table
};

// The MX planner: a pure function of the CU count, the blocks a CU holds and the shape.  Workers: as many as are resident at
// once, at most one per chunk.  Chunks: 1024 rows where a worker has at least 8192 rows to itself, 256 below; from the point
// where the rest would give every worker fewer than two of those, (rest / 2 workers) rows rounded down to whole stages, never
// fewer than one stage - the workers of a query block run dry within a stage of each other.
static bf_mx_plan make_mx_plan_core(int num_cu, int resident, int64_t N, int64_t M, std::vector<int>* tbl) {
    bf_mx_plan p;
    p.qblocks = (int)((N + 255) / 256);
    int64_t W = (int64_t)num_cu * resident / p.qblocks;
    if (W < 1) W = 1;
    if (W > 256) W = 256;
    const int64_t c = M / W >= 8192 ? 1024 : 256;
    std::vector<int>& b = *tbl;
    b.clear();
    b.push_back(0);
    int shrinking = 0;
    for (int64_t at = 0; at < M;) {
        int64_t len = c;
        const int64_t g = (M - at) / (2 * W) / SLAM_MX_STAGE * SLAM_MX_STAGE;
        if (g < len) { len = g < SLAM_MX_STAGE ? SLAM_MX_STAGE : g; shrinking++; }
        at = at + len < M ? at + len : M;
        b.push_back((int)at);
    }
    p.chunk = (int)c;
    p.S = (int)b.size() - 1;
    p.tail = shrinking;
    p.workers = (int)(W < p.S ? W : p.S);
    return p;
}

// The shapes the shipped engine (slam_bf_set_engine 0) runs on the matrix cores: where the engine sweep over 15 x 8 shapes
// (N 500 .. 262144, M 16384 .. 10^6; profiles/r05_mx_sweep.log) measured it at least as fast as the VALU kernel.  Outside: few
// queries against a train set of a few ten thousand rows (2048 x 16384 .. 40000: 10-13 % slower, 500 x 40000 .. 100000: 3-4 %).
static bool bf_mx_auto(int64_t N, int64_t M) {
    return (N >= 8192 && M >= 16384) || (N >= 3000 && M >= 40000) || (N >= 1000 && M >= 65536) || (N >= 500 && M >= 200000);
}

// The MX plan for N x M on a device with num_cu CUs, WITHOUT a device: h_plan int32 [8] = {query blocks, workers per query block,
// uniform chunk rows, chunks, shrinking chunks, rows per LDS stage, blocks per CU counted on, 1 when the shipped engine runs this
// shape on the matrix cores}; the chunk boundary table goes to h_tbl (up to tbl_cap entries; may be NULL), its length to *tbl_len.
extern "C" int slam_bf_mx_plan_describe(int num_cu, int64_t N, int64_t M, int32_t* h_plan, int32_t* h_tbl, int64_t tbl_cap,
                                        int64_t* tbl_len) {
    SLAM_REQUIRE(num_cu >= 1 && num_cu <= 4096, "num_cu out of range");
    SLAM_REQUIRE(N >= 1 && M >= 1 && M <= SLAM_MAX_TRAIN_PER_PASS && N <= (1ll << 30), "bad sizes");
    SLAM_REQUIRE(h_plan && tbl_len && (h_tbl || tbl_cap == 0) && tbl_cap >= 0, "slam_bf_mx_plan_describe: null argument");
    std::vector<int> tbl;
    const bf_mx_plan p = make_mx_plan_core(num_cu, SLAM_MX_RESIDENT, N, M, &tbl);
    h_plan[0] = p.qblocks; h_plan[1] = p.workers; h_plan[2] = p.chunk; h_plan[3] = p.S;
    h_plan[4] = p.tail; h_plan[5] = SLAM_MX_STAGE; h_plan[6] = SLAM_MX_RESIDENT; h_plan[7] = bf_mx_auto(N, M) ? 1 : 0;
    *tbl_len = (int64_t)tbl.size();
    for (int64_t i = 0; i < (int64_t)tbl.size() && i < tbl_cap; i++) h_tbl[i] = tbl[(size_t)i];
    return SLAM_OK;
}

// Which of the two matrix-core kernels the shipped engine runs a shape on that bf_mx_auto sends to the matrix cores: true = the
// 32x32x64 kernel (bf_mx32.hip).  The rule is measured, shape by shape (tools/ab_time.py lib:engine=2,lib:engine=3 --check, the
// whole range of five rounds below the 16x16 kernel's; table in DESIGN.md 3c "The 32x32x64 kernel"); a shape where it is not
// faster stays on the kernel it had.  Measured faster: the four corners of bf_mx_auto, 8192 x 65536, 20000 x 100000, 65536 x
// 65536 and 131072 x 65536 - every measured shape up to 131072 queries (two or more workers per query block on 256 CUs) and
// 200000 train rows.  Measured slower (0.5 %): 2^20 x 2^20, one worker per query block.  Nothing was measured between, so the
// rule is the box the measured gains span.
static bool bf_mx32_auto(int64_t N, int64_t M) {
    return N <= 131072 && M <= 200000;
}

// The kernel a matrix-core pass of N x M runs under `engine` (0, 2 or 3; 1 never gets here): 16 or 32, the M and N of its tiles.
extern "C" int slam_bf_mx_tile_describe(int engine, int64_t N, int64_t M, int32_t* h_tile) {
    SLAM_REQUIRE(h_tile, "slam_bf_mx_tile_describe: null argument");
    SLAM_REQUIRE(engine == 0 || engine == 2 || engine == 3, "engine must be 0 (auto), 2 or 3");
    SLAM_REQUIRE(N >= 1 && M >= 1, "bad sizes");
    *h_tile = engine == 3 || (engine == 0 && bf_mx32_auto(N, M)) ? 32 : 16;
    return SLAM_OK;
}

// The feed of the 32x32x64 kernel under feed 0 (auto): true = from the prepared image (bf_mx_image_kernel, then
// bf_mx32_image_top2_kernel), false = expanded in the kernel by every query block.  The image costs a launch of its own in
// front of the search and removes the staging's vector work from every stage of every block; the rule is measured like
// bf_mx32_auto's (tools/ab_time.py parent,lib --check, the whole range of five rounds below the parent's;
// profiles/mx_feed_ab.log, DESIGN.md 3c "Feed"): a shape where the image is not faster keeps the feed it had.  Measured faster
// (1.1 - 3.3 %): 65536 x 65536, 131072 x 65536, 65536 x 200000, 131072 x 200000 - the four corners of the box below - and
// 98304 x 65536, 65536 x 131072, 131072 x 131072 inside it.  Measured slower, the image's launch (6 - 16 us) outweighing what
// the search gains: every shape of the 32x32 routing box with fewer than 65536 queries or train rows that was tried (8192 x
// 16384 .. 32768 x 65536, 65536 x 32768, 20000 x 100000), 49152 x 65536 and 40000 x 200000 excepted (0.4 % and 2.2 % faster),
// which stay outside: the rule is the box whose corners were measured.
static bool bf_mx_feed_auto(int64_t N, int64_t M) {
    return N >= 65536 && N <= 131072 && M >= 65536 && M <= 200000;
}

// The feed a pass of N x M takes on the 32x32x64 kernel under `feed` (0, 1 or 2), WITHOUT a device: *h_feed = 1 or 2.
extern "C" int slam_bf_mx_feed_describe(int feed, int64_t N, int64_t M, int32_t* h_feed) {
    SLAM_REQUIRE(h_feed, "slam_bf_mx_feed_describe: null argument");
    SLAM_REQUIRE(feed >= 0 && feed <= 2, "feed must be 0 (auto), 1 (expand in the kernel) or 2 (prepared image)");
    SLAM_REQUIRE(N >= 1 && M >= 1, "bad sizes");
    *h_feed = feed == 2 || (feed == 0 && bf_mx_feed_auto(N, M)) ? 2 : 1;
    return SLAM_OK;
}

extern "C" int slam_bf_set_mx_feed(slam_ctx* ctx, int feed) {
    SLAM_REQUIRE(ctx, "slam_bf_set_mx_feed: null ctx");
    SLAM_REQUIRE(feed >= 0 && feed <= 2, "feed must be 0 (auto), 1 (expand in the kernel) or 2 (prepared image)");
    std::lock_guard<std::mutex> g(ctx->mu);
    ctx->bf_mx_feed = feed;
    return SLAM_OK;
}

// The image buffer of the context, at least `bytes` long.  A member of its own and not slam_workspace: a forced engine with M
// above SLAM_MAX_TRAIN_PER_PASS runs passes while slam_bf_knn2_keep holds the workspace for its per-pass tables.  Grows behind
// a stream synchronisation, like bf_state_get (callers hold ctx->call_mu).  Never cached: every pass that reads it writes the
// whole of what it reads first, in stream order (callers overwrite train buffers in place).
static int bf_mx_image_get(slam_ctx* ctx, uint64_t bytes, void** out) {
    if (bytes > ctx->bf_mx_img_bytes) {
        SLAM_HIP(hipStreamSynchronize(ctx->stream));
        if (ctx->bf_mx_img) SLAM_HIP(hipFree(ctx->bf_mx_img));
        ctx->bf_mx_img = nullptr;
        ctx->bf_mx_img_bytes = 0;
        const uint64_t want = bytes + (bytes >> 2);               // headroom: slightly larger calls do not realloc
        SLAM_HIP(hipMalloc(&ctx->bf_mx_img, want));
        ctx->bf_mx_img_bytes = want;
    }
    *out = ctx->bf_mx_img;
    return SLAM_OK;
}

// Test hooks beside slam_ctx_block_bytes / slam_ctx_block_fill: the image buffer's current size, and the buffer filled with
// `byte` once the stream has drained (a buffer not yet taken is a no-op).
extern "C" int slam_bf_mx_image_bytes(slam_ctx* ctx, int64_t* h_bytes) {
    SLAM_REQUIRE(ctx && h_bytes, "slam_bf_mx_image_bytes: null argument");
    std::lock_guard<std::mutex> lk(ctx->call_mu);
    *h_bytes = (int64_t)ctx->bf_mx_img_bytes;
    return SLAM_OK;
}
extern "C" int slam_bf_mx_image_fill(slam_ctx* ctx, int byte) {
    SLAM_REQUIRE(ctx, "slam_bf_mx_image_fill: null ctx");
    std::lock_guard<std::mutex> lk(ctx->call_mu);
    SLAM_HIP(hipSetDevice(ctx->device));
    SLAM_HIP(hipStreamSynchronize(ctx->stream));
    if (!ctx->bf_mx_img || !ctx->bf_mx_img_bytes) return SLAM_OK;
    SLAM_HIP(hipMemsetAsync(ctx->bf_mx_img, byte, ctx->bf_mx_img_bytes, ctx->stream));
    SLAM_HIP(hipStreamSynchronize(ctx->stream));
    return SLAM_OK;
}

// ---- pinned train sets ----------------------------------------------------
// A caller that holds a train set fixed says so (slam_bf_train_pin), and the image is then built once per train set and not
// once per search: DESIGN.md 3c "Pinned train sets".  Nothing is cached for a buffer that is not pinned.

// The feed of the 32x32x64 kernel under feed 0 for a pinned train set with an image: the image costs such a search no launch, so
// the box is bf_mx_feed_auto's, widened.  Measured like it (tools/ab_time.py parent,lib:pin=1 --check, 5 rounds x 30 launches,
// the whole range below the parent's; profiles/mx_pin_ab.log, table in DESIGN.md 3c "Pinned train sets"): a shape that is not
// faster from the pinned image keeps feed 1.  Measured faster (1.8 - 3.4 %): the new corners 40000 x 32768, 131072 x 32768 and
// 40000 x 200000, and 40000 x 65536, 49152 x 65536, 65536 x 32768, 65535 x 65536 inside; 65536 x 65535 in two sessions of
// three (ranges 0.14 us into each other in the third).  Not faster by that rule: every shape tried with fewer than 20000
// queries (8192 x 16384 .. 500 x 200000: level or 0.3 - 1.3 us slower, the image is four times the bytes and few query blocks
// share them) and 32768 x 65536 (median 1.2 - 1.6 % faster, ranges overlap in both sessions).  20000 x 32768 .. 200000
// measured faster too (1.0 - 2.8 %) and stay outside with 32768 x 65536 between them and the box: the rule is the box whose
// corners were measured and that adds no shape that failed twice.
static bool bf_mx_feed_pinned(int64_t N, int64_t M) {
    return N >= 40000 && N <= 131072 && M >= 32768 && M <= 200000;
}
// Whether some N takes the image of a pinned set of M rows under feed 0: the M range of bf_mx_feed_pinned
static bool bf_mx_feed_pinned_rows(int64_t M) {
    return M >= 32768 && M <= 200000;
}

// The feed a pass of N x M takes on the 32x32x64 kernel under `feed` (0, 1 or 2) when its train set is pinned, WITHOUT a device.
extern "C" int slam_bf_mx_feed_describe_pinned(int feed, int64_t N, int64_t M, int32_t* h_feed) {
    SLAM_REQUIRE(h_feed, "slam_bf_mx_feed_describe_pinned: null argument");
    SLAM_REQUIRE(feed >= 0 && feed <= 2, "feed must be 0 (auto), 1 (expand in the kernel) or 2 (prepared image)");
    SLAM_REQUIRE(N >= 1 && M >= 1, "bad sizes");
    *h_feed = feed == 2 || (feed == 0 && bf_mx_feed_pinned(N, M)) ? 2 : 1;
    return SLAM_OK;
}

static int64_t bf_mx_image_rows(int64_t M) { return (M + SLAM_MX_STAGE - 1) / SLAM_MX_STAGE * SLAM_MX_STAGE; }

// bf_mx_image_kernel of M train rows into img (whole stages), on the context's stream; callers hold ctx->call_mu
static int bf_mx_image_launch(slam_ctx* ctx, const void* d_train, int64_t M, void* img) {
    const int64_t rows = bf_mx_image_rows(M);
    bf_mx_image_kernel<<<dim3((unsigned)(rows * 2 / 256)), dim3(256), 0, ctx->stream>>>((const u32*)d_train, (int)M, (uint4*)img,
                                                                                        (int)rows);
    if (int rc = slam_launch_check("train image kernel")) return rc;
    ctx->bf_mx_img_launches++;
    return SLAM_OK;
}

// the registration of exactly (d_train, M), or null; callers hold ctx->call_mu
static bf_train_pin* bf_train_pin_find(slam_ctx* ctx, const void* d_train, int64_t M) {
    for (bf_train_pin& p : ctx->bf_pin)
        if (p.rows == d_train && p.M == M) return &p;
    return nullptr;
}

// Frees the slot's image behind a stream synchronisation (queued searches may still read it) and clears the slot
static int bf_train_pin_drop(slam_ctx* ctx, bf_train_pin* p) {
    if (p->img) {
        SLAM_HIP(hipStreamSynchronize(ctx->stream));
        SLAM_HIP(hipFree(p->img));
    }
    *p = bf_train_pin();
    return SLAM_OK;
}

extern "C" int slam_bf_train_pin(slam_ctx* ctx, const void* d_train, int64_t M) {
    SLAM_REQUIRE(ctx && d_train, "slam_bf_train_pin: null argument");
    SLAM_REQUIRE(M >= 1 && M <= (1ll << 40), "slam_bf_train_pin: bad size");
    int feed;
    {
        // slam_free drops a registration by the allocation it lies in, so the rows must lie in one of this context
        std::lock_guard<std::mutex> g(ctx->mu);
        feed = ctx->bf_mx_feed;
        bool owned = false;
        const uintptr_t a = (uintptr_t)d_train, b = a + (uint64_t)M * 32;
        for (const auto& kv : ctx->allocs)
            owned = owned || ((uintptr_t)kv.first <= a && b <= (uintptr_t)kv.first + (kv.second ? kv.second : 16));
        SLAM_REQUIRE(owned, "slam_bf_train_pin: rows %p .. + 32 x %lld are not inside one slam_malloc allocation of this context", d_train,
                     (long long)M);
    }
    std::lock_guard<std::mutex> lk(ctx->call_mu);
    SLAM_HIP(hipSetDevice(ctx->device));
    bf_train_pin* slot = nullptr;
    for (bf_train_pin& p : ctx->bf_pin)
        if (p.rows == d_train) slot = &p;                        // pinned already: the new registration replaces it
    if (slot) {
        if (int rc = bf_train_pin_drop(ctx, slot)) return rc;
    } else {
        for (bf_train_pin& p : ctx->bf_pin)
            if (!p.rows && !slot) slot = &p;
        SLAM_REQUIRE(slot, "slam_bf_train_pin: this context already holds %d pinned train sets; unpin one first", SLAM_BF_PINS);
    }
    void* img = nullptr;
    if (M <= SLAM_MAX_TRAIN_PER_PASS && (feed == 2 || bf_mx_feed_pinned_rows(M))) {
        SLAM_HIP(hipMalloc(&img, (uint64_t)bf_mx_image_rows(M) * SLAM_MX_IMAGE_ROW_BYTES));
        if (int rc = bf_mx_image_launch(ctx, d_train, M, img)) {
            (void)hipFree(img);
            return rc;
        }
    }
    slot->rows = d_train;
    slot->M = M;
    slot->img = img;
    return SLAM_OK;
}

extern "C" int slam_bf_train_refresh(slam_ctx* ctx, const void* d_train) {
    SLAM_REQUIRE(ctx && d_train, "slam_bf_train_refresh: null argument");
    std::lock_guard<std::mutex> lk(ctx->call_mu);
    SLAM_HIP(hipSetDevice(ctx->device));
    for (bf_train_pin& p : ctx->bf_pin)
        if (p.rows == d_train) return p.img ? bf_mx_image_launch(ctx, p.rows, p.M, p.img) : SLAM_OK;
    return slam_set_error(SLAM_ERR_INVALID, "slam_bf_train_refresh: %p is not a pinned train set of this context", d_train);
}

extern "C" int slam_bf_train_unpin(slam_ctx* ctx, const void* d_train) {
    SLAM_REQUIRE(ctx && d_train, "slam_bf_train_unpin: null argument");
    std::lock_guard<std::mutex> lk(ctx->call_mu);
    SLAM_HIP(hipSetDevice(ctx->device));
    for (bf_train_pin& p : ctx->bf_pin)
        if (p.rows == d_train) return bf_train_pin_drop(ctx, &p);
    return slam_set_error(SLAM_ERR_INVALID, "slam_bf_train_unpin: %p is not a pinned train set of this context", d_train);
}

void bf_train_unpin_range(slam_ctx* ctx, const void* d_ptr, uint64_t bytes, std::vector<void*>* imgs) {
    std::lock_guard<std::mutex> lk(ctx->call_mu);
    const uintptr_t a = (uintptr_t)d_ptr, b = a + bytes;
    for (bf_train_pin& p : ctx->bf_pin) {
        if (!p.rows || (uintptr_t)p.rows >= b || (uintptr_t)p.rows + (uint64_t)p.M * 32 <= a) continue;
        if (p.img) imgs->push_back(p.img);
        p = bf_train_pin();
    }
}

// Test hooks: the image-kernel launches this context has issued (searches of unpinned sets, pins and refreshes), and the
// train sets it holds pinned.
extern "C" int slam_bf_mx_image_launches(slam_ctx* ctx, int64_t* h_count) {
    SLAM_REQUIRE(ctx && h_count, "slam_bf_mx_image_launches: null argument");
    std::lock_guard<std::mutex> lk(ctx->call_mu);
    *h_count = ctx->bf_mx_img_launches;
    return SLAM_OK;
}
extern "C" int slam_bf_train_pins(slam_ctx* ctx, int64_t* h_count) {
    SLAM_REQUIRE(ctx && h_count, "slam_bf_train_pins: null argument");
    std::lock_guard<std::mutex> lk(ctx->call_mu);
    int64_t n = 0;
    for (const bf_train_pin& p : ctx->bf_pin) n += p.rows ? 1 : 0;
    *h_count = n;
    return SLAM_OK;
}

extern "C" int slam_bf_set_engine(slam_ctx* ctx, int engine) {
    SLAM_REQUIRE(ctx, "slam_bf_set_engine: null ctx");
    SLAM_REQUIRE(engine >= 0 && engine <= 3,
                 "engine must be 0 (auto), 1 (VALU), 2 (16x16 matrix-core kernel where eligible) or 3 (32x32 matrix-core kernel where eligible)");
    std::lock_guard<std::mutex> g(ctx->mu);
    ctx->bf_engine = engine;
    return SLAM_OK;
}

// Whether a single search pass of N x M runs on the matrix cores: one query per lane, train rows in device memory, every tuning
// knob at its shipped value (a forced knob describes a VALU plan), and the engine says so.
bool bf_mx_route(slam_ctx* ctx, int64_t N, int64_t M, bool rows_on_host) {
    std::lock_guard<std::mutex> g(ctx->mu);
    if (ctx->bf_engine == 1 || rows_on_host) return false;
    for (int i = 0; i < SLAM_BF_KNOBS; i++)
        if (ctx->bf_knob[i]) return false;
    return ctx->bf_engine == 2 || ctx->bf_engine == 3 || bf_mx_auto(N, M);
}

int bf_mx_pass(slam_ctx* ctx, const void* d_query, int64_t N, const void* d_train, int64_t M, int64_t train_base, int32_t* d_idx,
               int32_t* d_dist, void* d_keep, const bf_select& sel, int* qblocks_out) {
    int num_cu, engine, feed;
    {
        std::lock_guard<std::mutex> g(ctx->mu);
        num_cu = ctx->num_cu;
        engine = ctx->bf_engine;
        feed = ctx->bf_mx_feed;
    }
    const bool wide = engine == 3 || (engine == 0 && bf_mx32_auto(N, M));     // the 32x32x64 kernel
    // a train set pinned as exactly (d_train, M) brings its image along: such a pass takes it by the pinned rule, with no launch
    const bf_train_pin* pin = wide ? bf_train_pin_find(ctx, d_train, M) : nullptr;
    const bool pinned = pin && pin->img && (feed == 2 || (feed == 0 && bf_mx_feed_pinned(N, M)));
    const bool image = pinned || (wide && (feed == 2 || (feed == 0 && bf_mx_feed_auto(N, M))));   // ... fed from the prepared image
    const auto kernel = image ? bf_mx32_image_top2_kernel : wide ? bf_top2_mx32_kernel : bf_top2_mx_kernel;
    const int which = image ? 2 : wide ? 1 : 0;
    static std::atomic<int> occ_once[3] = {{0}, {0}, {0}};   // a property of the kernel and the architecture: asked once per process
    int occ = occ_once[which].load(std::memory_order_relaxed);
    if (!occ) {
        int o = 0;
        SLAM_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&o, kernel, 256, 0));
        occ = o > 0 ? o : SLAM_MX_RESIDENT;
        occ_once[which].store(occ, std::memory_order_relaxed);
    }
    std::vector<int> tbl;
    const bf_mx_plan p = make_mx_plan_core(num_cu, occ, N, M, &tbl);
    bf_state st;
    if (int rc = bf_state_get(ctx, N, &st)) return rc;
    const int* d_tbl = nullptr;
    if (int rc = bf_table_get(ctx, tbl, &d_tbl)) return rc;
    if (qblocks_out) *qblocks_out = p.qblocks;
    SLAM_HIP(hipGetLastError());
    const void* d_rows = d_train;
    if (image) {
        // a stage of the image kernel is one 16 KiB block of the image: every stage, hence every chunk, starts on a whole stage
        for (size_t i = 0; i + 1 < tbl.size(); i++)
            SLAM_REQUIRE(tbl[i] % SLAM_MX_STAGE == 0, "MX plan: chunk %zu starts at row %d, not a multiple of the stage", i, tbl[i]);
        void* img = pinned ? pin->img : nullptr;
        if (!pinned) {
            if (int rc = bf_mx_image_get(ctx, (uint64_t)bf_mx_image_rows(M) * SLAM_MX_IMAGE_ROW_BYTES, &img)) return rc;
            if (int rc = bf_mx_image_launch(ctx, d_train, M, img)) return rc;
        }
        d_rows = img;
    }
    if (int rc = slam_prof_begin(ctx)) return rc;
    kernel<<<dim3(p.qblocks, p.workers), dim3(256), 0, ctx->stream>>>(
        (const uint4*)d_query, (int)N, (const uint4*)d_rows, d_tbl, st, (int)train_base, (int2*)d_idx, (int2*)d_dist,
        (uint4*)d_keep, p.S, sel);
    if (int rc = slam_prof_end(ctx)) return rc;
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        (void)bf_state_reset(ctx);
        return slam_set_error(SLAM_ERR_HIP, "top-2 MX kernel launch failed: %s", hipGetErrorString(e));
    }
    return SLAM_OK;
}
