// bf_mx32.hip — the matrix-core top-2 Hamming search of bf_mx.hip on 32x32x64 FP4 tiles.  Same results as bf_top2_kernel
// (bf_hamming.hip) and as bf_top2_mx_kernel, bit for bit; see DESIGN.md §3c "The 32x32x64 kernel".
//
//   * why: the kernel of bf_mx.hip is bound by vector issue, and half of its issue floor is the hold of its MFMA instructions
//     (12.4 cycles each, paid per instruction, not per MAC).  v_mfma_f32_32x32x64_f8f6f4 does twice the MACs per instruction in
//     twice the cycles, and in the UNSCALED spelling (both scale operands of the builtin the constant 0) holds the vector issue
//     for 8.2 of its 32 cycles (tools/ubench/mx_issue.hip): a group-equivalent is 4 instructions, not 8, and up to five plain
//     vector instructions per MFMA issue in its shadow.
//   * encoding: as bf_mx.hip - descriptor bit 1 -> FP4 -1.0, bit 0 -> +1.0, hamming(a, b) = (256 - <a+-, b+->) / 2, every
//     partial sum an exact integer in f32.  mx_expand (bf_mx_common.h, the one copy) turns one 32-bit source word into the 16
//     bytes a lane holds of one operand: for K-quarter q (64 bits) of a row, lane (row & 31) + 32 hk holds source word 2 q + hk.
//     The query rows use the same map, so which bit meets which K position does not matter.
//   * geometry: a wave holds its 64 queries as the B operands of two 32-query tiles (4 K-quarters x 4 VGPRs each: 32 VGPRs,
//     expanded once).  A group is 32 train rows: 8 MFMAs, 2 tiles x 4 K-quarters, the first quarter with C = inline 0, the rest
//     accumulating in place in VGPRs (16 per tile; the Makefile's -amdgpu-mfma-vgpr-form for this file).  Lane l holds query
//     (l & 31) of the tile; its accumulator index 4 i + j is row 8 i + 4 (l >> 5) + j of the group (tests/test_mx32_gpu.py
//     proves the map with planted pairs at every distance).  A lane's rows ascend with the accumulator index.
//   * LDS stage: 128 rows as in bf_mx.hip, double buffered, one barrier per stage; a group of 32 rows is [K-quarter][lane] x
//     16 bytes, so an operand is one conflict-free ds_read_b128.  Thread tid stages half (tid & 1) of row (tid >> 1): its four
//     source words are the pieces of K-quarters 2 (tid & 1) and 2 (tid & 1) + 1.
//   * selection: the accumulators hold the bare dot D = 256 - 2 dist.  A lane keeps, per tile, the EXCLUSIVE threshold distance x
//     (a row passes when its distance is below x) and the bit pattern of the float 258 - 2 x beside it; the 16 results of a tile
//     fold as bit patterns with eight signed-integer maxima - a tree: the maxima of five row groups, then their maximum - and
//     one compare against that pattern.  Dots are exact integers and never -0, so for 258 - 2 x >= 0 (x <= 129) the signed comparison of patterns is the comparison of the values: negative
//     floats are negative integers, below every pattern of a value >= 0.  A signed maximum orders negative floats backwards, so
//     for x > 129 (a worker's first groups, or rows that are all far) the pattern is INT_MIN and the tile fires unconditionally:
//     the update path is exact whatever passes, since a key is built from D alone, key = (128 << 23 | row) - (D << 22).
//     The compare is per tile, so the fire test per tile is free, and a threshold move is one conversion.
//   * the tie rules of bf_mx.hip's header carry over unchanged, with two lanes per query where that kernel has four.  x only
//     ever falls, to one of:
//       - dist(own 2nd-best) after a fire, dist(2nd-best of the query's two lanes) at a chunk start and at an early exchange
//         (not at a stage end: that union spared 2 % of the fires and stood in front of every other barrier): chunks, stages,
//         groups and a lane's rows ascend, so every row the lane has still to see has a higher index than every row in those
//         pairs, and a tie against them loses;
//       - mx_bound_x(g, c0) for the key g read from bound[] at the start of the chunk that begins at row c0 (the row of g is
//         TESTED against c0: a tie against a key from a later row can win), and the same with the first row of the stage to come
//         at the early exchanges (SLAM_MX_EARLY).  bound[] holds 2nd-best keys below SLAM_MX_BOUND_LIMIT, as in bf_mx.hip.
//     A candidate is dropped only if some known 2nd-best key K has dist(K) < dist, or dist(K) == dist and row(K) < row.
//   * row gates: a fired tile tests ROW GROUPS, a partition of the accumulator indices 0 .. 15 (MX32_GATES groups, below): a
//     group's gate is "some lane of the tile has max(acc[i], i in the group) >= its pattern".  The group maxima are the first
//     level of the fold's tree, so the quiet fold keeps its eight maxima and one compare.  The group compares are issued back
//     to back into SGPR pairs, the wave-uniform branches test those on the scalar side (no branch waits on the compare in front
//     of it), and of an open group ALL rows are keyed and merged, with no inner branch.  Why this is the search it was:
//       - a group gate is open exactly when some row of the group passes in some lane, so a row that does not enter is below
//         the threshold of every lane of the tile, and the rows that enter are a superset of those the 16 row gates let in;
//       - the update path is exact whatever passes (selection, above): a lane's 2nd-best can only be nearer for the extra rows,
//         so its threshold is only tighter, and every key published to bound[] is still a real row's key;
//       - every row that enters lies below every row the lane has still to see, so the exclusive-threshold tie rule holds;
//       - every gate is evaluated against the threshold as it stood at the fold; the threshold moves only behind the rows;
//       - the short last stage keeps its test against c1 on every key it builds: a row past the end never enters.
//     The final tables are those of the full sort either way, bit for bit (tests/test_mx32_gates_cpu.py replays both).
//   * scan loop: a whole stage is one trip of four groups in which a tile's four MFMAs run together and the folds stand between
//     the runs: t0k0 .. t0k3 [fold of tile 1, previous group] t1k0 .. t1k3 [fold of tile 0].  A tile's fold, and its update path
//     where it fires, stands behind four MFMAs of the OTHER tile and behind the other tile's fold, so the wave keeps the matrix
//     pipe fed while it folds and the compiler owes no wait states in front of a fold (a vector read of an MFMA result is not
//     interlocked: 11 states after the MFMA).  Each tile sees its own MFMAs, fold and update in the order they always had;
//     the tiles share nothing.  The A operand of K-quarter q of group g + 1 is read once tile 1's MFMA of
//     quarter q of group g has issued, into the registers it frees, three MFMAs ahead of its use.  A stage that another follows
//     expands and stores the thread's four source words of the next stage (ONE 16-byte load at the trip's start) in groups 1 to
//     3, between MFMAs.  The last stage of the train set, if short, runs group by group, both folds behind the eight MFMAs, with
//     the test for rows past the chunk.
//   * plan, tickets, bound exchange, epilogue: those of bf_top2_mx_kernel; bf_mx.hip plans and launches both kernels.
//   * two feeds (slam_bf_set_mx_feed; DESIGN.md 3c "Feed"): the kernel's text is bf_mx32_scan.inc, included twice.
//     bf_top2_mx32_kernel stages as described above.  bf_mx32_image_top2_kernel reads an image of the train set that
//     bf_mx_image_kernel (below) expands once per search into the exact bytes of the LDS stages, and stages with four
//     direct-to-LDS copies per thread (mx32_copy_stage): no expand, no ds_write, nothing else differs.
#include "internal.h"
#include <type_traits>

#include "bf_common.h"
#include "bf_mx_common.h"

typedef float mx_v16f __attribute__((ext_vector_type(16)));

// The phase probe (tools/mx_phase_probe.py; MX_STAMP and the phases are in bf_mx_common.h): this kernel's buffer
#ifdef SLAM_MX_PROBE
__device__ unsigned long long* g_mx32_probe = nullptr;
extern "C" __attribute__((visibility("default"))) int slam_exp_set_mx32_probe(void* p) {
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_mx32_probe), &p, sizeof(p));
}
#endif

// c + A B over one K-quarter: A = 32 train rows, B = 32 queries, FP4 on both sides (format code 4).  Both scale operands are the
// constant 0: the compiler then selects the unscaled v_mfma_f32_32x32x64_f8f6f4, which holds the vector issue for a shorter time
__device__ __forceinline__ mx_v16f mx32_dot(uint4 a, uint4 b, mx_v16f c) {
    const mx_v8i av = {(int)a.x, (int)a.y, (int)a.z, (int)a.w, 0, 0, 0, 0};
    const mx_v8i bv = {(int)b.x, (int)b.y, (int)b.z, (int)b.w, 0, 0, 0, 0};
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, c, 4, 4, 0, 0, 0, 0);
}

#define MX32_GROUP 32                                  // train rows per group
#define MX32_GROUPS (SLAM_MX_STAGE / MX32_GROUP)       // groups per whole stage

// The gate groups of a fired tile: a partition of the accumulator indices 0 .. 15 whose maxima are the first level of the
// fold's tree.  Group 0 = {0, 1, 14, 15}, group j = 1 .. 4 = {3 j - 1, 3 j, 3 j + 1}
#define MX32_GATES 5
constexpr int mx32_gate_rows(int j) { return j ? 3 : 4; }
constexpr int mx32_gate_index(int j, int r) { return j ? 3 * j - 1 + r : (r < 2 ? r : 12 + r); }

// One 16 KiB stage of the prepared image straight from device memory into LDS: four global_load_lds_dwordx4 per thread, piece
// j = bytes 4096 j .. of the stage, there (scalar base src + 4096 j, plus the thread's fixed offset voff = 16 tid) and here
// (M0 = lds + 4096 j, wave-uniform: the wave's lane l writes M0 + 16 l, so lds is the stage buffer + 1024 wave).  No vector ALU
// work and no register holds the bytes.  Written as one asm statement because the compiler, which counts a direct-to-LDS load
// it knows of against every later ds_read, drains it (vmcnt(0)) in front of the trip's first operand read; this way the copies
// stay in flight behind the whole trip.  The compiler therefore does not count them: the caller waits (mx32_copies_done) in
// front of the barrier that hands the buffer to its readers, and until then the buffer is read by nobody.  M0 is saved and
// restored inside the statement (the compiler keeps it for itself); one wait state between a write of M0 and its use.
__device__ __forceinline__ void mx32_copy_stage(const uint4* src, u32 voff, u32 lds) {
    const char* p = (const char*)src;
    u32 keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %6\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\t"
        "s_add_u32 m0, m0, 0x1000\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\t"
        "s_add_u32 m0, m0, 0x1000\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %4\n\t"
        "s_add_u32 m0, m0, 0x1000\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %5\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff), "s"(p), "s"(p + 4096), "s"(p + 8192), "s"(p + 12288), "s"(lds)
        : "memory", "scc");
}
__device__ __forceinline__ void mx32_copies_done() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// The shipped kernel, then the same search fed from the prepared image (t is the image), under a name of its own: the
// listing tests of the shipped kernel find theirs by prefix
#define MX32_KERNEL bf_top2_mx32_kernel
#define MX32_IMAGE_FEED 0
#include "bf_mx32_scan.inc"
#undef MX32_KERNEL
#undef MX32_IMAGE_FEED
#define MX32_KERNEL bf_mx32_image_top2_kernel
#define MX32_IMAGE_FEED 1
#include "bf_mx32_scan.inc"
#undef MX32_KERNEL
#undef MX32_IMAGE_FEED

// The prepared image: the M compact train rows expanded once, in the order of an LDS stage of the search - group of 32 rows =
// [K-quarter][lane] x 16 bytes (4 KiB), groups consecutive, so the stage that begins at a multiple of 128 rows is one block of
// 16 KiB.  Thread i carries half (i & 1) of row (i >> 1), one 16-byte load, as a thread of the in-kernel feed does: source word
// 4 sh + j is the piece of K-quarter 2 sh + (j >> 1), lane (row & 31) + 32 (j & 1), of the row's group - the map of store_word
// / dst0.  Rows from M up to `rows` (M rounded up to whole stages) are written as the row of zero bits, which is what the
// in-kernel feed stores there: every launch writes the whole of what its search can read.
__global__ __launch_bounds__(256) void bf_mx_image_kernel(const u32* __restrict__ t, int M, uint4* __restrict__ img, int rows) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    const int row = i >> 1, sh = i & 1;
    if (row >= rows) return;
    const uint4 v = row < M ? ((const uint4*)t)[i] : make_uint4(0, 0, 0, 0);
    uint4* dst = img + (size_t)(row >> 5) * 256 + sh * 128 + (row & 31);
    dst[0] = mx_expand(v.x);
    dst[32] = mx_expand(v.y);
    dst[64] = mx_expand(v.z);
    dst[96] = mx_expand(v.w);
}
