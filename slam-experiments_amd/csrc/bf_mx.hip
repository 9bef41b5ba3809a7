// bf_mx.hip — the top-2 Hamming search of large searches on the MATRIX cores of gfx950 (MI355X), as a dot product of
// +-1 vectors in FP4.  Same results as bf_top2_kernel (bf_hamming.hip), bit for bit; see DESIGN.md §3c.
//
//   * encoding: descriptor bit 1 -> FP4 (E2M1) +1.0 (nibble 0x2), bit 0 -> -1.0 (nibble 0xA).  For 256-bit rows a, b:
//         hamming(a, b) = (256 - <a+-, b+->) / 2
//     Every product is +-1 and every partial sum an integer of magnitude <= 256 + 1022 (the threshold rides in the
//     accumulator, below): the f32 accumulator is exact.  Which bit goes to which K position does not matter as long as
//     both operands use the same map: mx_expand spreads bit 4n + w of a 32-bit word to nibble n of output word w (one
//     shift and one v_and_or per output word).
//   * v_mfma_scale_f32_16x16x128_f8f6f4 with FP4 on both sides (cbsz:4 blgp:4, scale 2^0): D[16 train rows][16 queries]
//     over K = 128 bits; two of them per 256-bit pair.  A wave holds 64 queries as the B operands of four 16-query tiles
//     (2 K-halves x 4 VGPRs each: 32 VGPRs, expanded once from the 32-byte rows); per 16 train rows it issues 8 MFMAs.
//   * train rows reach the A operand through an LDS stage shared by the block's four waves: the block loads 128 compact
//     rows (4 KiB, one 16-byte load per thread), expands them (8 VALU per word) straight into the operand order - group
//     of 16 rows = [K-half][lane] x 16 bytes, so a lane's operand is one conflict-free ds_read_b128 - double buffered,
//     one barrier per stage.  The compact train set (2 MiB at 65536 rows) stays what sits in the L2s.
//   * selection: the accumulator starts at C = 2 d2 - 256 (d2: the query's current 2nd-best distance), so D >= 0 <=>
//     distance <= d2 - ties pass, the keys decide (rows of one query reach different lanes out of index order).  Lane
//     (lane & 15, lane >> 4) of tile t holds query 16 t + (lane & 15) against rows 4 (lane >> 4) + r: the 16 results of a
//     group fold as bit patterns with v_max3_i32 (exact integers: the sign of the signed maximum says "some D >= 0") into
//     one compare and one branch; the update (laid out as unlikely) runs per tile, only for tiles whose own maximum passes,
//     and is the VALU kernel's on packed keys (dist << 23 | row: med3 / min).  The accumulators and C live in VGPRs (the
//     Makefile's -amdgpu-mfma-vgpr-form for this file): no AGPR round trip.  Each lane keeps the top-2 of ITS rows; the four
//     lanes of a query are united (two xor shuffles) once per stage that fired for the threshold, at each chunk start for the
//     bound exchange, and at the end, where lane l takes query 64 wave + l - the layout of bf_top2_kernel's epilogue, shared.
//   * plan: the queue plan of bf_top2_kernel<1, true, true> with tickets drawn per BLOCK: grid = (query blocks, workers),
//     the workers of a query block draw chunks of the boundary table by ticket, exchange the 2nd-best distance through
//     bound[] at every chunk, merge with the two returning atomic minima and the last arriver decodes (bf_common.h).
#include "internal.h"
#include <vector>
#include <atomic>

#include "bf_common.h"

#define SLAM_MX_STAGE 128        // train rows per LDS stage: 16 KiB expanded, two stages per block
#define SLAM_MX_RESIDENT 4       // blocks of bf_top2_mx_kernel a CU holds at once (the plan describe counts on it; launches ask)

typedef int mx_v8i __attribute__((ext_vector_type(8)));
typedef float mx_v4f __attribute__((ext_vector_type(4)));

// 32 descriptor bits -> 32 FP4 elements (+1.0 for a set bit, -1.0 for a clear one): nibble n of word w = bit 4n + w
__device__ __forceinline__ uint4 mx_expand(u32 x) {
    const u32 n = ~x;
    uint4 r;
    r.x = ((n << 3) & 0x88888888u) | 0x22222222u;
    r.y = ((n << 2) & 0x88888888u) | 0x22222222u;
    r.z = ((n << 1) & 0x88888888u) | 0x22222222u;
    r.w = (n & 0x88888888u) | 0x22222222u;
    return r;
}

// c + A B over one K-half: A = 16 train rows, B = 16 queries, FP4 on both sides (format code 4), scales 2^0 (E8M0 127)
__device__ __forceinline__ mx_v4f mx_dot(uint4 a, uint4 b, mx_v4f c) {
    const mx_v8i av = {(int)a.x, (int)a.y, (int)a.z, (int)a.w, 0, 0, 0, 0};
    const mx_v8i bv = {(int)b.x, (int)b.y, (int)b.z, (int)b.w, 0, 0, 0, 0};
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bv, c, 4, 4, 0, 127, 0, 127);
}

// top-2 of two top-2 pairs whose keys are distinct rows (or none)
__device__ __forceinline__ void mx_unite(u32& b1, u32& b2, u32 c1, u32 c2) {
    const u32 n2 = min(max(b1, c1), min(b2, c2));
    b1 = min(b1, c1);
    b2 = n2;
}

__device__ __forceinline__ u32 mx_pick(const u32 (&v)[4], int i) {
    return i == 0 ? v[0] : (i == 1 ? v[1] : (i == 2 ? v[2] : v[3]));
}

// grid = (query blocks, workers).  Block (x, y) works for query block (x + y) mod grid.x: the workers of a query block are
// spread over the XCDs, as in the VALU queue plan.
__global__ __launch_bounds__(256) void bf_top2_mx_kernel(const uint4* __restrict__ q, int N, const uint4* __restrict__ t,
                                                         const int* __restrict__ tbl, bf_state st, int train_base,
                                                         int2* __restrict__ out_idx, int2* __restrict__ out_dist,
                                                         uint4* __restrict__ keep, int nchunks, bf_select sel) {
    __shared__ uint4 tile[2][SLAM_MX_STAGE * 8];
    __shared__ u32 s_ticket, s_last;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int kg = lane >> 4, col = lane & 15;
    const int bx = ((int)blockIdx.x + (int)blockIdx.y) % (int)gridDim.x;
    const int qbase = bx * 256 + wave * 64 + lane;              // the lane's query in the epilogue (and in the bound exchange)

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
    if (keep && blockIdx.y == 0 && qbase < N) {                  // the caller wants the query rows left in device memory
        keep[2 * (size_t)qbase] = q[2 * (size_t)qbase];
        keep[2 * (size_t)qbase + 1] = q[2 * (size_t)qbase + 1];
    }

    // per tile: the lane's own top-2 over its rows, the threshold distance d2 and the accumulator start 2 d2 - 256, and ub: the
    // best bound known from elsewhere (the query's other lanes, the other blocks); d2 = min(own 2nd-best, ub)
    u32 b1[4], b2[4], d2[4], ub[4];
    mx_v4f cth[4];
#pragma unroll
    for (int tt = 0; tt < 4; tt++) {
        b1[tt] = b2[tt] = SLAM_KEY_NONE;
        d2[tt] = ub[tt] = SLAM_KEY_NONE >> SLAM_KEY_IDX_BITS;
        const float c = (float)(2 * (int)d2[tt] - 256);
        cth[tt] = mx_v4f{c, c, c, c};
    }
    auto set_threshold = [&](int tt) {
        d2[tt] = min(ub[tt], b2[tt] >> SLAM_KEY_IDX_BITS);
        const float c = (float)(2 * (int)d2[tt] - 256);
        cth[tt] = mx_v4f{c, c, c, c};
    };
    // the top-2 of each tile's query over the rows of all four lanes that hold it (ds_bpermute: it issues beside the VALU, which
    // is what bounds this kernel; the v_permlane16/32_swap form costs two copies and a wait per swap there and measured slower)
    auto unite_lanes = [&](u32 (&u1)[4], u32 (&u2)[4]) {
#pragma unroll
        for (int tt = 0; tt < 4; tt++) {
            u1[tt] = b1[tt];
            u2[tt] = b2[tt];
#pragma unroll
            for (int off = 16; off <= 32; off <<= 1) {
                const u32 c1 = (u32)__shfl_xor((int)u1[tt], off, 64), c2 = (u32)__shfl_xor((int)u2[tt], off, 64);
                mx_unite(u1[tt], u2[tt], c1, c2);
            }
        }
    };
    // exchange with the other workers of this query block through bound[] (share_bound; lane l speaks for query 64 wave + l)
    u32 gk[1] = {SLAM_BOUND_IDLE}, pend[1] = {0u};
    auto exchange = [&]() {
        u32 u1[4], u2[4];
        unite_lanes(u1, u2);
        u32 own[1] = {mx_pick(u2, kg)}, init[1];
        share_bound<1>(st.bound, qbase, N, own, init, gk, pend);
#pragma unroll
        for (int tt = 0; tt < 4; tt++) {
            const u32 g = (u32)__shfl((int)gk[0], tt * 16 + col, 64);
            ub[tt] = min(ub[tt], min(g, u2[tt] >> SLAM_KEY_IDX_BITS));
            set_threshold(tt);
        }
    };

    // staging: thread tid carries half (tid & 1) of row (tid >> 1) of a stage, i.e. the source words 4 h .. 4 h + 3, which
    // become the operand words of lanes 16 g + (row & 15), g = 0..3, of K-half h in the row's group of 16
    const int srow = tid >> 1, sh = tid & 1;
    auto load_stage = [&](int s, int c1) -> uint4 {
        const int row = s + srow;
        return row < c1 ? t[2 * (size_t)row + sh] : make_uint4(0, 0, 0, 0);
    };
    auto store_stage = [&](int b, uint4 v) {
        uint4* dst = tile[b] + (srow >> 4) * 128 + sh * 64 + (srow & 15);
        dst[0] = mx_expand(v.x);
        dst[16] = mx_expand(v.y);
        dst[32] = mx_expand(v.z);
        dst[48] = mx_expand(v.w);
    };

    u32* const cursor = st.cursor + (size_t)(4 * bx) * SLAM_CURSOR_STRIDE;
    if (tid == 0) s_ticket = __hip_atomic_fetch_add(cursor, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    int ci = __builtin_amdgcn_readfirstlane((int)s_ticket);
    while (ci < nchunks) {
        const int c0 = tbl[ci], c1 = tbl[ci + 1];
        uint4 nx = load_stage(c0, c1);
        exchange();
        store_stage(0, nx);
        __syncthreads();
        int buf = 0;
        for (int s0 = c0; s0 < c1; s0 += SLAM_MX_STAGE) {
            const int s1 = s0 + SLAM_MX_STAGE;
            const bool more = s1 < c1;
            if (more) nx = load_stage(s1, c1);
            // the next ticket is drawn while the chunk's last stage is scanned; read behind the stage's barrier
            else if (tid == 0) s_ticket = __hip_atomic_fetch_add(cursor, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int ng = __builtin_amdgcn_readfirstlane(min(SLAM_MX_STAGE / 16, (c1 - s0 + 15) >> 4));
            const uint4* tp = tile[buf];
            const int lim = s1 > c1 ? c1 : 0x7fffffff;           // rows past the chunk: only in the last stage of the last chunk
            bool fired = false;                                  // wave-uniform: some group of this stage took the update path
            for (int g = 0; g < ng; g++) {
                const uint4 a0 = tp[g * 128 + lane], a1 = tp[g * 128 + 64 + lane];
                mx_v4f acc[4];
#pragma unroll
                for (int tt = 0; tt < 4; tt++) acc[tt] = mx_dot(a0, qb[tt][0], cth[tt]);
#pragma unroll
                for (int tt = 0; tt < 4; tt++) acc[tt] = mx_dot(a1, qb[tt][1], acc[tt]);
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
                    // D = dot + 2 d2 - 256, so the distance (256 - dot) / 2 is d2 - D / 2 (D is even); rows past the chunk -
                    // the zero rows of a short stage - never enter.  Only the tiles that hold a candidate are updated (wave-
                    // uniform branches on the tile's own maximum), and only those get a new threshold
                    const int row0 = s0 + g * 16 + 4 * kg;
                    fired = true;
#pragma unroll
                    for (int tt = 0; tt < 4; tt++) {
                        if (__ballot(max(p[tt], __float_as_int(acc[tt][3])) >= 0) == 0ull) continue;
                        const u32 base = (d2[tt] << SLAM_KEY_IDX_BITS) + (u32)row0;
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            // key = (d2 - D / 2) << 23 | row, D even: base + r + (-D << 22)
                            u32 key = base + (u32)r + ((u32)(int)(-acc[tt][r]) << (SLAM_KEY_IDX_BITS - 1));
                            key = row0 + r < lim ? key : SLAM_KEY_NONE;
                            b2[tt] = umed3(b1[tt], b2[tt], key);
                            b1[tt] = min(b1[tt], key);
                        }
                        set_threshold(tt);
                    }
                }
            }
            if (fired) {   // once per stage in which a key changed: the threshold of the query's four lanes together
                u32 u1[4], u2[4];
                unite_lanes(u1, u2);
#pragma unroll
                for (int tt = 0; tt < 4; tt++) {
                    ub[tt] = min(ub[tt], u2[tt] >> SLAM_KEY_IDX_BITS);
                    set_threshold(tt);
                }
            }
            if (more) store_stage(buf ^ 1, nx);
            __syncthreads();
            buf ^= 1;
        }
        ci = __builtin_amdgcn_readfirstlane((int)s_ticket);
    }

    u32 u1[4], u2[4];
    unite_lanes(u1, u2);
    const u32 f1[1] = {mx_pick(u1, kg)}, f2[1] = {mx_pick(u2, kg)};
    bf_top2_epilogue<1, true>(st, bx, tid, lane, qbase, false, false, f1, f2, gk, pend, N, (int)gridDim.y, train_base, out_idx,
                              out_dist, sel, s_last);
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

extern "C" int slam_bf_set_engine(slam_ctx* ctx, int engine) {
    SLAM_REQUIRE(ctx, "slam_bf_set_engine: null ctx");
    SLAM_REQUIRE(engine >= 0 && engine <= 2, "engine must be 0 (auto), 1 (VALU) or 2 (matrix cores where eligible)");
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
    return ctx->bf_engine == 2 || bf_mx_auto(N, M);
}

int bf_mx_pass(slam_ctx* ctx, const void* d_query, int64_t N, const void* d_train, int64_t M, int64_t train_base, int32_t* d_idx,
               int32_t* d_dist, void* d_keep, const bf_select& sel, int* qblocks_out) {
    static std::atomic<int> occ_once{0};     // a property of the kernel and the architecture: asked once per process
    int occ = occ_once.load(std::memory_order_relaxed);
    if (!occ) {
        int o = 0;
        SLAM_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&o, bf_top2_mx_kernel, 256, 0));
        occ = o > 0 ? o : SLAM_MX_RESIDENT;
        occ_once.store(occ, std::memory_order_relaxed);
    }
    std::vector<int> tbl;
    int num_cu;
    {
        std::lock_guard<std::mutex> g(ctx->mu);
        num_cu = ctx->num_cu;
    }
    const bf_mx_plan p = make_mx_plan_core(num_cu, occ, N, M, &tbl);
    bf_state st;
    if (int rc = bf_state_get(ctx, N, &st)) return rc;
    const int* d_tbl = nullptr;
    if (int rc = bf_table_get(ctx, tbl, &d_tbl)) return rc;
    if (qblocks_out) *qblocks_out = p.qblocks;
    SLAM_HIP(hipGetLastError());
    if (int rc = slam_prof_begin(ctx)) return rc;
    bf_top2_mx_kernel<<<dim3(p.qblocks, p.workers), dim3(256), 0, ctx->stream>>>(
        (const uint4*)d_query, (int)N, (const uint4*)d_train, d_tbl, st, (int)train_base, (int2*)d_idx, (int2*)d_dist,
        (uint4*)d_keep, p.S, sel);
    if (int rc = slam_prof_end(ctx)) return rc;
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        (void)bf_state_reset(ctx);
        return slam_set_error(SLAM_ERR_HIP, "top-2 MX kernel launch failed: %s", hipGetErrorString(e));
    }
    return SLAM_OK;
}
