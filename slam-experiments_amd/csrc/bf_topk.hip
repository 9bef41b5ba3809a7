// bf_topk.hip — brute-force Hamming top-k (k <= 32) over 256-bit ORB descriptors on gfx950 (MI355X).  Replaces
// cv2.BFMatcher(NORM_HAMMING).knnMatch(query, train, k) for any k up to SLAM_BF_KNN_MAX: the several candidates per
// descriptor that keyframe voting over a KeyframeDatabase needs, where the top-2 search (bf_hamming.hip) stops at two.
//
// Design (DESIGN.md "Top-k search"), the top-2 search's where it carries over:
//   * one lane per query (R = 1), the query's 8 words in VGPRs; train rows staged global -> LDS in 256-row tiles (double
//     buffered) and read back as wave-uniform ds_read_b128; the 16-VALU row of row_acc<1> with its s_setprio pairing.
//   * each lane keeps its sorted top-K as packed keys dist << 23 | row (SLAM_KEY_IDX_BITS, the top-2's keys) in registers.
//     The kernel is instantiated for K = 4, 8, 16, 32; a requested k runs on the next instantiation up, with the first K - k
//     slots pinned to the key 0: an insertion passes through them unchanged (min(0, x) = 0, max(0, x) = x), so the list
//     proper is keys[K - k .. K - 1] and its k-th key is always keys[K - 1] - a fixed register, the filter's threshold.
//   * the biased-accumulator sign-bit filter of filter_update with one ballot per group of 16 rows; a group that fires
//     inserts its rows (those whose ballot is non-zero) with a branch-free compare-exchange sweep through the K keys,
//     2K VALU per row.  The first 128 rows of a chunk that starts before anybody has published a bound go in unfiltered.
//   * the train axis is split into chunks (grid = query blocks x chunks, one round of resident blocks); the blocks of a
//     query exchange their k-th distance through bound[] of the top-2's merge state (share_bound: returning atomicMin,
//     "+ 1 keeps ties").  Each block writes its sorted k keys to a partial table [chunks][N][k] in the context's
//     workspace; a second small kernel merges the lists of a query (a list is left at its first key that cannot enter),
//     decodes (idx + train_base, dist) and puts bound[] back to idle.  A search of one chunk writes its results directly.
//   * train sets larger than 2^23 rows run in passes into decoded per-pass tables, merged by bf_merge_topk_kernel.
#include "bf_common.h"
#include <atomic>

#define SLAM_TOPK_WS_CAP (64ull << 20)   // bytes of partial tables one search may use (fewer chunks beyond)
#define SLAM_TOPK_MIN_CHUNK 256          // rows: one LDS tile
#define SLAM_TOPK_PLAN 8                 // entries of slam_bf_topk_plan_describe's h_plan

static int topk_width(int k) { return k <= 4 ? 4 : k <= 8 ? 8 : k <= 16 ? 16 : 32; }
// Blocks of bf_topk_kernel<K> a CU holds at once: waves per SIMD by VGPRs (-Rpass-analysis=kernel-resource-usage; one
// 256-thread block is one wave per SIMD).  The planner counts on these; a device that holds fewer (the occupancy query)
// gets fewer chunks.
static int topk_resident(int K) { return K <= 4 ? 8 : K <= 8 ? 7 : K <= 16 ? 6 : 4; }

// Insert x into the ascending list keys[0 .. K-1], dropping the largest key: one min and one max per slot, no branch.
template <int K, typename T>
__device__ __forceinline__ void topk_insert(T (&keys)[K], T x) {
#pragma unroll
    for (int i = 0; i < K; i++) {
        const T lo = x < keys[i] ? x : keys[i];
        x = x < keys[i] ? keys[i] : x;
        keys[i] = lo;
    }
}

// filter_update with a top-K list: "some lane improved" is the sign bit of the AND of the group's 16 biased accumulators;
// a group that fires inserts the rows whose own ballot is non-zero (wave-uniform), then tightens the threshold to the
// lane's k-th distance (only tighten: init may hold a smaller bound learnt from other chunks).
template <int K, int U>
__device__ __forceinline__ void topk_filter_update(const u32 (&acc)[U][1], u32 first_train_idx, u32 (&keys)[K], u32 (&init)[1]) {
    u32 m = acc[0][0];
#pragma unroll
    for (int u = 1; u < U; u++) m &= acc[u][0];
    if (__builtin_expect(__ballot((int)m >= 0) != 0ull, 0)) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            if (U > 1 && __ballot((int)acc[u][0] >= 0) == 0ull) continue;
            topk_insert<K>(keys, ((acc[u][0] - init[0]) << SLAM_KEY_IDX_BITS) | (first_train_idx + u));
        }
        init[0] = max(init[0], SLAM_ACC_BIAS - (keys[K - 1] >> SLAM_KEY_IDX_BITS));
    }
}

struct topk_args {
    const uint4* q;     // [N] query rows (two uint4 each)
    const uint4* t;     // [M] train rows of this pass
    int N, M;
    int chunk;          // rows per chunk: block (x, y) scans rows [y * chunk, min(M, (y + 1) * chunk))
    int k;              // columns written (1 .. K)
    int train_base;     // added to every decoded index
    int cold;           // rows folded in unfiltered at a cold chunk start (a multiple of 16)
    u32* bound;         // [N] per-query bound (bf_state); null: one chunk, nothing to exchange
    u32* part;          // [chunks][N][k] sorted keys; null: one chunk, the decoded results go to idx / dist
    int32_t* idx;       // [N][k]
    int32_t* dist;      // [N][k]
};

template <int K>
__global__ __launch_bounds__(256) void bf_topk_kernel(const topk_args a) {
    __shared__ uint4 tile[2][SLAM_TILE_ROWS * 2 + 4];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int N = a.N;
    const int qbase = blockIdx.x * 256 + wave * 64 + lane;
    const bool nobound = a.bound == nullptr;
    const int pad = K - a.k;                                        // leading slots pinned to key 0

    u32 qr[1][8];
    bf_load_query(a.q, qbase < N ? qbase : N - 1, qr[0]);          // clamp: tail lanes compute a duplicate and never store
    u32 keys[K];
#pragma unroll
    for (int i = 0; i < K; i++) keys[i] = i < pad ? 0u : SLAM_KEY_NONE;
    u32 init[1] = {SLAM_ACC_BIAS - (SLAM_KEY_NONE >> SLAM_KEY_IDX_BITS)};   // "distance 511": everything enters
    u32 gk[1] = {SLAM_BOUND_IDLE}, pend[1] = {0u};
    auto share = [&]() {
        const u32 kth[1] = {keys[K - 1]};
        share_bound<1>(a.bound, qbase, N, kth, init, gk, pend);
    };
    auto nobody_published = [&]() -> bool { return __ballot(gk[0] != SLAM_BOUND_IDLE) == 0ull; };
    auto tighten = [&]() { init[0] = max(init[0], SLAM_ACC_BIAS - (keys[K - 1] >> SLAM_KEY_IDX_BITS)); };

    const int t0 = blockIdx.y * a.chunk;
    const int t1 = min(a.M, t0 + a.chunk);
    const uint4* __restrict__ t = a.t;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int g = 2 * t0 + tid + i * 256;
        tile[0][tid + i * 256] = g < 2 * t1 ? t[(size_t)g] : make_uint4(0, 0, 0, 0);
    }
    __syncthreads();

    int buf = 0;
    for (int tb = t0; tb < t1; tb += SLAM_TILE_ROWS) {
        const int nb = tb + SLAM_TILE_ROWS;
        uint4 nxt[2];
        if (nb < t1) {
#pragma unroll
            for (int i = 0; i < 2; i++) {
                const int g = 2 * nb + tid + i * 256;
                nxt[i] = g < 2 * t1 ? t[(size_t)g] : make_uint4(0, 0, 0, 0);
            }
        }
        if (!nobound) share();
        const int cnt = __builtin_amdgcn_readfirstlane(min(SLAM_TILE_ROWS, t1 - tb));
        const uint4* tp = tile[buf];
        int j = 0;
        uint4 a0 = tp[0], c0 = tp[1];
        constexpr int U = SLAM_GROUP_PAIRS;
        // (through a lambda: called directly, the two call sites compile to other code than they did with the read written here)
        auto group = [&](const u32 (&ini)[1], u32 (&acc)[U][1]) { bf_group_acc<U>(qr, tp, j, a0, c0, ini, acc); };
        // the bound is re-read after 16, 32, 64 and 128 rows of the chunk, later once per tile
        int seg_end = tb == t0 ? 16 : cnt;
        if (tb == t0 && a.cold >= U && (nobound || nobody_published())) {
            const int lim = min(a.cold, cnt);
            const u32 zero[1] = {0u};
            for (; j + U <= lim; j += U) {
                u32 acc[U][1];
                group(zero, acc);
#pragma unroll
                for (int u = 0; u < U; u++) topk_insert<K>(keys, (acc[u][0] << SLAM_KEY_IDX_BITS) | (u32)(tb + j + u));
            }
            tighten();
            if (j < cnt && !nobound) share();
            while (seg_end <= j) seg_end *= 2;
        }
        while (true) {
            const int lim = min(seg_end, cnt);
            for (; j + U <= lim; j += U) {
                u32 acc[U][1];
                group(init, acc);
                topk_filter_update<K, U>(acc, (u32)(tb + j), keys, init);
            }
            if (lim >= cnt) break;
            if (!nobound) share();
            seg_end *= 2;
        }
        for (; j < cnt; j++) {                                      // fewer than 16 rows left: only at the end of a chunk
            const uint4 x0 = tp[2 * j], y0 = tp[2 * j + 1];
            u32 acc1[1][1];
            row_acc<1>(qr, x0, y0, init, acc1[0]);
            topk_filter_update<K, 1>(acc1, (u32)(tb + j), keys, init);
        }
        if (nb < t1) {
#pragma unroll
            for (int i = 0; i < 2; i++) tile[buf ^ 1][tid + i * 256] = nxt[i];
        }
        __syncthreads();
        buf ^= 1;
    }
    __builtin_amdgcn_s_setprio(0);   // the scan raised it (row_acc)
    asm volatile("" ::"v"(pend[0]));   // the parked return of share_bound: every write to bound[] is done when the block ends
    if (qbase >= N) return;
    if (a.part) {
        u32* dst = a.part + ((size_t)blockIdx.y * N + qbase) * a.k;
#pragma unroll
        for (int i = 0; i < K; i++)
            if (i >= pad) dst[i - pad] = keys[i];
    } else {
        int32_t* oi = a.idx + (size_t)qbase * a.k;
        int32_t* od = a.dist + (size_t)qbase * a.k;
#pragma unroll
        for (int i = 0; i < K; i++)
            if (i >= pad) {
                oi[i - pad] = bf_key_idx(keys[i], a.train_base);
                od[i - pad] = bf_key_dist(keys[i]);
            }
    }
}

// Merge the S sorted chunk lists of every query into its top-k, decode, and put bound[] back to idle.  The head of each
// list is loaded ahead, eight lists at a time, independently of the insertions: most lists are rejected at their head,
// and a dependent load per list would put S round trips in a row on the critical path.
template <int K>
__global__ __launch_bounds__(256) void bf_topk_merge_kernel(const u32* __restrict__ part, int S, int N, int k, int train_base,
                                                            u32* __restrict__ bound, int32_t* __restrict__ idx,
                                                            int32_t* __restrict__ dist) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const int pad = K - k;
    u32 keys[K];
#pragma unroll
    for (int i = 0; i < K; i++) keys[i] = i < pad ? 0u : SLAM_KEY_NONE;
    const size_t stride = (size_t)N * k;
    const u32* l0 = part + (size_t)n * k;
    for (int s0 = 0; s0 < S; s0 += 8) {
        u32 head[8];
#pragma unroll
        for (int u = 0; u < 8; u++) head[u] = s0 + u < S ? l0[(size_t)(s0 + u) * stride] : SLAM_KEY_NONE;
#pragma unroll
        for (int u = 0; u < 8; u++) {
            if (head[u] >= keys[K - 1]) continue;                  // the list's best key cannot enter: nor can the rest
            topk_insert<K>(keys, head[u]);
            const u32* l = l0 + (size_t)(s0 + u) * stride;
            for (int j = 1; j < k; j++) {
                const u32 x = l[j];
                if (x >= keys[K - 1]) break;
                topk_insert<K>(keys, x);
            }
        }
    }
    int32_t* oi = idx + (size_t)n * k;
    int32_t* od = dist + (size_t)n * k;
#pragma unroll
    for (int i = 0; i < K; i++)
        if (i >= pad) {
            oi[i - pad] = bf_key_idx(keys[i], train_base);
            od[i - pad] = bf_key_dist(keys[i]);
        }
    if (bound) bound[n] = SLAM_BOUND_IDLE;                          // (the next search is ordered behind this kernel by the stream)
}

// Merge G decoded [N][k] tables (global indices) by (dist, idx): passes over train sets beyond 2^23 rows, shards.
template <int K>
__global__ __launch_bounds__(256) void bf_merge_topk_kernel(const int32_t* __restrict__ idx_parts, const int32_t* __restrict__ dist_parts,
                                                            int G, int N, int k, int32_t* __restrict__ idx, int32_t* __restrict__ dist) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const int pad = K - k;
    const uint64_t NONE = ~0ull;
    uint64_t keys[K];
#pragma unroll
    for (int i = 0; i < K; i++) keys[i] = i < pad ? 0ull : NONE;
    for (int g = 0; g < G; g++) {
        const size_t off = ((size_t)g * N + n) * k;
        for (int j = 0; j < k; j++) {
            const int32_t pi = idx_parts[off + j];
            const uint64_t x = pi < 0 ? NONE : ((uint64_t)(u32)dist_parts[off + j] << 32) | (u32)pi;
            if (x >= keys[K - 1]) break;                             // the table is sorted: nothing behind it can enter
            topk_insert<K>(keys, x);
        }
    }
    int32_t* oi = idx + (size_t)n * k;
    int32_t* od = dist + (size_t)n * k;
#pragma unroll
    for (int i = 0; i < K; i++)
        if (i >= pad) {
            const uint64_t key = keys[i];
            oi[i - pad] = key == NONE ? SLAM_NO_MATCH_IDX : (int)(u32)key;
            od[i - pad] = key == NONE ? SLAM_NO_MATCH_DIST : (int)(key >> 32);
        }
}

__global__ __launch_bounds__(256) void bf_topk_fill_none_kernel(int64_t count, int32_t* __restrict__ idx, int32_t* __restrict__ dist) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    idx[i] = SLAM_NO_MATCH_IDX;
    dist[i] = SLAM_NO_MATCH_DIST;
}

// ---- host side -----------------------------------------------------------

struct topk_plan {
    int K;          // instantiation
    int qblocks;    // grid.x
    int chunks;     // grid.y of every full pass
    int chunk;      // rows per chunk
    int resident;   // blocks per CU counted on
    int passes;     // ceil(M / 2^23)
    int64_t ws;     // bytes of partial tables (0: one chunk, no merge kernel)
};

// A pure function of the CU count, the blocks per CU and the shape (slam_bf_topk_plan_describe exposes it without a device).
// The chunks are bf_chunk_rule's, of at least one tile and under the partial tables' cap.  The plan of the first (largest)
// pass serves every pass.
static topk_plan topk_plan_core(int num_cu, int resident, int64_t N, int64_t M, int k) {
    topk_plan p;
    p.K = topk_width(k);
    p.resident = resident;
    const int64_t PASS = SLAM_MAX_TRAIN_PER_PASS;
    p.passes = (int)((M + PASS - 1) / PASS);
    const int64_t per = N * k * 4;                                  // one chunk's partial table
    const bf_chunks c = bf_chunk_rule(num_cu, resident, N, M < PASS ? M : PASS, SLAM_TOPK_MIN_CHUNK, per, SLAM_TOPK_WS_CAP);
    p.qblocks = c.qblocks;
    p.chunks = c.chunks;
    p.chunk = (int)c.chunk;
    p.ws = p.chunks > 1 ? (int64_t)p.chunks * per : 0;
    return p;
}

// f(std::integral_constant<int, K>()) for the instantiation K (topk_width)
template <typename F>
static int topk_dispatch(int K, F f) {
    switch (K) {
        case 4: return f(std::integral_constant<int, 4>());
        case 8: return f(std::integral_constant<int, 8>());
        case 16: return f(std::integral_constant<int, 16>());
        default: return f(std::integral_constant<int, 32>());
    }
}

static int topk_make_plan(slam_ctx* ctx, int64_t N, int64_t M, int k, topk_plan* p) {
    const int K = topk_width(k);
    int occ = 0;
    const int rc = topk_dispatch(K, [&](auto Kc) -> int {
        static std::atomic<int> once{0};                             // one per instantiation
        return slam_occupancy_once((const void*)bf_topk_kernel<Kc()>, &once, &occ);
    });
    if (rc) return rc;
    const int res = topk_resident(K);
    *p = topk_plan_core(ctx->num_cu, occ < res ? occ : res, N, M, k);
    return SLAM_OK;
}

extern "C" int slam_bf_topk_plan_describe(int num_cu, int64_t N, int64_t M, int K, int32_t* h_plan) {
    SLAM_REQUIRE(h_plan, "slam_bf_topk_plan_describe: null h_plan");
    SLAM_REQUIRE(num_cu >= 1 && num_cu <= 65536, "num_cu=%d out of range", num_cu);
    SLAM_REQUIRE(K >= 1 && K <= SLAM_BF_KNN_MAX, "K=%d outside [1, %d]", K, SLAM_BF_KNN_MAX);
    SLAM_REQUIRE(N >= 0 && M >= 0 && N <= (1ll << 30) && M <= 0x7FFFFFFFll, "bad sizes (N=%lld, M=%lld)", (long long)N, (long long)M);
    const topk_plan p = topk_plan_core(num_cu, topk_resident(topk_width(K)), N, M, K);
    const int32_t v[SLAM_TOPK_PLAN] = {p.K, p.qblocks, p.chunks, p.chunk, p.resident, p.passes, (int32_t)p.ws, p.chunks > 1 ? 1 : 0};
    memcpy(h_plan, v, sizeof(v));
    return SLAM_OK;
}

// one pass over at most 2^23 train rows: the search, then (several chunks) the merge of the chunk lists
static int topk_pass(slam_ctx* ctx, const topk_plan& p, const void* d_query, int64_t N, const void* d_train, int64_t M,
                     int64_t train_base, int k, int32_t* d_idx, int32_t* d_dist, u32* part, u32* bound) {
    topk_args a;
    a.q = (const uint4*)d_query;
    a.t = (const uint4*)d_train;
    a.N = (int)N;
    a.M = (int)M;
    a.chunk = p.chunk;
    const int chunks = (int)((M + p.chunk - 1) / p.chunk);          // (a shorter last pass may need fewer)
    a.k = k;
    a.train_base = (int)train_base;
    a.cold = SLAM_COLD_ROWS;
    a.bound = chunks > 1 ? bound : nullptr;
    a.part = chunks > 1 ? part : nullptr;
    a.idx = d_idx;
    a.dist = d_dist;
    const dim3 grid(p.qblocks, chunks), block(256);
    SLAM_HIP(hipGetLastError());
    if (int rc = slam_prof_begin(ctx)) return rc;
    const dim3 mg((unsigned)((N + 255) / 256));
    topk_dispatch(p.K, [&](auto Kc) -> int {
        bf_topk_kernel<Kc()><<<grid, block, 0, ctx->stream>>>(a);
        if (chunks > 1)
            bf_topk_merge_kernel<Kc()><<<mg, block, 0, ctx->stream>>>(part, chunks, (int)N, k, a.train_base, bound, d_idx, d_dist);
        return SLAM_OK;
    });
    if (int rc = slam_prof_end(ctx)) return rc;
    const int rc = slam_launch_check("top-k kernel");
    if (rc) (void)bf_state_reset(ctx);
    return rc;
}

static int topk_merge_launch(slam_ctx* ctx, const int32_t* d_idx_parts, const int32_t* d_dist_parts, int64_t G, int64_t N, int k,
                             int32_t* d_idx, int32_t* d_dist) {
    const dim3 grid((unsigned)((N + 255) / 256)), block(256);
    return topk_dispatch(topk_width(k), [&](auto Kc) -> int {
        bf_merge_topk_kernel<Kc()><<<grid, block, 0, ctx->stream>>>(d_idx_parts, d_dist_parts, (int)G, (int)N, k, d_idx, d_dist);
        SLAM_HIP(hipGetLastError());
        return SLAM_OK;
    });
}

// slam_bf_knn_u256 without the call lock
static int topk_search(slam_ctx* ctx, const void* d_query, int64_t N, const void* d_train, int64_t M, int64_t train_base,
                       int K, int32_t* d_idx, int32_t* d_dist) {
    SLAM_REQUIRE(ctx, "slam_bf_knn_u256: null ctx");
    SLAM_REQUIRE(K >= 1 && K <= SLAM_BF_KNN_MAX, "K=%d outside [1, %d]", K, SLAM_BF_KNN_MAX);
    SLAM_REQUIRE(N >= 0 && M >= 0, "negative size (N=%lld, M=%lld)", (long long)N, (long long)M);
    SLAM_REQUIRE(N <= (1ll << 30), "N=%lld exceeds 2^30 query rows per call", (long long)N);
    SLAM_REQUIRE(train_base >= 0 && train_base + M <= 0x7FFFFFFFll, "train_base + M must fit int32");
    if (N == 0) return SLAM_OK;
    SLAM_REQUIRE(d_query && d_idx && d_dist, "slam_bf_knn_u256: null device pointer");
    SLAM_REQUIRE(((uintptr_t)d_query & 15) == 0 && ((uintptr_t)d_train & 15) == 0,
                 "descriptor pointers must be 16-byte aligned");
    SLAM_REQUIRE(((uintptr_t)d_idx & 3) == 0 && ((uintptr_t)d_dist & 3) == 0, "result pointers must be 4-byte aligned");
    SLAM_HIP(hipSetDevice(ctx->device));
    if (M == 0) {
        const int64_t count = N * K;
        bf_topk_fill_none_kernel<<<dim3((unsigned)((count + 255) / 256)), dim3(256), 0, ctx->stream>>>(count, d_idx, d_dist);
        SLAM_HIP(hipGetLastError());
        return SLAM_OK;
    }
    SLAM_REQUIRE(d_train, "slam_bf_knn_u256: null train pointer");
    topk_plan p;
    if (int rc = topk_make_plan(ctx, N, M, K, &p)) return rc;
    // one workspace request for everything the call needs: per-pass tables (several passes), then the partial tables
    const uint64_t table = (uint64_t)N * K * sizeof(int32_t);
    const uint64_t pass_bytes = p.passes > 1 ? 2 * (uint64_t)p.passes * table : 0;
    void* ws = nullptr;
    if (pass_bytes + (uint64_t)p.ws > 0)
        if (int rc = slam_workspace(ctx, pass_bytes + (uint64_t)p.ws, &ws)) return rc;
    u32* part = (u32*)((char*)ws + pass_bytes);
    bf_state st = {};
    if (p.chunks > 1)
        if (int rc = bf_state_get(ctx, N, &st)) return rc;
    if (p.passes == 1) return topk_pass(ctx, p, d_query, N, d_train, M, train_base, K, d_idx, d_dist, part, st.bound);
    int32_t* idx_parts = (int32_t*)ws;
    int32_t* dist_parts = (int32_t*)((char*)ws + p.passes * table);
    const int64_t PASS = SLAM_MAX_TRAIN_PER_PASS;
    for (int64_t g = 0; g < p.passes; g++) {
        const int64_t m0 = g * PASS, m = (M - m0) < PASS ? (M - m0) : PASS;
        if (int rc = topk_pass(ctx, p, d_query, N, (const char*)d_train + m0 * SLAM_DESC_BYTES, m, train_base + m0, K,
                               idx_parts + g * N * K, dist_parts + g * N * K, part, st.bound))
            return rc;
    }
    return topk_merge_launch(ctx, idx_parts, dist_parts, p.passes, N, K, d_idx, d_dist);
}

extern "C" int slam_bf_knn_u256(slam_ctx* ctx, const void* d_query, int64_t N, const void* d_train, int64_t M, int64_t train_base,
                                int K, int32_t* d_idx, int32_t* d_dist) {
    SLAM_REQUIRE(ctx, "slam_bf_knn_u256: null ctx");
    std::lock_guard<std::mutex> lk(ctx->call_mu);
    return topk_search(ctx, d_query, N, d_train, M, train_base, K, d_idx, d_dist);
}

extern "C" int slam_bf_merge_topk(slam_ctx* ctx, const int32_t* d_idx_parts, const int32_t* d_dist_parts, int64_t G, int64_t N, int K,
                                  int32_t* d_idx, int32_t* d_dist) {
    SLAM_REQUIRE(ctx, "slam_bf_merge_topk: null ctx");
    SLAM_REQUIRE(K >= 1 && K <= SLAM_BF_KNN_MAX, "K=%d outside [1, %d]", K, SLAM_BF_KNN_MAX);
    SLAM_REQUIRE(G >= 1 && G <= 0x7FFFFFFFll && N >= 0 && N <= (1ll << 30), "bad sizes (G=%lld, N=%lld)", (long long)G, (long long)N);
    if (N == 0) return SLAM_OK;
    SLAM_REQUIRE(d_idx_parts && d_dist_parts && d_idx && d_dist, "slam_bf_merge_topk: null device pointer");
    SLAM_REQUIRE(((uintptr_t)d_idx_parts & 3) == 0 && ((uintptr_t)d_dist_parts & 3) == 0 && ((uintptr_t)d_idx & 3) == 0 &&
                 ((uintptr_t)d_dist & 3) == 0, "table pointers must be 4-byte aligned");
    SLAM_HIP(hipSetDevice(ctx->device));
    return topk_merge_launch(ctx, d_idx_parts, d_dist_parts, G, N, K, d_idx, d_dist);
}

// upload, search, download, one stream synchronisation (through the context's host-buffer arena)
extern "C" int slam_bf_knn_u256_host(slam_ctx* ctx, const uint8_t* h_query, int64_t N, const uint8_t* h_train, int64_t M, int K,
                                     int32_t* h_idx, int32_t* h_dist) {
    SLAM_REQUIRE(ctx, "slam_bf_knn_u256_host: null ctx");
    SLAM_REQUIRE(K >= 1 && K <= SLAM_BF_KNN_MAX, "K=%d outside [1, %d]", K, SLAM_BF_KNN_MAX);
    SLAM_REQUIRE(N >= 0 && M >= 0 && N <= (1ll << 28) && M <= (1ll << 28), "bad sizes N=%lld M=%lld", (long long)N, (long long)M);
    if (N == 0) return SLAM_OK;
    SLAM_REQUIRE(h_query && h_idx && h_dist && (h_train || M == 0), "slam_bf_knn_u256_host: null host pointer");
    std::lock_guard<std::mutex> lk(ctx->call_mu);
    SLAM_HIP(hipSetDevice(ctx->device));
    const uint64_t qbytes = (uint64_t)N * SLAM_DESC_BYTES, tbytes = (uint64_t)M * SLAM_DESC_BYTES, table = (uint64_t)N * K * 4;
    const uint64_t off_t = slam_align_up(qbytes), off_i = off_t + slam_align_up(tbytes), off_d = off_i + slam_align_up(table);
    const uint64_t total = off_d + slam_align_up(table);
    void *dev = nullptr, *host = nullptr;
    if (int rc = slam_io_arena(ctx, total, total, &dev, &host)) return rc;
    uint8_t* hb = (uint8_t*)host;
    uint8_t* db = (uint8_t*)dev;
    memcpy(hb, h_query, qbytes);
    if (tbytes) memcpy(hb + off_t, h_train, tbytes);
    ctx->io_h2d_bytes += qbytes + tbytes;
    ctx->io_d2h_bytes += 2 * table;
    SLAM_HIP(hipMemcpyAsync(db, hb, off_t + tbytes, hipMemcpyHostToDevice, ctx->stream));
    if (int rc = topk_search(ctx, db, N, db + off_t, M, 0, K, (int32_t*)(db + off_i), (int32_t*)(db + off_d))) return rc;
    SLAM_HIP(hipMemcpyAsync(hb + off_i, db + off_i, off_d - off_i + table, hipMemcpyDeviceToHost, ctx->stream));
    SLAM_HIP(hipStreamSynchronize(ctx->stream));
    memcpy(h_idx, hb + off_i, table);
    memcpy(h_dist, hb + off_d, table);
    return SLAM_OK;
}
