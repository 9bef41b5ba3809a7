// bf_radius.hip — brute-force Hamming radius search over 256-bit ORB descriptors on gfx950 (MI355X).  Replaces
// cv2.BFMatcher(NORM_HAMMING).radiusMatch(query, train, maxDistance): EVERY train row within a distance of each query,
// what loop closure and relocalisation collect as candidates, where the top-2 and top-k searches return a fixed number.
//
// Design: the threshold is known before the first row, so the scan is the top-k search's without a list
// and without any exchange between blocks; the new part is output of variable length, in compressed-row (CSR) form.
//   1. count   bf_radius_scan_kernel<false>: grid = query blocks x train chunks, one query per lane, train rows through
//              the LDS tile of bf_topk_kernel (bf_group_acc), row_acc<1> with init = 2^31 - th (d < th <=> sign bit clear), one ballot
//              per group of 16 rows; only a group that fires pays for the per-lane count.  Plain stores into a
//              [chunks][N] table: no atomics, no bound[].
//   2. scan    three small kernels: each query's chunk counts become its per-chunk prefixes (in place), and an exclusive
//              scan over the queries gives offsets[N + 1]; the host reads the total back.
//   3. emit    bf_radius_scan_kernel<true>: the same scan again; each lane writes its passing rows in ascending row order
//              at its chunk's prefix, as (row + train_base, distance).  Chunks cover ascending row ranges, so each
//              query's list comes out in row order, into a staging area of the context's workspace.
//   4. order   a stable per-query counting sort by distance (257 bins) from the staging area into the caller's arrays:
//              (distance, row) order without packing keys, so nothing limits the row index to 23 bits.  Lists of up to
//              SLAM_RADIUS_SHORT entries are sorted by one wave each; longer ones are cut into tiles of as many entries,
//              and take a histogram per tile, a scan per list over (bin, tile), and a stable scatter per tile.
// Every step is deterministic (counts are summed in a fixed order, every position is computed, not claimed), so the
// results are bit-identical whatever the grid and chunking.  Row indices are plain int32: no passes are needed.
#include "bf_common.h"
#include <atomic>
#include <cmath>

#define SLAM_RADIUS_WS_CAP (64ull << 20)   // bytes of chunk count table one search may use (fewer chunks beyond)
#define SLAM_RADIUS_MIN_CHUNK 256          // rows: one LDS tile
#define SLAM_RADIUS_SHORT 4096             // entries a list may hold to be sorted by one wave; also the long path's tile
#define SLAM_RADIUS_BINS 257               // distances 0 .. 256
#define SLAM_RADIUS_RESIDENT 8             // blocks of bf_radius_scan_kernel a CU holds (VGPRs: DESIGN.md §3d)
#define SLAM_RADIUS_PLAN 8                 // entries of slam_bf_radius_plan_describe's h_plan

// The selection boundary, in one place: a row is kept when (float)distance <= max_distance, which for an integer distance
// in [0, 256] is distance < th with th = floor(max_distance) + 1, clamped to [0, 257] (NaN and negative radii keep
// nothing, 256 and beyond keep everything).  OpenCV's CPU matcher compares with <=; its CUDA matcher with <.
extern "C" int slam_bf_radius_threshold(float max_distance) {
    if (!(max_distance >= 0.0f)) return 0;                          // NaN, negative
    if (max_distance >= 256.0f) return SLAM_RADIUS_BINS;
    return (int)std::floor(max_distance) + 1;
}

struct radius_args {
    const uint4* q;        // [N] query rows (two uint4 each)
    const uint4* t;        // [M] train rows
    int N;
    int64_t M;
    int64_t chunk;         // rows per chunk: block (x, y) scans rows [y * chunk, min(M, (y + 1) * chunk))
    u32 init;              // 2^31 - th
    int train_base;        // added to every emitted index
    int32_t* cnt;          // [chunks][N]: counts (count), then each query's exclusive prefix over the chunks (emit)
    const int64_t* off;    // [N + 1] list offsets (emit)
    int2* stage;           // [total] (row + train_base, distance) in row order (emit)
};

// One block = 256 queries (one per lane) x one chunk of train rows.  EMIT = false counts the rows with d < th, EMIT = true
// writes them.  The tile feed is bf_topk_kernel's, the 16-row group bf_group_acc.
template <bool EMIT>
__global__ __launch_bounds__(256) void bf_radius_scan_kernel(const radius_args a) {
    __shared__ uint4 tile[2][SLAM_TILE_ROWS * 2 + 4];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int N = a.N;
    const int qbase = blockIdx.x * 256 + wave * 64 + lane;
    const bool valid = qbase < N;

    u32 qr[1][8];
    bf_load_query(a.q, valid ? qbase : N - 1, qr[0]);               // clamp: tail lanes compute a duplicate and never store
    const u32 init[1] = {a.init};
    int count = 0;
    int2* out = nullptr;
    if (EMIT && valid) out = a.stage + a.off[qbase] + a.cnt[(size_t)blockIdx.y * N + qbase];

    const int64_t t0 = (int64_t)blockIdx.y * a.chunk;
    const int64_t t1 = min(a.M, t0 + a.chunk);
    const uint4* __restrict__ t = a.t;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int64_t g = 2 * t0 + tid + i * 256;
        tile[0][tid + i * 256] = g < 2 * t1 ? t[g] : make_uint4(0, 0, 0, 0);
    }
    __syncthreads();

    // the rows of one group whose sign bit is clear: counted, or written in row order
    constexpr int U = SLAM_GROUP_PAIRS;
    auto take = [&](const u32 (&acc)[U][1], int n, int row0) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            if (u < n) {                                            // (n is wave-uniform)
                if (!EMIT) {
                    count += (int)((acc[u][0] >> 31) ^ 1u);
                } else if (__ballot((int)acc[u][0] >= 0) != 0ull) {
                    if ((int)acc[u][0] >= 0 && valid) *out++ = make_int2(row0 + u + a.train_base, (int)(acc[u][0] - init[0]));
                }
            }
        }
    };

    int buf = 0;
    for (int64_t tb = t0; tb < t1; tb += SLAM_TILE_ROWS) {
        const int64_t nb = tb + SLAM_TILE_ROWS;
        uint4 nxt[2];
        if (nb < t1) {
#pragma unroll
            for (int i = 0; i < 2; i++) {
                const int64_t g = 2 * nb + tid + i * 256;
                nxt[i] = g < 2 * t1 ? t[g] : make_uint4(0, 0, 0, 0);
            }
        }
        const int cnt = __builtin_amdgcn_readfirstlane((int)min((int64_t)SLAM_TILE_ROWS, t1 - tb));
        const uint4* tp = tile[buf];
        int j = 0;
        uint4 a0 = tp[0], c0 = tp[1];
        for (; j + U <= cnt; j += U) {
            u32 acc[U][1];
            bf_group_acc<U>(qr, tp, j, a0, c0, init, acc);
            u32 m = acc[0][0];
#pragma unroll
            for (int u = 1; u < U; u++) m &= acc[u][0];
            if (__builtin_expect(__ballot((int)m >= 0) != 0ull, 0)) take(acc, U, (int)(tb + j));
        }
        if (j < cnt) {                                              // fewer than 16 rows left: only at the end of a chunk
            u32 acc[U][1];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int r = j + u < cnt ? j + u : j;
                row_acc<1>(qr, tp[2 * r], tp[2 * r + 1], init, acc[u]);
            }
            take(acc, cnt - j, (int)(tb + j));
        }
        if (nb < t1) {
#pragma unroll
            for (int i = 0; i < 2; i++) tile[buf ^ 1][tid + i * 256] = nxt[i];
        }
        __syncthreads();
        buf ^= 1;
    }
    __builtin_amdgcn_s_setprio(0);   // the scan raised it (row_acc)
    if (!EMIT && valid) a.cnt[(size_t)blockIdx.y * N + qbase] = count;
}

// ---- the scan: chunk counts -> per-chunk prefixes, list lengths -> offsets[N + 1] -------------------------------------

// one thread per query: its chunk counts become exclusive prefixes (in place) and its list length goes to len[q];
// per block of 256 queries the sums of (entries, long lists, tiles of long lists) go to bsum[3 * block]
__global__ __launch_bounds__(256) void bf_radius_prefix_kernel(int32_t* __restrict__ cnt, int S, int N, int32_t* __restrict__ len,
                                                               int64_t* __restrict__ bsum) {
    __shared__ int64_t lds4[4];
    const int q = blockIdx.x * 256 + threadIdx.x;
    int64_t run = 0;
    if (q < N) {
        for (int y = 0; y < S; y++) {
            int32_t* c = cnt + (size_t)y * N + q;
            const int32_t v = *c;
            *c = (int32_t)run;
            run += v;
        }
        len[q] = (int32_t)run;
    }
    const bool lng = run > SLAM_RADIUS_SHORT;
    const int64_t v[3] = {run, lng ? 1 : 0, lng ? (run + SLAM_RADIUS_SHORT - 1) / SLAM_RADIUS_SHORT : 0};
    for (int i = 0; i < 3; i++) {
        int64_t tot;
        (void)bf_block_excl_scan<int64_t>(v[i], lds4, &tot);
        if (threadIdx.x == 0) bsum[3 * (size_t)blockIdx.x + i] = tot;
    }
}

// one block: exclusive scan of the B block sums (in place); the grand totals go to tot[3] and offsets[N]
__global__ __launch_bounds__(256) void bf_radius_blocks_kernel(int64_t* __restrict__ bsum, int64_t B, int64_t* __restrict__ tot,
                                                               int64_t* __restrict__ offsets, int N) {
    __shared__ int64_t lds4[4];
    const int64_t per = (B + 255) / 256;
    const int64_t b0 = min(B, (int64_t)threadIdx.x * per), b1 = min(B, b0 + per);
    for (int i = 0; i < 3; i++) {
        int64_t s = 0;
        for (int64_t b = b0; b < b1; b++) s += bsum[3 * b + i];
        int64_t all;
        int64_t run = bf_block_excl_scan<int64_t>(s, lds4, &all);
        for (int64_t b = b0; b < b1; b++) {
            const int64_t v = bsum[3 * b + i];
            bsum[3 * b + i] = run;
            run += v;
        }
        if (threadIdx.x == 0) {
            tot[i] = all;
            if (i == 0) offsets[N] = all;
        }
    }
}

// one thread per query: offsets[q]; a long list gets its rank among the long lists (lq_id) and the end of its tiles
__global__ __launch_bounds__(256) void bf_radius_offsets_kernel(const int32_t* __restrict__ len, int N, const int64_t* __restrict__ bsum,
                                                                int64_t* __restrict__ offsets, int32_t* __restrict__ lq_id,
                                                                int64_t* __restrict__ lq_tile_end) {
    __shared__ int64_t lds4[4];
    const int q = blockIdx.x * 256 + threadIdx.x;
    const int64_t n = q < N ? len[q] : 0;
    const bool lng = n > SLAM_RADIUS_SHORT;
    const int64_t tiles = lng ? (n + SLAM_RADIUS_SHORT - 1) / SLAM_RADIUS_SHORT : 0;
    int64_t tot;
    const int64_t off = bsum[3 * (size_t)blockIdx.x] + bf_block_excl_scan<int64_t>(n, lds4, &tot);
    const int64_t rank = bsum[3 * (size_t)blockIdx.x + 1] + bf_block_excl_scan<int64_t>(lng ? 1 : 0, lds4, &tot);
    const int64_t tbeg = bsum[3 * (size_t)blockIdx.x + 2] + bf_block_excl_scan<int64_t>(tiles, lds4, &tot);
    if (q < N) {
        offsets[q] = off;
        if (lng) {
            lq_id[rank] = q;
            lq_tile_end[rank] = tbeg + tiles;
        }
    }
}

// ---- the order: stable counting sort by distance -----------------------------------------------------------------

// h[0 .. 256] = histogram of the distances of src[0 .. n) (one wave)
__device__ __forceinline__ void wave_histogram(int32_t* h, const int2* __restrict__ src, int n) {
    const int lane = threadIdx.x & 63;
    for (int b = lane; b < SLAM_RADIUS_BINS; b += 64) h[b] = 0;
    bf_wave_lds_sync();
    for (int i = lane; i < n; i += 64) atomicAdd(&h[src[i].y], 1);
    bf_wave_lds_sync();
}

// h[0 .. 256] -> its exclusive scan (one wave: four bins per lane, bin 256 last)
__device__ __forceinline__ void wave_excl_scan_bins(int32_t* h) {
    const int lane = threadIdx.x & 63;
    const int32_t v0 = h[4 * lane], v1 = h[4 * lane + 1], v2 = h[4 * lane + 2], v3 = h[4 * lane + 3];
    const int32_t s = v0 + v1 + v2 + v3;
    int32_t x = s;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int32_t y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
    const int32_t e = x - s;
    h[4 * lane] = e;
    h[4 * lane + 1] = e + v0;
    h[4 * lane + 2] = e + v0 + v1;
    h[4 * lane + 3] = e + v0 + v1 + v2;
    const int32_t all = __shfl(x, 63, 64);
    if (lane == 0) h[256] = all;
    bf_wave_lds_sync();
}

// Write src[0 .. n) to dst_* [dst0 + base[d] + (rank among the earlier entries of distance d)], 64 entries per round in
// order; base[] (LDS) advances by what each round placed.  Ties keep their order: the sort is stable.
__device__ __forceinline__ void wave_stable_scatter(int32_t* base, const int2* __restrict__ src, int n, int32_t* __restrict__ dst_idx,
                                                    int32_t* __restrict__ dst_dist, int64_t dst0) {
    const int lane = threadIdx.x & 63;
    const unsigned long long lt = lane ? (~0ull >> (64 - lane)) : 0ull;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const bool in = i < n;
        const int2 e = in ? src[i] : make_int2(0, 0);
        // lanes holding the same distance: nine ballots over its bits
        unsigned long long same = __ballot(in);
#pragma unroll
        for (int b = 0; b < 9; b++) {
            const bool bit = (e.y >> b) & 1;
            const unsigned long long m = __ballot(in && bit);
            same &= bit ? m : ~m;
        }
        const int32_t pos = in ? base[e.y] + __popcll(same & lt) : 0;
        bf_wave_lds_sync();
        if (in) {
            dst_idx[dst0 + pos] = e.x;
            dst_dist[dst0 + pos] = e.y;
            if (63 - __clzll(same) == lane) base[e.y] = pos + 1;     // the group's last lane: one past its last entry
        }
        bf_wave_lds_sync();
    }
}

// one wave per query whose list holds 1 .. SLAM_RADIUS_SHORT entries: histogram, scan, scatter
__global__ __launch_bounds__(256) void bf_radius_sort_short_kernel(const int2* __restrict__ stage, const int64_t* __restrict__ offsets,
                                                                   int N, int32_t* __restrict__ idx, int32_t* __restrict__ dist) {
    __shared__ int32_t hist[4][SLAM_RADIUS_BINS + 3];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + wave;
    if (q >= N) return;
    const int64_t o = offsets[q];
    const int n = (int)(offsets[q + 1] - o);
    if (n == 0 || n > SLAM_RADIUS_SHORT) return;
    if (n == 1) {
        if (lane == 0) {
            const int2 e = stage[o];
            idx[o] = e.x;
            dist[o] = e.y;
        }
        return;
    }
    int32_t* h = hist[wave];
    wave_histogram(h, stage + o, n);
    wave_excl_scan_bins(h);
    wave_stable_scatter(h, stage + o, n, idx, dist, o);
}

// the long list and the tile within it of global tile w (lq_tile_end: inclusive ends, ascending)
__device__ __forceinline__ int64_t radius_find_tile(const int64_t* __restrict__ lq_tile_end, int64_t L, int64_t w, int64_t* first) {
    int64_t lo = 0, hi = L - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (lq_tile_end[mid] > w) hi = mid;
        else lo = mid + 1;
    }
    *first = lo ? lq_tile_end[lo - 1] : 0;
    return lo;
}

// one wave per tile of a long list: its histogram, to ghist[w][257]
__global__ __launch_bounds__(256) void bf_radius_sort_hist_kernel(const int2* __restrict__ stage, const int64_t* __restrict__ offsets,
                                                                  const int32_t* __restrict__ lq_id, const int64_t* __restrict__ lq_tile_end,
                                                                  int64_t L, int64_t tiles, int32_t* __restrict__ ghist) {
    __shared__ int32_t hist[4][SLAM_RADIUS_BINS + 3];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + wave;
    if (w >= tiles) return;
    int64_t first;
    const int q = lq_id[radius_find_tile(lq_tile_end, L, w, &first)];
    const int64_t o = offsets[q], n = offsets[q + 1] - o;
    const int64_t s = (w - first) * SLAM_RADIUS_SHORT;
    int32_t* h = hist[wave];
    wave_histogram(h, stage + o + s, (int)min((int64_t)SLAM_RADIUS_SHORT, n - s));
    for (int b = lane; b < SLAM_RADIUS_BINS; b += 64) ghist[w * SLAM_RADIUS_BINS + b] = h[b];
}

// one block per long list: ghist[tile][bin] -> the list position of the tile's first entry of that distance
__global__ __launch_bounds__(256) void bf_radius_sort_scan_kernel(const int64_t* __restrict__ lq_tile_end, int32_t* __restrict__ ghist) {
    __shared__ int32_t tot[SLAM_RADIUS_BINS + 3];
    const int64_t l = blockIdx.x;
    const int64_t w0 = l ? lq_tile_end[l - 1] : 0, w1 = lq_tile_end[l];
    for (int b = threadIdx.x; b < SLAM_RADIUS_BINS; b += 256) {
        int32_t run = 0;
        for (int64_t w = w0; w < w1; w++) {
            int32_t* c = ghist + w * SLAM_RADIUS_BINS + b;
            const int32_t v = *c;
            *c = run;
            run += v;
        }
        tot[b] = run;
    }
    __syncthreads();
    if (threadIdx.x < 64) wave_excl_scan_bins(tot);
    __syncthreads();
    for (int b = threadIdx.x; b < SLAM_RADIUS_BINS; b += 256) {
        const int32_t add = tot[b];
        for (int64_t w = w0; w < w1; w++) ghist[w * SLAM_RADIUS_BINS + b] += add;
    }
}

// one wave per tile of a long list: the stable scatter from the positions of bf_radius_sort_scan_kernel
__global__ __launch_bounds__(256) void bf_radius_sort_scatter_kernel(const int2* __restrict__ stage, const int64_t* __restrict__ offsets,
                                                                     const int32_t* __restrict__ lq_id, const int64_t* __restrict__ lq_tile_end,
                                                                     int64_t L, int64_t tiles, const int32_t* __restrict__ ghist,
                                                                     int32_t* __restrict__ idx, int32_t* __restrict__ dist) {
    __shared__ int32_t hist[4][SLAM_RADIUS_BINS + 3];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + wave;
    if (w >= tiles) return;
    int64_t first;
    const int q = lq_id[radius_find_tile(lq_tile_end, L, w, &first)];
    const int64_t o = offsets[q], n = offsets[q + 1] - o;
    const int64_t s = (w - first) * SLAM_RADIUS_SHORT;
    int32_t* h = hist[wave];
    for (int b = lane; b < SLAM_RADIUS_BINS; b += 64) h[b] = ghist[w * SLAM_RADIUS_BINS + b];
    bf_wave_lds_sync();
    wave_stable_scatter(h, stage + o + s, (int)min((int64_t)SLAM_RADIUS_SHORT, n - s), idx, dist, o);
}

// ---- host side -----------------------------------------------------------

struct radius_plan {
    int qblocks;      // grid.x
    int chunks;       // grid.y
    int64_t chunk;    // rows per chunk
    int resident;     // blocks per CU counted on
    int64_t ws;       // bytes of the chunk count table
};

// A pure function of the CU count and the shape (slam_bf_radius_plan_describe exposes it without a device): the top-k
// search's rule (bf_chunk_rule), chunks of at least one tile and under the count table's cap, over ALL train rows: the
// row index is a plain int32 here, so there are no passes.
static radius_plan radius_plan_core(int num_cu, int resident, int64_t N, int64_t M) {
    radius_plan p;
    p.resident = resident;
    const int64_t per = N * 4;                                      // one chunk's counts
    const bf_chunks c = bf_chunk_rule(num_cu, resident, N, M, SLAM_RADIUS_MIN_CHUNK, per, SLAM_RADIUS_WS_CAP);
    p.qblocks = c.qblocks;
    p.chunks = c.chunks;
    p.chunk = c.chunk;
    p.ws = (int64_t)p.chunks * per;
    return p;
}

extern "C" int slam_bf_radius_plan_describe(int num_cu, int64_t N, int64_t M, int32_t* h_plan) {
    SLAM_REQUIRE(h_plan, "slam_bf_radius_plan_describe: null h_plan");
    SLAM_REQUIRE(num_cu >= 1 && num_cu <= 65536, "num_cu=%d out of range", num_cu);
    SLAM_REQUIRE(N >= 0 && M >= 0 && N <= (1ll << 30) && M <= 0x7FFFFFFFll, "bad sizes (N=%lld, M=%lld)", (long long)N, (long long)M);
    const radius_plan p = radius_plan_core(num_cu, SLAM_RADIUS_RESIDENT, N, M);
    const int32_t v[SLAM_RADIUS_PLAN] = {p.qblocks, p.chunks, (int32_t)p.chunk, p.resident, 1,
                                         (int32_t)(p.ws < 0x7FFFFFFF ? p.ws : 0x7FFFFFFF), SLAM_RADIUS_SHORT,
                                         SLAM_RADIUS_BINS};
    memcpy(h_plan, v, sizeof(v));
    return SLAM_OK;
}

// the context's grow-only block for the count table and the scan's arrays (kept apart from slam_workspace, which the
// staging area of the emit step grows once the total is known)
static int radius_tables(slam_ctx* ctx, uint64_t bytes, void** out) {    // (under ctx->call_mu)
    if (bytes > ctx->radius_mem_bytes) {
        SLAM_HIP(hipStreamSynchronize(ctx->stream));
        if (ctx->radius_mem) SLAM_HIP(hipFree(ctx->radius_mem));
        ctx->radius_mem = nullptr;
        ctx->radius_mem_bytes = 0;
        const uint64_t want = bytes + (bytes >> 2);
        SLAM_HIP(hipMalloc(&ctx->radius_mem, want));
        ctx->radius_mem_bytes = want;
    }
    *out = ctx->radius_mem;
    return SLAM_OK;
}

// slam_bf_radius_u256 without the call lock
static int radius_search(slam_ctx* ctx, const void* d_query, int64_t N, const void* d_train, int64_t M, float max_distance,
                         int64_t train_base, int64_t* d_offsets, int64_t capacity, int32_t* d_idx, int32_t* d_dist,
                         int64_t* h_total) {
    SLAM_REQUIRE(ctx, "slam_bf_radius_u256: null ctx");
    SLAM_REQUIRE(N >= 0 && M >= 0 && capacity >= 0, "negative size (N=%lld, M=%lld, capacity=%lld)", (long long)N, (long long)M,
                 (long long)capacity);
    SLAM_REQUIRE(N <= (1ll << 30), "N=%lld exceeds 2^30 query rows per call", (long long)N);
    SLAM_REQUIRE(train_base >= 0 && train_base + M <= 0x7FFFFFFFll, "train_base + M must fit int32");
    SLAM_REQUIRE(d_offsets && h_total, "slam_bf_radius_u256: null offsets or total pointer");
    SLAM_REQUIRE(N == 0 || d_query, "slam_bf_radius_u256: null query pointer");
    SLAM_REQUIRE(N == 0 || M == 0 || d_train, "slam_bf_radius_u256: null train pointer");
    SLAM_REQUIRE(capacity == 0 || (d_idx && d_dist), "slam_bf_radius_u256: null result pointer");
    SLAM_REQUIRE(((uintptr_t)d_query & 15) == 0 && ((uintptr_t)d_train & 15) == 0, "descriptor pointers must be 16-byte aligned");
    SLAM_REQUIRE(((uintptr_t)d_offsets & 7) == 0 && ((uintptr_t)d_idx & 3) == 0 && ((uintptr_t)d_dist & 3) == 0,
                 "offsets must be 8-byte and result pointers 4-byte aligned");
    SLAM_HIP(hipSetDevice(ctx->device));
    const int th = slam_bf_radius_threshold(max_distance);
    *h_total = 0;
    if (N == 0 || M == 0 || th == 0) {                               // N + 1 zero offsets, nothing to emit
        SLAM_HIP(hipMemsetAsync(d_offsets, 0, (size_t)(N + 1) * sizeof(int64_t), ctx->stream));
        SLAM_HIP(hipStreamSynchronize(ctx->stream));
        return SLAM_OK;
    }
    static std::atomic<int> once{0};
    int occ = 0;
    if (int rc = slam_occupancy_once((const void*)bf_radius_scan_kernel<false>, &once, &occ)) return rc;
    const radius_plan p = radius_plan_core(ctx->num_cu, occ < SLAM_RADIUS_RESIDENT ? occ : SLAM_RADIUS_RESIDENT, N, M);
    // tables: counts [chunks][N] i32 | len [N] i32 | bsum [B][3] i64 | tot [3] i64 | lq_id [N] i32 | lq_tile_end [N] i64
    const int64_t B = (N + 255) / 256;
    const uint64_t o_len = slam_align_up((uint64_t)p.ws), o_bsum = o_len + slam_align_up(N * 4ull),
                   o_tot = o_bsum + slam_align_up(B * 24ull), o_lq = o_tot + 256, o_lqe = o_lq + slam_align_up(N * 4ull),
                   tbytes = o_lqe + slam_align_up(N * 8ull);
    void* tmem = nullptr;
    if (int rc = radius_tables(ctx, tbytes, &tmem)) return rc;
    char* tb = (char*)tmem;
    int32_t* cnt = (int32_t*)tb;
    int32_t* len = (int32_t*)(tb + o_len);
    int64_t* bsum = (int64_t*)(tb + o_bsum);
    int64_t* tot = (int64_t*)(tb + o_tot);
    int32_t* lq_id = (int32_t*)(tb + o_lq);
    int64_t* lq_tile_end = (int64_t*)(tb + o_lqe);

    radius_args a;
    a.q = (const uint4*)d_query;
    a.t = (const uint4*)d_train;
    a.N = (int)N;
    a.M = M;
    a.chunk = p.chunk;
    a.init = SLAM_ACC_BIAS - (u32)th;
    a.train_base = (int)train_base;
    a.cnt = cnt;
    a.off = d_offsets;
    a.stage = nullptr;
    const dim3 grid(p.qblocks, p.chunks), block(256);
    SLAM_HIP(hipGetLastError());
    if (int rc = slam_prof_begin(ctx)) return rc;
    bf_radius_scan_kernel<false><<<grid, block, 0, ctx->stream>>>(a);
    if (int rc = slam_prof_end(ctx)) return rc;
    bf_radius_prefix_kernel<<<dim3((unsigned)B), block, 0, ctx->stream>>>(cnt, p.chunks, (int)N, len, bsum);
    bf_radius_blocks_kernel<<<dim3(1), block, 0, ctx->stream>>>(bsum, B, tot, d_offsets, (int)N);
    bf_radius_offsets_kernel<<<dim3((unsigned)B), block, 0, ctx->stream>>>(len, (int)N, bsum, d_offsets, lq_id, lq_tile_end);
    if (int rc = slam_launch_check("radius count")) return rc;
    int64_t h_tot[3] = {0, 0, 0};                                    // entries, long lists, tiles of long lists
    SLAM_HIP(hipMemcpyAsync(h_tot, tot, sizeof(h_tot), hipMemcpyDeviceToHost, ctx->stream));
    SLAM_HIP(hipStreamSynchronize(ctx->stream));
    *h_total = h_tot[0];
    if (h_tot[0] == 0 || h_tot[0] > capacity) return SLAM_OK;        // "too small" is a total, not an error

    // staging area [total] int2 | long-list tile histograms [tiles][257] i32, in the context's workspace
    const int64_t T = h_tot[0], L = h_tot[1], tiles = h_tot[2];
    const uint64_t o_hist = slam_align_up((uint64_t)T * 8);
    void* ws = nullptr;
    if (int rc = slam_workspace(ctx, o_hist + (uint64_t)tiles * SLAM_RADIUS_BINS * 4, &ws)) return rc;
    int2* stage = (int2*)ws;
    int32_t* ghist = (int32_t*)((char*)ws + o_hist);
    a.stage = stage;
    bf_radius_scan_kernel<true><<<grid, block, 0, ctx->stream>>>(a);
    bf_radius_sort_short_kernel<<<dim3((unsigned)((N + 3) / 4)), block, 0, ctx->stream>>>(stage, d_offsets, (int)N, d_idx, d_dist);
    if (L > 0) {
        const dim3 tg((unsigned)((tiles + 3) / 4));
        bf_radius_sort_hist_kernel<<<tg, block, 0, ctx->stream>>>(stage, d_offsets, lq_id, lq_tile_end, L, tiles, ghist);
        bf_radius_sort_scan_kernel<<<dim3((unsigned)L), block, 0, ctx->stream>>>(lq_tile_end, ghist);
        bf_radius_sort_scatter_kernel<<<tg, block, 0, ctx->stream>>>(stage, d_offsets, lq_id, lq_tile_end, L, tiles, ghist, d_idx, d_dist);
    }
    return slam_launch_check("radius emit / sort");
}

extern "C" int slam_bf_radius_u256(slam_ctx* ctx, const void* d_query, int64_t N, const void* d_train, int64_t M, float max_distance,
                                   int64_t train_base, int64_t* d_offsets, int64_t capacity, int32_t* d_idx, int32_t* d_dist,
                                   int64_t* h_total) {
    SLAM_REQUIRE(ctx, "slam_bf_radius_u256: null ctx");
    std::lock_guard<std::mutex> lk(ctx->call_mu);
    return radius_search(ctx, d_query, N, d_train, M, max_distance, train_base, d_offsets, capacity, d_idx, d_dist, h_total);
}

// upload, search, download, one stream synchronisation (through the context's host-buffer arena)
extern "C" int slam_bf_radius_u256_host(slam_ctx* ctx, const uint8_t* h_query, int64_t N, const uint8_t* h_train, int64_t M,
                                        float max_distance, int64_t* h_offsets, int64_t capacity, int32_t* h_idx, int32_t* h_dist,
                                        int64_t* h_total) {
    SLAM_REQUIRE(ctx, "slam_bf_radius_u256_host: null ctx");
    SLAM_REQUIRE(N >= 0 && M >= 0 && capacity >= 0 && N <= (1ll << 28) && M <= (1ll << 28), "bad sizes N=%lld M=%lld capacity=%lld",
                 (long long)N, (long long)M, (long long)capacity);
    SLAM_REQUIRE(h_offsets && h_total && (h_query || N == 0) && (h_train || M == 0) && (capacity == 0 || (h_idx && h_dist)),
                 "slam_bf_radius_u256_host: null host pointer");
    std::lock_guard<std::mutex> lk(ctx->call_mu);
    SLAM_HIP(hipSetDevice(ctx->device));
    const int64_t cap = capacity < N * M ? capacity : N * M;         // (no list holds more than M entries)
    const uint64_t qbytes = (uint64_t)N * SLAM_DESC_BYTES, tbytes = (uint64_t)M * SLAM_DESC_BYTES, obytes = (uint64_t)(N + 1) * 8,
                   rbytes = (uint64_t)cap * 4;
    const uint64_t off_t = slam_align_up(qbytes), off_o = off_t + slam_align_up(tbytes), off_i = off_o + slam_align_up(obytes),
                   off_d = off_i + slam_align_up(rbytes), total = off_d + slam_align_up(rbytes);
    void *dev = nullptr, *host = nullptr;
    if (int rc = slam_io_arena(ctx, total, total, &dev, &host)) return rc;
    uint8_t* hb = (uint8_t*)host;
    uint8_t* db = (uint8_t*)dev;
    if (qbytes) memcpy(hb, h_query, qbytes);
    if (tbytes) memcpy(hb + off_t, h_train, tbytes);
    ctx->io_h2d_bytes += qbytes + tbytes;
    if (qbytes + tbytes) SLAM_HIP(hipMemcpyAsync(db, hb, off_t + tbytes, hipMemcpyHostToDevice, ctx->stream));
    if (int rc = radius_search(ctx, db, N, db + off_t, M, max_distance, 0, (int64_t*)(db + off_o), cap, (int32_t*)(db + off_i),
                                     (int32_t*)(db + off_d), h_total))
        return rc;
    const int64_t T = *h_total <= cap ? *h_total : 0;                // (beyond the capacity only the offsets come back)
    SLAM_HIP(hipMemcpyAsync(hb + off_o, db + off_o, obytes, hipMemcpyDeviceToHost, ctx->stream));
    if (T) {
        SLAM_HIP(hipMemcpyAsync(hb + off_i, db + off_i, (size_t)T * 4, hipMemcpyDeviceToHost, ctx->stream));
        SLAM_HIP(hipMemcpyAsync(hb + off_d, db + off_d, (size_t)T * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    SLAM_HIP(hipStreamSynchronize(ctx->stream));
    ctx->io_d2h_bytes += obytes + 8 * (uint64_t)T;
    memcpy(h_offsets, hb + off_o, obytes);
    if (T) {
        memcpy(h_idx, hb + off_i, (size_t)T * 4);
        memcpy(h_dist, hb + off_d, (size_t)T * 4);
    }
    return SLAM_OK;
}
