// loop_detect.hip — loop and relocalisation candidates (slam_loop_*): the covisibility-group stage of ORB-SLAM's
// KeyFrameDatabase::DetectLoopCandidates / DetectRelocalizationCandidates over the dense tables slam_bow_query leaves on the
// device and a table of best covisibles.  The reference detects no loops: PARITY UNPINNED.
//
// Every kernel but `exclude` runs on the grid (tiles of LP_TILE entries, Q queries), a thread on LP_PER entries a stride of
// the workgroup apart (coalesced rows):
//   exclude   a thread per entry of the excluded lists: its bit in the query's excluded bitmap, and for a derived min_s the
//             greatest ~s over the excluded entries other than the query's own (a maximum, so the least s).
//   cmax      the greatest common over the entries that share: a reduction per workgroup, one atomicMax.
//   acc       per candidate the nb gathers of its row of d_best into the query's rows of d_s / d_common; acc, gbest and the
//             greatest acc (one 64-bit atomicMax a workgroup).  The row is not staged: a workgroup holds 1 024 of its entries
//             and gathers from all of it, the tiles of a query would each stage the whole row, and 40 KiB a row stays in L2.
//   retain    a candidate with 4 acc > 3 acc_max sets the bit of its gbest in the result bitmap (atomicOr: duplicates fold).
//   count     the set bits of every (tile, query); the host sums them.
//   fill      the tiles in front are summed, the 32 words of the tile scanned in one wave, every set bit written to its slot
//             with its own s - ascending, no atomics.
//
// Integers only.  Atomics take a maximum, set bits or count: two runs give the same bytes.  The workspace is the caller's
// (slam_loop_workspace); nothing here takes a block of the context.
#include "internal.h"

#define LP_THREADS 256
#define LP_PER 4                                // entries a thread takes
#define LP_TILE (LP_THREADS * LP_PER)           // entries of a workgroup: 32 words of a bitmap row
#define LP_TILE_WORDS (LP_TILE / 32)
#define LP_NB_MAX 16
#define LP_QUERIES_MAX 65535
#define LP_ENTRIES_MAX (1ll << 24)
#define LP_EXCL_MAX ((1ll << 31) - 1)
#define LP_SCAL_BYTES 256                       // the scalar block at the head of the workspace: uint32 [64], [0] = indices skipped
#define LP_DERIVE 0xFFFFFFFFu
#define LP_NO_CONNECTED 0x80000000u             // the derived min_s of a query without a connected entry: 2^31 = a score of 1

typedef unsigned long long lp_u64;

#define LP_AT(T, ws, off) ((T*)((char*)(ws) + (off)))

struct lp_par {                                 // what the host says about a query
    int32_t own, limit;
    uint32_t min_s, pad;
};

struct lp_state {                               // what the kernels learn about it (zeroed by the call)
    lp_u64 acc_max;
    lp_u64 inv_min;                             // 1 + the greatest ~s over the connected entries, 0 = none
    int32_t cmax, pad[3];
};

struct lp_tables {
    const uint32_t* s;                          // [Q,E]
    const int32_t* common;                      // [Q,E]
    const int32_t* best;                        // [E,nb]
    const uint32_t* excl;                       // [Q,W] or null (relocalisation)
    const lp_par* par;                          // [Q]
    lp_state* state;                            // [Q]
    int64_t E, W;
    int nb, mode;
};

__device__ __forceinline__ void lp_index_error(unsigned* scal, unsigned* index_errors) {
    atomicAdd(&scal[0], 1u);
    atomicAdd(index_errors, 1u);
}

// the last q in [0, Q) with off[q] <= e (off[0] = 0 <= e)
__device__ __forceinline__ int lp_owner(const int64_t* off, int Q, int64_t e) {
    int lo = 0, hi = Q;
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (off[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

// step 1 of the specification; i in [0, E)
__device__ __forceinline__ bool lp_shares(const lp_tables& t, int q, int64_t i, int limit) {
    if (i >= limit) return false;
    if (t.excl && (t.excl[(int64_t)q * t.W + (i >> 5)] >> (i & 31) & 1u)) return false;
    return t.common[(int64_t)q * t.E + i] > 0;
}

// step 2: 5 common > 4 cmax
__device__ __forceinline__ bool lp_words_ok(const lp_tables& t, int q, int64_t i, int limit, int cmax) {
    return lp_shares(t, q, i, limit) && 5ll * t.common[(int64_t)q * t.E + i] > 4ll * cmax;
}

__device__ __forceinline__ uint32_t lp_min_s(const lp_tables& t, int q) {
    if (t.mode == 1) return 0u;
    const uint32_t m = t.par[q].min_s;
    if (m != LP_DERIVE) return m;
    const lp_u64 inv = t.state[q].inv_min;
    return inv ? ~(uint32_t)(inv - 1) : LP_NO_CONNECTED;
}

__global__ __launch_bounds__(LP_THREADS) void lp_exclude(const int32_t* excl_ids, const int64_t* off, int Q, int64_t n, const uint32_t* s,
                                                         const lp_par* par, lp_state* state, uint32_t* excl, int64_t E, int64_t W, unsigned* scal,
                                                         unsigned* index_errors) {
    const int64_t e = (int64_t)blockIdx.x * LP_THREADS + threadIdx.x;
    if (e >= n) return;
    const int q = lp_owner(off, Q, e);
    const int j = excl_ids[e];
    if (j < 0 || j >= E) {                                     // counted, never dereferenced
        lp_index_error(scal, index_errors);
        return;
    }
    atomicOr(&excl[(int64_t)q * W + (j >> 5)], 1u << (j & 31));                  // idempotent: an id listed twice sets a bit once
    if (par[q].min_s == LP_DERIVE && j != par[q].own)
        atomicMax(&state[q].inv_min, (lp_u64)(~s[(int64_t)q * E + j]) + 1ull);   // a maximum: the order of arrival does not show
}

// the maximum of v over the workgroup, in thread 0
template <typename T>
__device__ __forceinline__ T lp_block_max(T v, T* wmax) {
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const T other = __shfl_xor(v, off, 64);
        v = other > v ? other : v;
    }
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = v;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < LP_THREADS / 64; ++k) v = wmax[k] > v ? wmax[k] : v;
    return v;
}

__global__ __launch_bounds__(LP_THREADS) void lp_cmax(const lp_tables t) {
    __shared__ int wmax[LP_THREADS / 64];
    const int q = blockIdx.y, limit = t.par[q].limit;
    int c = 0;
#pragma unroll
    for (int k = 0; k < LP_PER; ++k) {
        const int64_t i = (int64_t)blockIdx.x * LP_TILE + k * LP_THREADS + threadIdx.x;
        if (i < t.E && lp_shares(t, q, i, limit)) {
            const int v = t.common[(int64_t)q * t.E + i];
            c = v > c ? v : c;
        }
    }
    c = lp_block_max(c, wmax);
    if (threadIdx.x == 0 && c > 0) atomicMax(&t.state[q].cmax, c);
}

__global__ __launch_bounds__(LP_THREADS) void lp_acc(const lp_tables t, lp_u64* acc_out, int32_t* gbest_out, unsigned* scal, unsigned* index_errors) {
    __shared__ lp_u64 wmax[LP_THREADS / 64];
    const int q = blockIdx.y, limit = t.par[q].limit, cmax = t.state[q].cmax;
    const uint32_t min_s = lp_min_s(t, q);
    const uint32_t* s = t.s + (int64_t)q * t.E;
    lp_u64 top = 0;
#pragma unroll
    for (int k = 0; k < LP_PER; ++k) {
        const int64_t i = (int64_t)blockIdx.x * LP_TILE + k * LP_THREADS + threadIdx.x;
        if (i >= t.E) continue;
        lp_u64 acc = 0;
        int32_t gbest = -1;
        if (cmax > 0 && lp_words_ok(t, q, i, limit, cmax) && s[i] >= min_s) {
            uint32_t bs = s[i];
            acc = bs;
            gbest = (int32_t)i;
            for (int n = 0; n < t.nb; ++n) {
                const int j = t.best[i * t.nb + n];
                if (j < 0) continue;                           // padding
                if (j >= t.E) {                                // counted, never dereferenced
                    lp_index_error(scal, index_errors);
                    continue;
                }
                if (!lp_words_ok(t, q, j, limit, cmax)) continue;
                const uint32_t sj = s[j];
                acc += sj;
                if (sj > bs) {                                 // ties: the candidate, then the earlier position
                    bs = sj;
                    gbest = j;
                }
            }
        }
        acc_out[(int64_t)q * t.E + i] = acc;
        gbest_out[(int64_t)q * t.E + i] = gbest;
        top = acc > top ? acc : top;
    }
    top = lp_block_max(top, wmax);
    if (threadIdx.x == 0 && top) atomicMax(&t.state[q].acc_max, top);
}

__global__ __launch_bounds__(LP_THREADS) void lp_retain(const lp_u64* acc, const int32_t* gbest, const lp_state* state, int64_t E, int64_t W,
                                                        uint32_t* bitmap) {
    const int q = blockIdx.y;
    const lp_u64 acc_max = state[q].acc_max;
#pragma unroll
    for (int k = 0; k < LP_PER; ++k) {
        const int64_t i = (int64_t)blockIdx.x * LP_TILE + k * LP_THREADS + threadIdx.x;
        if (i >= E) continue;
        const int g = gbest[(int64_t)q * E + i];
        if (g < 0 || g >= E) continue;                         // (no candidate; gbest is an entry by construction)
        if (4ull * acc[(int64_t)q * E + i] > 3ull * acc_max) atomicOr(&bitmap[(int64_t)q * W + (g >> 5)], 1u << (g & 31));
    }
}

// wave 0 of a workgroup holds the 32 words of its tile, a lane a word; n = the set bits of the lane's word
__device__ __forceinline__ uint32_t lp_tile_word(const uint32_t* bitmap, int64_t W, int q, int64_t* word_at) {
    const int64_t w = (int64_t)blockIdx.x * LP_TILE_WORDS + threadIdx.x;
    *word_at = w;
    return (threadIdx.x < LP_TILE_WORDS && w < W) ? bitmap[(int64_t)q * W + w] : 0u;
}

__global__ __launch_bounds__(64) void lp_count(const uint32_t* bitmap, int64_t W, int tiles, uint32_t* tilecount) {
    const int q = blockIdx.y;
    int64_t w;
    unsigned n = __popc(lp_tile_word(bitmap, W, q, &w));
#pragma unroll
    for (int off = 32; off; off >>= 1) n += __shfl_xor(n, off, 64);
    if (threadIdx.x == 0) tilecount[(int64_t)q * tiles + blockIdx.x] = n;
}

__global__ __launch_bounds__(64) void lp_fill(const uint32_t* bitmap, const uint32_t* s, int64_t E, int64_t W, int tiles, const uint32_t* tilecount,
                                              const int64_t* out_off, int64_t total, int32_t* ids, uint32_t* scores) {
    const int q = blockIdx.y, lane = threadIdx.x;
    unsigned front = 0;
    for (int k = lane; k < (int)blockIdx.x; k += 64) front += tilecount[(int64_t)q * tiles + k];
#pragma unroll
    for (int off = 32; off; off >>= 1) front += __shfl_xor(front, off, 64);
    int64_t w;
    uint32_t v = lp_tile_word(bitmap, W, q, &w);
    const unsigned n = __popc(v);
    unsigned inc = n;                                          // inclusive scan of the word counts
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned up = __shfl_up(inc, off, 64);
        if (lane >= off) inc += up;
    }
    if (out_off[q] < 0) return;
    const int64_t end = out_off[q + 1] < total ? out_off[q + 1] : total;
    int64_t pos = out_off[q] + front + inc - n;
    while (v) {
        const int64_t i = w * 32 + (__ffs(v) - 1);
        if (pos < end && i < E) {                              // never store outside the query's slice
            ids[pos] = (int32_t)i;
            scores[pos] = s[(int64_t)q * E + i];
        }
        ++pos;
        v &= v - 1;
    }
}

// ---- the host side ----------------------------------------------------------------------------------------------------------------
extern "C" int slam_loop_limits(int32_t* h_limits) {
    SLAM_REQUIRE(h_limits, "slam_loop_limits: null limits");
    h_limits[0] = LP_THREADS;
    h_limits[1] = LP_TILE;
    h_limits[2] = LP_NB_MAX;
    h_limits[3] = LP_QUERIES_MAX;
    return SLAM_OK;
}

struct lp_layout {
    int64_t W;
    int tiles;
    uint64_t off, par, state, excl, tilecount, out_off, bytes;
    uint64_t state_bytes, excl_bytes;
};

static int lp_sizes(const char* who, int64_t Q, int64_t E) {
    SLAM_REQUIRE(Q >= 0 && Q <= LP_QUERIES_MAX && E >= 1 && E <= LP_ENTRIES_MAX, "%s: bad sizes (Q=%lld, E=%lld)", who, (long long)Q, (long long)E);
    return SLAM_OK;
}

static lp_layout lp_lay(int64_t Q, int64_t E) {
    lp_layout y = {};
    const uint64_t q1 = (uint64_t)(Q > 0 ? Q : 1);
    y.W = (E + 31) / 32;
    y.tiles = (int)((E + LP_TILE - 1) / LP_TILE);
    y.off = LP_SCAL_BYTES;                                     // offsets and parameters lie together: one copy brings both
    y.par = y.off + slam_align_up((q1 + 1) * 8);
    y.state = y.par + slam_align_up(q1 * sizeof(lp_par));
    y.state_bytes = slam_align_up(q1 * sizeof(lp_state));
    y.excl = y.state + y.state_bytes;
    y.excl_bytes = slam_align_up(q1 * (uint64_t)y.W * 4);
    y.tilecount = y.excl + y.excl_bytes;
    y.out_off = y.tilecount + slam_align_up(q1 * (uint64_t)y.tiles * 4);
    y.bytes = y.out_off + slam_align_up((q1 + 1) * 8);
    return y;
}

extern "C" int slam_loop_workspace(int64_t Q, int64_t E, uint64_t* h_bytes) {
    SLAM_REQUIRE(h_bytes, "slam_loop_workspace: null bytes");
    if (int rc = lp_sizes("slam_loop_workspace", Q, E)) return rc;
    *h_bytes = lp_lay(Q, E).bytes;
    return SLAM_OK;
}

static int lp_check_offsets(const char* who, const char* what, const int64_t* off, int64_t n, int64_t limit) {
    SLAM_REQUIRE(off && off[0] == 0, "%s: null %s offsets, or offsets that do not start at 0", who, what);
    for (int64_t i = 0; i < n; ++i) SLAM_REQUIRE(off[i + 1] >= off[i], "%s: the %s offsets descend at %lld", who, what, (long long)i);
    SLAM_REQUIRE(off[n] <= limit, "%s: the %s offsets end at %lld, past %lld", who, what, (long long)off[n], (long long)limit);
    return SLAM_OK;
}

extern "C" int slam_loop_candidates(slam_ctx* ctx, int64_t Q, int64_t E, const uint32_t* d_s, const int32_t* d_common, int nb, const int32_t* d_best,
                                    const int32_t* d_excl, const int64_t* h_excl_offsets, const int32_t* h_own, const int32_t* h_limit,
                                    const uint32_t* h_min_s, int mode, void* d_ws, uint64_t* d_acc, int32_t* d_gbest, uint32_t* d_bitmap,
                                    int64_t* h_counts, int64_t* h_skipped) {
    const char* who = "slam_loop_candidates";
    SLAM_REQUIRE(ctx, "%s: null ctx", who);
    SLAM_REQUIRE(mode == 0 || mode == 1, "%s: mode %d is not 0 (loop) or 1 (relocalisation)", who, mode);
    SLAM_REQUIRE(nb >= 0 && nb <= LP_NB_MAX, "%s: nb=%d outside [0, %d]", who, nb, LP_NB_MAX);
    if (int rc = lp_sizes(who, Q, E)) return rc;
    if (h_skipped) *h_skipped = 0;
    if (Q == 0) return SLAM_OK;
    SLAM_REQUIRE(h_counts, "%s: null counts", who);
    int64_t n_excl = 0;
    if (mode == 0) {
        SLAM_REQUIRE(h_own, "%s: null own ids", who);
        if (int rc = lp_check_offsets(who, "excluded", h_excl_offsets, Q, LP_EXCL_MAX)) return rc;
        n_excl = h_excl_offsets[Q];
    }
    for (int64_t q = 0; h_limit && q < Q; ++q)
        SLAM_REQUIRE(h_limit[q] >= 0 && h_limit[q] <= E, "%s: limit[%lld] = %d outside [0, %lld]", who, (long long)q, h_limit[q], (long long)E);
    SLAM_REQUIRE(d_s && d_common && d_ws && d_acc && d_gbest && d_bitmap && (nb == 0 || d_best) && (n_excl == 0 || d_excl), "%s: null device pointer", who);
    SLAM_REQUIRE(((uintptr_t)d_acc & 7) == 0 && ((uintptr_t)d_ws & 7) == 0, "%s: misaligned pointer", who);
    const lp_layout y = lp_lay(Q, E);
    // offsets and parameters in one block, as they lie in the workspace
    std::vector<char> h((size_t)(y.state - y.off), 0);
    int64_t* off = (int64_t*)h.data();
    lp_par* par = (lp_par*)(h.data() + (y.par - y.off));
    for (int64_t q = 0; q < Q; ++q) {
        off[q] = mode == 0 ? h_excl_offsets[q] : 0;
        par[q].own = mode == 0 ? h_own[q] : -1;
        par[q].limit = h_limit ? h_limit[q] : (int32_t)E;
        par[q].min_s = mode == 0 ? (h_min_s ? h_min_s[q] : LP_DERIVE) : 0u;
        par[q].pad = 0;
    }
    off[Q] = n_excl;
    SLAM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    unsigned *scal = (unsigned*)d_ws, *ie = slam_index_error_counter(ctx);
    lp_tables t;
    t.s = d_s;
    t.common = d_common;
    t.best = d_best;
    t.excl = mode == 0 ? LP_AT(const uint32_t, d_ws, y.excl) : nullptr;
    t.par = LP_AT(const lp_par, d_ws, y.par);
    t.state = LP_AT(lp_state, d_ws, y.state);
    t.E = E;
    t.W = y.W;
    t.nb = nb;
    t.mode = mode;
    uint32_t* tilecount = LP_AT(uint32_t, d_ws, y.tilecount);
    SLAM_HIP(hipMemsetAsync(d_ws, 0, LP_SCAL_BYTES, st));
    SLAM_HIP(hipMemcpyAsync(LP_AT(char, d_ws, y.off), h.data(), h.size(), hipMemcpyHostToDevice, st));      // (pageable: it has left h on return)
    SLAM_HIP(hipMemsetAsync(t.state, 0, y.state_bytes + (mode == 0 ? y.excl_bytes : 0), st));               // the state and the excluded bitmap behind it
    SLAM_HIP(hipMemsetAsync(d_bitmap, 0, (size_t)(Q * y.W) * 4, st));
    const dim3 grid((unsigned)y.tiles, (unsigned)Q);
    if (n_excl)
        lp_exclude<<<(unsigned)((n_excl + LP_THREADS - 1) / LP_THREADS), LP_THREADS, 0, st>>>(d_excl, LP_AT(const int64_t, d_ws, y.off), (int)Q, n_excl, d_s, t.par, t.state,
                                                                                            LP_AT(uint32_t, d_ws, y.excl), E, y.W, scal, ie);
    lp_cmax<<<grid, LP_THREADS, 0, st>>>(t);
    lp_acc<<<grid, LP_THREADS, 0, st>>>(t, (lp_u64*)d_acc, d_gbest, scal, ie);
    lp_retain<<<grid, LP_THREADS, 0, st>>>((const lp_u64*)d_acc, d_gbest, t.state, E, y.W, d_bitmap);
    lp_count<<<grid, 64, 0, st>>>(d_bitmap, y.W, y.tiles, tilecount);
    if (int rc = slam_launch_check(who)) return rc;
    std::vector<uint32_t> hc((size_t)Q * y.tiles);
    uint32_t skipped = 0;
    SLAM_HIP(hipMemcpyAsync(hc.data(), tilecount, hc.size() * 4, hipMemcpyDeviceToHost, st));
    SLAM_HIP(hipMemcpyAsync(&skipped, d_ws, 4, hipMemcpyDeviceToHost, st));
    SLAM_HIP(hipStreamSynchronize(st));
    for (int64_t q = 0; q < Q; ++q) {
        int64_t n = 0;
        for (int k = 0; k < y.tiles; ++k) n += hc[(size_t)(q * y.tiles + k)];
        h_counts[q] = n;
    }
    if (h_skipped) *h_skipped = skipped;
    return SLAM_OK;
}

extern "C" int slam_loop_fill(slam_ctx* ctx, int64_t Q, int64_t E, const uint32_t* d_s, const uint32_t* d_bitmap, void* d_ws,
                              const int64_t* h_out_offsets, int32_t* d_ids, uint32_t* d_scores) {
    const char* who = "slam_loop_fill";
    SLAM_REQUIRE(ctx, "%s: null ctx", who);
    if (int rc = lp_sizes(who, Q, E)) return rc;
    if (Q == 0) return SLAM_OK;
    if (int rc = lp_check_offsets(who, "output", h_out_offsets, Q, Q * E)) return rc;
    const int64_t total = h_out_offsets[Q];
    SLAM_REQUIRE(d_ws && d_bitmap && d_s && (total == 0 || (d_ids && d_scores)), "%s: null device pointer", who);
    if (total == 0) return SLAM_OK;
    const lp_layout y = lp_lay(Q, E);
    SLAM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int64_t* out_off = LP_AT(int64_t, d_ws, y.out_off);
    SLAM_HIP(hipMemcpyAsync(out_off, h_out_offsets, (size_t)(Q + 1) * 8, hipMemcpyHostToDevice, st));
    lp_fill<<<dim3((unsigned)y.tiles, (unsigned)Q), 64, 0, st>>>(d_bitmap, d_s, E, y.W, y.tiles, LP_AT(const uint32_t, d_ws, y.tilecount), out_off, total, d_ids,
                                                                 d_scores);
    return slam_launch_check(who);
}
