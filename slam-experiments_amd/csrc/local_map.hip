// local_map.hip — which part of the map a step runs on (slam_lmap_*): Tracking::UpdateLocalKeyFrames' vote,
// UpdateLocalPoints and LocalMapping::KeyFrameCulling over the tables a fuse_points call leaves on the device.
//
//   frame_points   a thread per slot of obs: the inverse table row -> point (atomicMax: the greatest claimant stays, whatever
//                  the order; a second claimant of a row is counted and the caller refuses the table).
//   vote           a workgroup per query frame, a thread per tracked point, the F counters in LDS (4 096 or 40 448 of them:
//                  16 KiB keeps ten workgroups on a CU, 158 KiB is what one workgroup may have); above that the counters are
//                  the rows of d_votes themselves.  The arg-max is a reduction over the key votes << 32 | (2^31 - 1 - frame).
//   points_mark    a workgroup per (query, local keyframe): atomicOr of one bit per point into the caller's bitmap; then a
//                  thread per tracked point clears its bit; then the set bits of every (query, tile of 1 024 words) are counted.
//   points_fill    a workgroup per (query, tile): the tiles in front are summed, the words of the tile scanned, every set bit
//                  written to its slot - ascending in the point, no atomics.
//   cull_count     G lanes per row of a candidate keyframe, G in {16, 64, 256} by the length of the point's observation list
//                  (a launch per class over the same rows; a row belongs to one class), lane k its observation k; the verdicts
//                  of a wave are summed by shuffles and leave in one 64-bit atomic (n_points low, n_redundant high).
//
// Integers only.  Atomics count, or, and, or take a maximum: no output depends on the order they arrive in.  The workspaces
// are the caller's (slam_lmap_workspace); nothing here takes a block of the context.
#include "internal.h"
#include <limits.h>

#define LM_THREADS 256
#define LM_VOTE_LDS_SMALL 4096                  // frames whose counters a workgroup keeps in 16 KiB of LDS
#define LM_VOTE_LDS_FRAMES 40448                // frames whose counters fit the LDS of a CU (158 KiB + the reduction's words)
#define LM_SCAN_WORDS 4                         // bitmap words a thread of a scan tile takes
#define LM_SCAN_TILE (LM_THREADS * LM_SCAN_WORDS)
#define LM_SCAL_BYTES 256                       // the scalar block at the head of a workspace: uint32 [64]
#define LM_OBS_MAX 256
#define LM_POINTS_MAX (1ll << 24)
#define LM_FRAMES_MAX (1ll << 24)
#define LM_QUERIES_MAX 65535
#define LM_ROWS_MAX ((1ll << 31) - 1)
#define LM_CULL_GROUPS_MAX (1ll << 24)          // candidates x rows of the longest: a launch of 256 threads each stays below 2^32 threads

typedef unsigned long long lm_u64;

#define LM_AT(T, ws, off) ((T*)((char*)(ws) + (off)))

static inline int64_t lm_tiles(int64_t n, int64_t tile) { return (n + tile - 1) / tile; }
static inline unsigned lm_grid(int64_t n) { return (unsigned)lm_tiles(n > 0 ? n : 1, LM_THREADS); }

// the last i in [0, n) with off[i] <= s (off[0] <= s): the list a slot lies in
__device__ __forceinline__ int64_t lm_owner(const int64_t* off, int64_t n, int64_t s) {
    int64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= s) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ void lm_index_error(unsigned* scal, unsigned* index_errors) {
    atomicAdd(&scal[0], 1u);
    atomicAdd(index_errors, 1u);
}

// the tables every kernel reads
struct lm_map {
    const int64_t* offsets;        // [M + 1]
    const int2* obs;               // [nnz] (frame, row)
    const uint8_t* bad;            // [M] or null
    const int64_t* fo;             // [F + 1] frame offsets
    const uint8_t* removed;        // [F] or null
    int64_t M, nnz, n_rows;
    int F;
};

// the list of point m, or n = -1 where the offsets would take a read outside obs
__device__ __forceinline__ int lm_list(const lm_map& t, int m, int64_t* start) {
    const int64_t a = t.offsets[m], n = t.offsets[m + 1] - a;
    *start = a;
    return (a < 0 || n < 0 || n > LM_OBS_MAX || a + n > t.nnz) ? -1 : (int)n;
}

// the first row of frame f and the number of its rows, or -1 where the offsets would take a read outside the row tables
__device__ __forceinline__ int64_t lm_rows(const lm_map& t, int f, int64_t* first) {
    const int64_t a = t.fo[f], e = t.fo[f + 1];
    *first = a;
    return (a < 0 || e < a || e > t.n_rows) ? -1 : e - a;
}

// ---- the inverse table ----------------------------------------------------------------------------------------------------------
// scalars: 0 slots out of range, 1 rows claimed twice
__global__ __launch_bounds__(LM_THREADS) void lm_inverse(const lm_map t, int32_t* fp, unsigned* scal, unsigned* index_errors) {
    const int64_t s = (int64_t)blockIdx.x * LM_THREADS + threadIdx.x;
    if (s >= t.nnz) return;
    const int m = (int)lm_owner(t.offsets, t.M, s);
    const int2 o = t.obs[s];
    int64_t first = 0, rows = -1;
    if (o.x >= 0 && o.x < t.F) rows = lm_rows(t, o.x, &first);
    if (rows < 0 || o.y < 0 || o.y >= rows) {                  // counted, never dereferenced
        lm_index_error(scal, index_errors);
        return;
    }
    if (atomicMax(&fp[first + o.y], m) != -1) atomicAdd(&scal[1], 1u);
}

// ---- the vote ---------------------------------------------------------------------------------------------------------------------
// (frame, votes) of the greatest key votes << 32 | (INT_MAX - frame) over the frames with votes, and how many have votes
__device__ __forceinline__ void lm_best(const int32_t* cnt, int F, int32_t* best, int32_t* nvoted) {
    __shared__ long long wkey[LM_THREADS / 64];
    __shared__ int wnz[LM_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    long long key = -1;
    int nz = 0;
    for (int f = tid; f < F; f += LM_THREADS) {
        const int v = cnt[f];
        if (v > 0) {
            const long long k = ((long long)v << 32) | (long long)(INT_MAX - f);
            key = k > key ? k : key;
            ++nz;
        }
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const long long other = __shfl_xor(key, off, 64);
        key = other > key ? other : key;
        nz += __shfl_xor(nz, off, 64);
    }
    if (lane == 0) {
        wkey[w] = key;
        wnz[w] = nz;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int k = 1; k < LM_THREADS / 64; ++k) {
            key = wkey[k] > key ? wkey[k] : key;
            nz += wnz[k];
        }
        best[0] = key < 0 ? -1 : INT_MAX - (int)(key & 0x7fffffffll);
        best[1] = key < 0 ? 0 : (int)(key >> 32);
        *nvoted = nz;
    }
}

// CAP > 0: the counters of the F <= CAP frames in LDS; CAP = 0: the (zeroed) row of d_votes, and lm_vote_best follows
template <int CAP>
__global__ __launch_bounds__(LM_THREADS) void lm_vote(const lm_map t, const int32_t* qpoints, const int64_t* qoff, int64_t Q, int32_t* votes,
                                                      int32_t* best, int32_t* nvoted, unsigned* scal, unsigned* index_errors) {
    __shared__ int32_t lds[CAP > 0 ? CAP : 1];
    const int b = blockIdx.x, tid = threadIdx.x;
    int32_t* row = votes + (int64_t)b * t.F;
    int32_t* cnt = CAP > 0 ? lds : row;
    if (CAP > 0) {
        for (int f = tid; f < t.F; f += LM_THREADS) lds[f] = 0;
        __syncthreads();
    }
    int64_t i0 = qoff[b], i1 = qoff[b + 1];
    if (i0 < 0 || i1 > Q) i0 = i1 = 0;                         // holds by construction; never load outside
    for (int64_t i = i0 + tid; i < i1; i += LM_THREADS) {
        const int m = qpoints[i];
        if (m == -1) continue;
        if (m < 0 || m >= t.M) {
            lm_index_error(scal, index_errors);
            continue;
        }
        if (t.bad && t.bad[m]) continue;
        int64_t s0;
        const int n = lm_list(t, m, &s0);
        if (n < 0) {
            lm_index_error(scal, index_errors);
            continue;
        }
        for (int k = 0; k < n; ++k) {
            const int f = t.obs[s0 + k].x;
            if (f < 0 || f >= t.F) {
                lm_index_error(scal, index_errors);
                continue;
            }
            if (t.removed && t.removed[f]) continue;
            atomicAdd(&cnt[f], 1);                             // a count: the order of arrival does not show
        }
    }
    if (CAP > 0) {
        __syncthreads();
        for (int f = tid; f < t.F; f += LM_THREADS) row[f] = lds[f];
        lm_best(lds, t.F, best + 2 * b, nvoted + b);
    }
}

__global__ __launch_bounds__(LM_THREADS) void lm_vote_best(const int32_t* votes, int F, int32_t* best, int32_t* nvoted) {
    const int b = blockIdx.x;
    lm_best(votes + (int64_t)b * F, F, best + 2 * b, nvoted + b);
}

// ---- local points -----------------------------------------------------------------------------------------------------------------
// a workgroup per entry of the local keyframe lists
__global__ __launch_bounds__(LM_THREADS) void lm_mark(const lm_map t, const int32_t* fp, const int32_t* lkf, const int64_t* lkf_off, int B, int64_t W,
                                                      uint32_t* bitmap, unsigned* scal, unsigned* index_errors) {
    const int64_t e = blockIdx.x;
    const int b = (int)lm_owner(lkf_off, B, e);
    const int f = lkf[e];
    if (f < 0 || f >= t.F) {
        if (threadIdx.x == 0) lm_index_error(scal, index_errors);
        return;
    }
    if (t.removed && t.removed[f]) return;
    int64_t first;
    const int64_t rows = lm_rows(t, f, &first);
    if (rows < 0) {
        if (threadIdx.x == 0) lm_index_error(scal, index_errors);
        return;
    }
    uint32_t* bits = bitmap + (int64_t)b * W;
    for (int64_t r = threadIdx.x; r < rows; r += LM_THREADS) {
        const int m = fp[first + r];
        if (m < 0) continue;
        if (m >= t.M) {
            lm_index_error(scal, index_errors);
            continue;
        }
        if (t.bad && t.bad[m]) continue;
        atomicOr(&bits[m >> 5], 1u << (m & 31));               // idempotent: overlapping keyframes set a bit once
    }
}

// a thread per tracked point: what the query tracks already is not a local point to search for
__global__ __launch_bounds__(LM_THREADS) void lm_clear(const int32_t* qpoints, const int64_t* qoff, int64_t Q, int B, int64_t M, int64_t W,
                                                       uint32_t* bitmap, unsigned* scal, unsigned* index_errors) {
    const int64_t i = (int64_t)blockIdx.x * LM_THREADS + threadIdx.x;
    if (i >= Q) return;
    const int m = qpoints[i];
    if (m == -1) return;
    if (m < 0 || m >= M) {
        lm_index_error(scal, index_errors);
        return;
    }
    const int b = (int)lm_owner(qoff, B, i);
    atomicAnd(&bitmap[(int64_t)b * W + (m >> 5)], ~(1u << (m & 31)));
}

// the sum of v over the workgroup, in every thread
__device__ __forceinline__ unsigned lm_block_sum(unsigned v, unsigned* wsum) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();                                          // (wsum may still be read from an earlier call)
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned all = 0;
#pragma unroll
    for (int k = 0; k < LM_THREADS / 64; ++k) all += wsum[k];
    return all;
}

// grid (T, B): the set bits of tile x of query y
__global__ __launch_bounds__(LM_THREADS) void lm_popcount(const uint32_t* bitmap, int64_t W, int T, uint32_t* tilecount) {
    __shared__ unsigned wsum[LM_THREADS / 64];
    const int b = blockIdx.y, tile = blockIdx.x;
    const uint32_t* bits = bitmap + (int64_t)b * W;
    const int64_t base = (int64_t)tile * LM_SCAN_TILE + (int64_t)threadIdx.x * LM_SCAN_WORDS;
    unsigned s = 0;
#pragma unroll
    for (int k = 0; k < LM_SCAN_WORDS; ++k)
        if (base + k < W) s += __popc(bits[base + k]);
    const unsigned all = lm_block_sum(s, wsum);
    if (threadIdx.x == 0) tilecount[(int64_t)b * T + tile] = all;
}

// grid (T, B): the points of tile x of query y, ascending, behind those of the tiles in front
__global__ __launch_bounds__(LM_THREADS) void lm_fill(const uint32_t* bitmap, int64_t W, int T, const uint32_t* tilecount, const int64_t* out_off,
                                                      int64_t total, int32_t* out) {
    __shared__ unsigned wsum[LM_THREADS / 64];
    __shared__ unsigned wave_sum[LM_THREADS / 64];
    const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    unsigned front = 0;
    for (int k = tid; k < tile; k += LM_THREADS) front += tilecount[(int64_t)b * T + k];
    front = lm_block_sum(front, wsum);
    const uint32_t* bits = bitmap + (int64_t)b * W;
    const int64_t base = (int64_t)tile * LM_SCAN_TILE + (int64_t)tid * LM_SCAN_WORDS;
    uint32_t word[LM_SCAN_WORDS];
    unsigned s = 0;
#pragma unroll
    for (int k = 0; k < LM_SCAN_WORDS; ++k) {
        word[k] = base + k < W ? bits[base + k] : 0u;
        s += __popc(word[k]);
    }
    unsigned inc = s;                                         // inclusive scan of the thread sums inside the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned up = __shfl_up(inc, off, 64);
        if (lane >= off) inc += up;
    }
    if (lane == 63) wave_sum[w] = inc;
    __syncthreads();
    unsigned before = 0;
#pragma unroll
    for (int k = 0; k < LM_THREADS / 64; ++k)
        if (k < w) before += wave_sum[k];
    const int64_t end = out_off[b + 1] < total ? out_off[b + 1] : total;
    int64_t pos = out_off[b] + front + before + inc - s;
    if (out_off[b] < 0) return;
#pragma unroll
    for (int k = 0; k < LM_SCAN_WORDS; ++k) {
        uint32_t v = word[k];
        while (v) {
            const int bit = __ffs(v) - 1;
            if (pos < end) out[pos] = (int32_t)((base + k) * 32 + bit);       // never store outside the query's slice
            ++pos;
            v &= v - 1;
        }
    }
}

// ---- keyframe culling -------------------------------------------------------------------------------------------------------------
// G lanes per row, 256 / G rows per workgroup, `tiles` workgroups per candidate.  The launch owns the rows whose point has a
// list of more than lo and at most hi entries.
template <int G>
__global__ __launch_bounds__(LM_THREADS) void lm_cull(const lm_map t, const int32_t* fp, const int32_t* level, const int32_t* cand,
                                                      const int64_t* crow_off, int64_t crows, unsigned tiles, int th_obs, int lo, int hi,
                                                      lm_u64* counts, uint8_t* flags, unsigned* scal, unsigned* index_errors) {
    __shared__ unsigned gsum[LM_THREADS / 64];
    constexpr int PER = LM_THREADS / G;
    const int tid = threadIdx.x, g = tid / G, lane = tid % G;
    const unsigned ci = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int c = cand ? cand[ci] : (int)ci;                   // checked on the host
    int64_t first = 0, rows = -1;
    if (c >= 0 && c < t.F && !(t.removed && t.removed[c])) rows = lm_rows(t, c, &first);
    const int64_t local = (int64_t)tile * PER + g;
    int m = -1, n = 0, l = 0;
    int64_t s0 = 0;
    if (local < rows) {
        m = fp[first + local];
        if (m >= t.M) {
            if (lane == 0) lm_index_error(scal, index_errors);
            m = -1;
        }
        if (m >= 0 && t.bad && t.bad[m]) m = -1;
        if (m >= 0) {
            n = lm_list(t, m, &s0);
            if (n < 0) {
                if (lane == 0) lm_index_error(scal, index_errors);
                m = -1;
            }
        }
    }
    const bool mine = m >= 0 && n > lo && n <= hi;
    if (mine) l = level[first + local];
    unsigned v = 0;                                            // observers | qualifying observers << 16, each at most 256
    for (int k = lane; k < (mine ? n : 0); k += G) {
        const int2 o = t.obs[s0 + k];
        if (o.x < 0 || o.x >= t.F) {
            lm_index_error(scal, index_errors);
            continue;
        }
        if (t.removed && t.removed[o.x]) continue;             // a removed keyframe observes nothing
        v += 1u;
        if (o.x == c) continue;                                // the candidate's own observation does not count
        int64_t f1;
        const int64_t r1 = lm_rows(t, o.x, &f1);
        if (o.y < 0 || o.y >= r1) {
            lm_index_error(scal, index_errors);
            continue;
        }
        if (level[f1 + o.y] <= l + 1) v += 1u << 16;
    }
    if (G <= 64) {
#pragma unroll
        for (int off = G / 2; off; off >>= 1) v += __shfl_xor(v, off, 64);
    } else {
#pragma unroll
        for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((tid & 63) == 0) gsum[tid >> 6] = v;
        __syncthreads();
        v = gsum[0] + gsum[1] + gsum[2] + gsum[3];
    }
    const int N = (int)(v & 0xffffu), q = (int)(v >> 16);
    const bool head = mine && lane == 0;
    const bool redundant = head && N > th_obs && q >= th_obs;
    if (head && flags) {
        const int64_t at = crow_off[ci] + local;
        if (at >= 0 && at < crows) flags[at] = redundant ? 2 : 1;            // holds by construction; never store outside
    }
    lm_u64 sum = (head ? 1ull : 0ull) | (redundant ? 1ull << 32 : 0ull);      // n_points low, n_redundant high
#pragma unroll
    for (int off = 32; off; off >>= 1) sum += __shfl_xor(sum, off, 64);
    if ((tid & 63) == 0 && sum) atomicAdd(&counts[ci], sum);                  // one counting atomic a wave
}

// ---- the host side ----------------------------------------------------------------------------------------------------------------
extern "C" int slam_lmap_limits(int32_t* h_limits) {
    SLAM_REQUIRE(h_limits, "slam_lmap_limits: null limits");
    h_limits[0] = LM_THREADS;
    h_limits[1] = LM_VOTE_LDS_SMALL;
    h_limits[2] = LM_VOTE_LDS_FRAMES;                          // above: the global-memory form
    h_limits[3] = 16;                                         // lanes per row of the culling kernel: lists of at most 16,
    h_limits[4] = 64;                                         // of at most 64,
    h_limits[5] = LM_OBS_MAX;                                 // and of at most 256 entries
    h_limits[6] = LM_SCAN_TILE;                               // bitmap words of one scan tile
    h_limits[7] = LM_SCAL_BYTES;
    return SLAM_OK;
}

static int lm_sizes(const char* who, int64_t B, int64_t F, int64_t M, int64_t C) {
    SLAM_REQUIRE(B >= 0 && B <= LM_QUERIES_MAX && F >= 1 && F <= LM_FRAMES_MAX && M >= 1 && M <= LM_POINTS_MAX && C >= 0 && C <= LM_FRAMES_MAX,
                 "%s: bad sizes (B=%lld, F=%lld, M=%lld, C=%lld)", who, (long long)B, (long long)F, (long long)M, (long long)C);
    return SLAM_OK;
}

struct lm_layout {
    int64_t W;                                                // words of one bitmap row
    int T;                                                    // scan tiles of one bitmap row
    uint64_t qoff, lkf_off, out_off, tilecount;               // vote: qoff; points: all four
    uint64_t cand, crow_off;                                  // cull
    uint64_t inverse_bytes, vote_bytes, points_bytes, cull_bytes;
};

static lm_layout lm_lay(int64_t B, int64_t M, int64_t C) {
    lm_layout y = {};
    y.W = (M + 31) / 32;
    y.T = (int)lm_tiles(y.W, LM_SCAN_TILE);
    const uint64_t off_bytes = slam_align_up((uint64_t)(B + 1) * 8);
    y.inverse_bytes = LM_SCAL_BYTES;
    y.qoff = LM_SCAL_BYTES;
    y.vote_bytes = y.qoff + off_bytes;
    y.lkf_off = y.vote_bytes;
    y.out_off = y.lkf_off + off_bytes;
    y.tilecount = y.out_off + off_bytes;
    y.points_bytes = y.tilecount + slam_align_up((uint64_t)(B > 0 ? B : 1) * (uint64_t)y.T * 4);
    y.cand = LM_SCAL_BYTES;
    y.crow_off = y.cand + slam_align_up((uint64_t)(C > 0 ? C : 1) * 4);
    y.cull_bytes = y.crow_off + slam_align_up((uint64_t)(C + 1) * 8);
    return y;
}

extern "C" int slam_lmap_workspace(int64_t B, int64_t F, int64_t M, int64_t C, uint64_t* h_bytes) {
    SLAM_REQUIRE(h_bytes, "slam_lmap_workspace: null bytes");
    if (int rc = lm_sizes("slam_lmap_workspace", B, F, M, C)) return rc;
    const lm_layout y = lm_lay(B, M, C);
    h_bytes[0] = y.inverse_bytes;
    h_bytes[1] = y.vote_bytes;
    h_bytes[2] = y.points_bytes;
    h_bytes[3] = y.cull_bytes;
    return SLAM_OK;
}

// offsets [n + 1] that ascend from 0 to at most `limit`
static int lm_check_offsets(const char* who, const char* what, const int64_t* off, int64_t n, int64_t limit) {
    SLAM_REQUIRE(off && off[0] == 0, "%s: null %s offsets, or offsets that do not start at 0", who, what);
    for (int64_t i = 0; i < n; ++i) SLAM_REQUIRE(off[i + 1] >= off[i], "%s: the %s offsets descend at %lld", who, what, (long long)i);
    SLAM_REQUIRE(off[n] <= limit, "%s: the %s offsets end at %lld, past %lld", who, what, (long long)off[n], (long long)limit);
    return SLAM_OK;
}

// the tables of a call; which of them a call reads, and so which pointers it needs, is the entry point's to check
static int lm_map_arg(const char* who, lm_map* t, int64_t M, int64_t nnz, const int64_t* d_offsets, const int32_t* d_obs, const uint8_t* d_bad,
                      int64_t F, const int64_t* d_frame_offsets, int64_t n_rows, const uint8_t* d_removed) {
    SLAM_REQUIRE(nnz >= 0 && nnz <= LM_ROWS_MAX && n_rows >= 0 && n_rows <= LM_ROWS_MAX, "%s: bad sizes (nnz=%lld, rows=%lld)", who, (long long)nnz,
                 (long long)n_rows);
    SLAM_REQUIRE(((uintptr_t)d_obs & 7) == 0 && ((uintptr_t)d_offsets & 7) == 0 && ((uintptr_t)d_frame_offsets & 7) == 0, "%s: misaligned pointer", who);
    t->offsets = d_offsets;
    t->obs = (const int2*)d_obs;
    t->bad = d_bad;
    t->fo = d_frame_offsets;
    t->removed = d_removed;
    t->M = M;
    t->nnz = nnz;
    t->n_rows = n_rows;
    t->F = (int)F;
    return SLAM_OK;
}

extern "C" int slam_lmap_frame_points(slam_ctx* ctx, int64_t M, int64_t nnz, const int64_t* d_offsets, const int32_t* d_obs, int64_t F,
                                      const int64_t* d_frame_offsets, int64_t n_rows, int32_t* d_frame_points, void* d_ws, int64_t* h_scalars) {
    const char* who = "slam_lmap_frame_points";
    SLAM_REQUIRE(ctx && h_scalars, "%s: null argument", who);
    if (int rc = lm_sizes(who, 0, F, M, 0)) return rc;
    lm_map t;
    if (int rc = lm_map_arg(who, &t, M, nnz, d_offsets, d_obs, nullptr, F, d_frame_offsets, n_rows, nullptr)) return rc;
    SLAM_REQUIRE(d_ws && d_offsets && d_frame_offsets && (nnz == 0 || d_obs) && (n_rows == 0 || d_frame_points), "%s: null device pointer", who);
    SLAM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    SLAM_HIP(hipMemsetAsync(d_ws, 0, LM_SCAL_BYTES, st));
    if (n_rows) SLAM_HIP(hipMemsetAsync(d_frame_points, 0xFF, (size_t)n_rows * 4, st));
    if (nnz) lm_inverse<<<lm_grid(nnz), LM_THREADS, 0, st>>>(t, d_frame_points, (unsigned*)d_ws, slam_index_error_counter(ctx));
    if (int rc = slam_launch_check(who)) return rc;
    uint32_t h[2];
    SLAM_HIP(hipMemcpyAsync(h, d_ws, sizeof(h), hipMemcpyDeviceToHost, st));
    SLAM_HIP(hipStreamSynchronize(st));
    h_scalars[0] = h[0];
    h_scalars[1] = h[1];
    return SLAM_OK;
}

extern "C" int slam_lmap_vote(slam_ctx* ctx, int64_t B, const int32_t* d_qpoints, const int64_t* h_qoffsets, int64_t M, int64_t nnz,
                              const int64_t* d_offsets, const int32_t* d_obs, const uint8_t* d_point_bad, int64_t F, const uint8_t* d_frame_removed,
                              int form, void* d_ws, int32_t* d_votes, int32_t* d_best, int32_t* d_nvoted, int64_t* h_skipped) {
    const char* who = "slam_lmap_vote";
    SLAM_REQUIRE(ctx, "%s: null ctx", who);
    if (int rc = lm_sizes(who, B, F, M, 0)) return rc;
    SLAM_REQUIRE(form >= 0 && form <= 3, "%s: form %d is not 0 (by F), 1, 2 (LDS) or 3 (global memory)", who, form);
    SLAM_REQUIRE(form == 0 || form == 3 || F <= (form == 1 ? LM_VOTE_LDS_SMALL : LM_VOTE_LDS_FRAMES), "%s: F=%lld frames do not fit form %d", who,
                 (long long)F, form);
    SLAM_REQUIRE(B * F <= LM_ROWS_MAX, "%s: B x F = %lld votes, more than 2^31 - 1", who, (long long)(B * F));
    if (h_skipped) *h_skipped = 0;
    if (B == 0) return SLAM_OK;
    if (int rc = lm_check_offsets(who, "query", h_qoffsets, B, LM_ROWS_MAX)) return rc;
    const int64_t Q = h_qoffsets[B];
    lm_map t;                                                  // (the vote reads no frame row)
    if (int rc = lm_map_arg(who, &t, M, nnz, d_offsets, d_obs, d_point_bad, F, nullptr, 0, d_frame_removed)) return rc;
    SLAM_REQUIRE(d_ws && d_votes && d_best && d_nvoted && d_offsets && (nnz == 0 || d_obs) && (Q == 0 || d_qpoints), "%s: null device pointer", who);
    SLAM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const lm_layout y = lm_lay(B, M, 0);
    unsigned* scal = (unsigned*)d_ws;
    int64_t* qoff = LM_AT(int64_t, d_ws, y.qoff);
    SLAM_HIP(hipMemsetAsync(d_ws, 0, LM_SCAL_BYTES, st));
    SLAM_HIP(hipMemcpyAsync(qoff, h_qoffsets, (size_t)(B + 1) * 8, hipMemcpyHostToDevice, st));      // (pageable: it has left the host array on return)
    if (form == 0) form = F <= LM_VOTE_LDS_SMALL ? 1 : (F <= LM_VOTE_LDS_FRAMES ? 2 : 3);
    unsigned* ie = slam_index_error_counter(ctx);
    if (form == 1) {
        lm_vote<LM_VOTE_LDS_SMALL><<<(unsigned)B, LM_THREADS, 0, st>>>(t, d_qpoints, qoff, Q, d_votes, d_best, d_nvoted, scal, ie);
    } else if (form == 2) {
        lm_vote<LM_VOTE_LDS_FRAMES><<<(unsigned)B, LM_THREADS, 0, st>>>(t, d_qpoints, qoff, Q, d_votes, d_best, d_nvoted, scal, ie);
    } else {
        SLAM_HIP(hipMemsetAsync(d_votes, 0, (size_t)(B * F) * 4, st));
        lm_vote<0><<<(unsigned)B, LM_THREADS, 0, st>>>(t, d_qpoints, qoff, Q, d_votes, d_best, d_nvoted, scal, ie);
        lm_vote_best<<<(unsigned)B, LM_THREADS, 0, st>>>(d_votes, (int)F, d_best, d_nvoted);
    }
    if (int rc = slam_launch_check(who)) return rc;
    if (h_skipped) {
        uint32_t h = 0;
        SLAM_HIP(hipMemcpyAsync(&h, d_ws, sizeof(h), hipMemcpyDeviceToHost, st));
        SLAM_HIP(hipStreamSynchronize(st));
        *h_skipped = h;
    }
    return SLAM_OK;
}

extern "C" int slam_lmap_points_mark(slam_ctx* ctx, int64_t B, const int32_t* d_lkf, const int64_t* h_lkf_offsets, const int32_t* d_qpoints,
                                     const int64_t* h_qoffsets, int64_t M, const uint8_t* d_point_bad, int64_t F, const int64_t* d_frame_offsets,
                                     int64_t n_rows, const int32_t* d_frame_points, const uint8_t* d_frame_removed, uint32_t* d_bitmap, void* d_ws,
                                     int64_t* h_counts) {
    const char* who = "slam_lmap_points_mark";
    SLAM_REQUIRE(ctx, "%s: null ctx", who);
    if (int rc = lm_sizes(who, B, F, M, 0)) return rc;
    if (B == 0) return SLAM_OK;
    SLAM_REQUIRE(h_counts, "%s: null counts", who);
    if (int rc = lm_check_offsets(who, "local keyframe", h_lkf_offsets, B, LM_ROWS_MAX)) return rc;
    if (int rc = lm_check_offsets(who, "query", h_qoffsets, B, LM_ROWS_MAX)) return rc;
    const int64_t E = h_lkf_offsets[B], Q = h_qoffsets[B];
    lm_map t;                                                  // (no observation list is read)
    if (int rc = lm_map_arg(who, &t, M, 0, nullptr, nullptr, d_point_bad, F, d_frame_offsets, n_rows, d_frame_removed)) return rc;
    SLAM_REQUIRE(d_ws && d_bitmap && d_frame_offsets && (E == 0 || d_lkf) && (Q == 0 || d_qpoints) && (n_rows == 0 || d_frame_points), "%s: null device pointer", who);
    const lm_layout y = lm_lay(B, M, 0);
    SLAM_REQUIRE((int64_t)B * y.W <= LM_ROWS_MAX, "%s: a bitmap of %lld words", who, (long long)(B * y.W));
    SLAM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    unsigned *scal = (unsigned*)d_ws, *ie = slam_index_error_counter(ctx);
    int64_t *qoff = LM_AT(int64_t, d_ws, y.qoff), *lkf_off = LM_AT(int64_t, d_ws, y.lkf_off);
    uint32_t* tilecount = LM_AT(uint32_t, d_ws, y.tilecount);
    SLAM_HIP(hipMemsetAsync(d_ws, 0, LM_SCAL_BYTES, st));
    SLAM_HIP(hipMemsetAsync(d_bitmap, 0, (size_t)(B * y.W) * 4, st));
    SLAM_HIP(hipMemcpyAsync(qoff, h_qoffsets, (size_t)(B + 1) * 8, hipMemcpyHostToDevice, st));
    SLAM_HIP(hipMemcpyAsync(lkf_off, h_lkf_offsets, (size_t)(B + 1) * 8, hipMemcpyHostToDevice, st));
    if (E) lm_mark<<<(unsigned)E, LM_THREADS, 0, st>>>(t, d_frame_points, d_lkf, lkf_off, (int)B, y.W, d_bitmap, scal, ie);
    if (Q) lm_clear<<<lm_grid(Q), LM_THREADS, 0, st>>>(d_qpoints, qoff, Q, (int)B, M, y.W, d_bitmap, scal, ie);
    lm_popcount<<<dim3((unsigned)y.T, (unsigned)B), LM_THREADS, 0, st>>>(d_bitmap, y.W, y.T, tilecount);
    if (int rc = slam_launch_check(who)) return rc;
    std::vector<uint32_t> h((size_t)B * y.T);
    SLAM_HIP(hipMemcpyAsync(h.data(), tilecount, h.size() * 4, hipMemcpyDeviceToHost, st));
    SLAM_HIP(hipStreamSynchronize(st));
    for (int64_t b = 0; b < B; ++b) {
        int64_t s = 0;
        for (int k = 0; k < y.T; ++k) s += h[(size_t)(b * y.T + k)];
        h_counts[b] = s;
    }
    return SLAM_OK;
}

extern "C" int slam_lmap_points_fill(slam_ctx* ctx, int64_t B, int64_t M, const uint32_t* d_bitmap, void* d_ws, const int64_t* h_out_offsets,
                                     int32_t* d_lpoints) {
    const char* who = "slam_lmap_points_fill";
    SLAM_REQUIRE(ctx, "%s: null ctx", who);
    if (int rc = lm_sizes(who, B, 1, M, 0)) return rc;
    if (B == 0) return SLAM_OK;
    if (int rc = lm_check_offsets(who, "output", h_out_offsets, B, LM_ROWS_MAX)) return rc;
    const int64_t total = h_out_offsets[B];
    SLAM_REQUIRE(d_ws && d_bitmap && (total == 0 || d_lpoints), "%s: null device pointer", who);
    if (total == 0) return SLAM_OK;
    const lm_layout y = lm_lay(B, M, 0);
    SLAM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int64_t* out_off = LM_AT(int64_t, d_ws, y.out_off);
    SLAM_HIP(hipMemcpyAsync(out_off, h_out_offsets, (size_t)(B + 1) * 8, hipMemcpyHostToDevice, st));
    lm_fill<<<dim3((unsigned)y.T, (unsigned)B), LM_THREADS, 0, st>>>(d_bitmap, y.W, y.T, LM_AT(const uint32_t, d_ws, y.tilecount), out_off, total,
                                                                    d_lpoints);
    return slam_launch_check(who);
}

extern "C" int slam_lmap_cull_count(slam_ctx* ctx, int64_t C, const int32_t* h_cand, int64_t M, int64_t nnz, const int64_t* d_offsets,
                                    const int32_t* d_obs, const uint8_t* d_point_bad, int64_t F, const int64_t* h_frame_offsets,
                                    const int64_t* d_frame_offsets, const int32_t* d_frame_points, const int32_t* d_level,
                                    const uint8_t* d_frame_removed, int th_obs, int max_list, void* d_ws, int32_t* d_counts, uint8_t* d_flags) {
    const char* who = "slam_lmap_cull_count";
    SLAM_REQUIRE(ctx, "%s: null ctx", who);
    if (!h_cand) C = F;
    if (int rc = lm_sizes(who, 0, F, M, C)) return rc;
    SLAM_REQUIRE(th_obs >= 0 && th_obs <= LM_OBS_MAX, "%s: th_obs=%d outside [0, %d]", who, th_obs, LM_OBS_MAX);
    SLAM_REQUIRE(max_list >= 0 && max_list <= LM_OBS_MAX, "%s: max_list=%d outside [0, %d]", who, max_list, LM_OBS_MAX);
    if (int rc = lm_check_offsets(who, "frame", h_frame_offsets, F, LM_ROWS_MAX)) return rc;
    if (C == 0) return SLAM_OK;
    const int64_t n_rows = h_frame_offsets[F];
    std::vector<int64_t> crow((size_t)C + 1);
    int64_t max_rows = 0;
    crow[0] = 0;
    for (int64_t i = 0; i < C; ++i) {
        const int64_t c = h_cand ? h_cand[i] : i;
        SLAM_REQUIRE(c >= 0 && c < F, "%s: candidate[%lld] = %lld names no frame", who, (long long)i, (long long)c);
        const int64_t rows = h_frame_offsets[c + 1] - h_frame_offsets[c];
        crow[(size_t)i + 1] = crow[(size_t)i] + rows;
        max_rows = rows > max_rows ? rows : max_rows;
    }
    SLAM_REQUIRE(crow[(size_t)C] <= LM_ROWS_MAX, "%s: more than 2^31 - 1 candidate rows", who);
    lm_map t;
    if (int rc = lm_map_arg(who, &t, M, nnz, d_offsets, d_obs, d_point_bad, F, d_frame_offsets, n_rows, d_frame_removed)) return rc;
    SLAM_REQUIRE(d_ws && d_counts && d_offsets && d_frame_offsets && (nnz == 0 || d_obs) && (n_rows == 0 || (d_frame_points && d_level)),
                 "%s: null device pointer", who);
    SLAM_REQUIRE(((uintptr_t)d_counts & 7) == 0, "%s: misaligned counts", who);
    SLAM_REQUIRE(max_rows * C <= LM_CULL_GROUPS_MAX, "%s: %lld candidates of up to %lld rows: more than the 2^24 workgroups one launch takes", who,
                 (long long)C, (long long)max_rows);
    SLAM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const lm_layout y = lm_lay(0, M, C);
    unsigned *scal = (unsigned*)d_ws, *ie = slam_index_error_counter(ctx);
    int32_t* cand = h_cand ? LM_AT(int32_t, d_ws, y.cand) : nullptr;
    int64_t* crow_off = LM_AT(int64_t, d_ws, y.crow_off);
    SLAM_HIP(hipMemsetAsync(d_ws, 0, LM_SCAL_BYTES, st));
    SLAM_HIP(hipMemsetAsync(d_counts, 0, (size_t)C * 8, st));
    if (d_flags && crow[(size_t)C]) SLAM_HIP(hipMemsetAsync(d_flags, 0, (size_t)crow[(size_t)C], st));
    if (h_cand) SLAM_HIP(hipMemcpyAsync(cand, h_cand, (size_t)C * 4, hipMemcpyHostToDevice, st));
    SLAM_HIP(hipMemcpyAsync(crow_off, crow.data(), (size_t)(C + 1) * 8, hipMemcpyHostToDevice, st));
    // (the copies read pageable memory: they have left the host arrays when they return)
    if (max_rows) {
        // a class per group size; the last class launched takes every longer list too (its lanes stride), so a max_list below
        // the longest list of the table costs time, never a verdict
        const int top = max_list <= 16 ? 0 : (max_list <= 64 ? 1 : 2);
        lm_u64* counts = (lm_u64*)d_counts;
        const unsigned t16 = (unsigned)lm_tiles(max_rows, LM_THREADS / 16), t64 = (unsigned)lm_tiles(max_rows, LM_THREADS / 64), t256 = (unsigned)max_rows;
        lm_cull<16><<<(unsigned)(C * t16), LM_THREADS, 0, st>>>(t, d_frame_points, d_level, cand, crow_off, crow[(size_t)C], t16, th_obs, -1, top == 0 ? INT_MAX : 16, counts,
                                                               d_flags, scal, ie);
        if (top >= 1)
            lm_cull<64><<<(unsigned)(C * t64), LM_THREADS, 0, st>>>(t, d_frame_points, d_level, cand, crow_off, crow[(size_t)C], t64, th_obs, 16, top == 1 ? INT_MAX : 64,
                                                                   counts, d_flags, scal, ie);
        if (top >= 2)
            lm_cull<256><<<(unsigned)(C * t256), LM_THREADS, 0, st>>>(t, d_frame_points, d_level, cand, crow_off, crow[(size_t)C], t256, th_obs, 64, INT_MAX, counts, d_flags,
                                                                     scal, ie);
    }
    return slam_launch_check(who);
}
