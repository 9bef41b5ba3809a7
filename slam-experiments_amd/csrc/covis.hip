// covis.hip — the covisibility graph on the device (slam_covis_*).
//
// slamhip.covisibility, bit for bit: edges (k1 < k2, ascending), weights, pair_ptr and the pair lists pair_a / pair_b
// (ascending in the point inside an edge), from the observation tables a sparse bundle adjustment already keeps on the device.
//
//   count   1. key(o) = point << (pb + 1) | fixed << pb | pose, payload o; a stable LSD radix sort of the O keys.  The free
//              observations of a point are then one run, ascending in pose; two equal neighbours are a (pose, point) pair
//              observed twice (counted, on fixed poses too).
//           2. n_l free observers of point l give n_l (n_l - 1) / 2 pairs; an exclusive scan in 64 bits gives each point its
//              first pair slot and P.  The host compares P and the duplicate count with its limits before anything else runs.
//   pairs   3. thread t < P finds its point by bisection of the scan and its (i, j) inside the point by bisection of the row
//              starts of the strict upper triangle, and writes (key = k1 K + k2, a, b) to slot t: point order, all integers.
//           4. a stable LSD radix sort by key over the bits K^2 - 1 has; pairs arrive ascending in the point, so they leave
//              ordered by (k1, k2, l).  Keys are 32 bits up to K = 65 536 and 64 bits above.
//           5. run heads of the sorted keys, an exclusive scan of the head flags: E and the rank of every head.
//   edges   6. head i of rank r writes edges[r], pair_ptr[r]; weights[r] = pair_ptr[r + 1] - pair_ptr[r].
//
// The sort (cv_hist / scan / cv_scatter) is this file's own: 8-bit digits, a tile of CV_TILE keys per workgroup, the digit
// counts of every tile scanned digit-major, ranks inside a tile from wave ballots (64 lanes) in item order.  Integer atomics
// only count (LDS histograms, the scalars); no output depends on the order they arrive in.  No floating point.
#include "internal.h"

#define CV_THREADS 256
#define CV_ITEMS 16                          // keys a thread of a sort tile takes
#define CV_TILE (CV_THREADS * CV_ITEMS)      // keys of one sort tile
#define CV_DIGIT_BITS 8
#define CV_DIGITS 256
#define CV_SCAN_ITEMS 8
#define CV_SCAN_TILE (CV_THREADS * CV_SCAN_ITEMS)
#define CV_SCAL_BYTES 256                    // the scalar block at the head of a workspace: uint64 [8], the rest padding

typedef unsigned long long cv_u64;

// ---- exclusive scan, any length ------------------------------------------------------------------------------------------------
// One workgroup scans CV_SCAN_TILE entries in place and leaves its total in sums[block]; the totals are scanned the same way
// and added back.  A single workgroup also writes the total of all to *total.
template <typename T>
__global__ __launch_bounds__(CV_THREADS) void cv_scan_tile(T* d, int64_t n, T* sums, T* total) {
    __shared__ T wave_sum[CV_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t base = (int64_t)blockIdx.x * CV_SCAN_TILE + (int64_t)tid * CV_SCAN_ITEMS;
    T v[CV_SCAN_ITEMS], s = 0;
#pragma unroll
    for (int k = 0; k < CV_SCAN_ITEMS; ++k) {
        v[k] = base + k < n ? d[base + k] : (T)0;
        s += v[k];
    }
    T inc = s;                                               // inclusive scan of the thread sums inside the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T up = __shfl_up(inc, off, 64);
        if (lane >= off) inc += up;
    }
    if (lane == 63) wave_sum[w] = inc;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < CV_THREADS / 64; ++k) {
        if (k < w) before += wave_sum[k];
        all += wave_sum[k];
    }
    T run = before + inc - s;
#pragma unroll
    for (int k = 0; k < CV_SCAN_ITEMS; ++k) {
        if (base + k < n) d[base + k] = run;
        run += v[k];
    }
    if (tid == 0) {
        sums[blockIdx.x] = all;
        if (total && gridDim.x == 1) *total = all;
    }
}

template <typename T>
__global__ __launch_bounds__(CV_THREADS) void cv_scan_add(T* d, int64_t n, const T* sums) {
    const T add = sums[blockIdx.x];
    const int64_t base = (int64_t)blockIdx.x * CV_SCAN_TILE + (int64_t)threadIdx.x * CV_SCAN_ITEMS;
#pragma unroll
    for (int k = 0; k < CV_SCAN_ITEMS; ++k)
        if (base + k < n) d[base + k] += add;
}

static inline int64_t cv_tiles(int64_t n, int64_t tile) { return (n + tile - 1) / tile; }

// entries of scratch a scan of n entries takes: the totals of every level, each level on a 32-entry boundary
static uint64_t cv_scan_scratch(int64_t n) {
    uint64_t s = 0;
    for (int64_t m = cv_tiles(n > 0 ? n : 1, CV_SCAN_TILE);; m = cv_tiles(m, CV_SCAN_TILE)) {
        s += slam_align_up((uint64_t)m, 32);
        if (m == 1) break;
    }
    return s;
}

template <typename T>
static void cv_scan(hipStream_t st, T* d, int64_t n, T* scratch, T* total) {
    const int64_t nb = cv_tiles(n, CV_SCAN_TILE);
    cv_scan_tile<T><<<(unsigned)nb, CV_THREADS, 0, st>>>(d, n, scratch, total);
    if (nb == 1) return;
    cv_scan(st, scratch, nb, scratch + slam_align_up((uint64_t)nb, 32), total);
    cv_scan_add<T><<<(unsigned)nb, CV_THREADS, 0, st>>>(d, n, scratch);
}

// ---- stable LSD radix sort ---------------------------------------------------------------------------------------------------------
// hist[digit * tiles + tile]: digit-major, so ONE exclusive scan gives every (digit, tile) its first output slot.
template <typename KT>
__global__ __launch_bounds__(CV_THREADS) void cv_hist(const KT* keys, int64_t n, int shift, uint32_t* hist, int64_t tiles) {
    __shared__ uint32_t h[CV_DIGITS];
    const int tid = threadIdx.x;
    h[tid] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * CV_TILE;
    for (int c = 0; c < CV_ITEMS; ++c) {
        const int64_t i = base + c * CV_THREADS + tid;
        if (i < n) atomicAdd(&h[(unsigned)(keys[i] >> shift) & (CV_DIGITS - 1)], 1u);    // a count: the order of arrival does not show
    }
    __syncthreads();
    hist[(int64_t)tid * tiles + blockIdx.x] = h[tid];
}

// Ranks inside a tile in item order: the tile is taken 256 keys at a time, thread t the t-th; inside a wave the lanes with the
// same digit are found by eight ballots, the waves of a round and the rounds follow each other through LDS counters.
template <typename KT, bool TWO>
__global__ __launch_bounds__(CV_THREADS) void cv_scatter(const KT* kin, const int32_t* ain, const int32_t* bin, KT* kout, int32_t* aout,
                                                         int32_t* bout, int64_t n, int shift, const uint32_t* hist, int64_t tiles) {
    __shared__ uint32_t run[CV_DIGITS];
    __shared__ uint32_t wc[CV_THREADS / 64][CV_DIGITS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    run[tid] = hist[(int64_t)tid * tiles + blockIdx.x];
#pragma unroll
    for (int k = 0; k < CV_THREADS / 64; ++k) wc[k][tid] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * CV_TILE;
    for (int c = 0; c < CV_ITEMS; ++c) {
        if (base + (int64_t)c * CV_THREADS >= n) break;                               // the same for every thread
        const int64_t i = base + c * CV_THREADS + tid;
        const bool valid = i < n;
        const KT key = valid ? kin[i] : (KT)0;
        const unsigned d = (unsigned)(key >> shift) & (CV_DIGITS - 1);
        cv_u64 same = __ballot(valid);
#pragma unroll
        for (int b = 0; b < CV_DIGIT_BITS; ++b) {
            const bool bit = (d >> b) & 1;
            const cv_u64 bal = __ballot(bit);
            same &= bit ? bal : ~bal;
        }
        const unsigned rank = __popcll(same & ((1ull << lane) - 1));
        if (valid && rank == 0) wc[w][d] = __popcll(same);
        __syncthreads();
        if (valid) {
            uint32_t pos = run[d] + rank;
            for (int k = 0; k < w; ++k) pos += wc[k][d];
            if ((int64_t)pos < n) {                                                    // holds by construction; never store outside
                kout[pos] = key;
                aout[pos] = ain[i];
                if (TWO) bout[pos] = bin[i];
            }
        }
        __syncthreads();
        uint32_t add = 0;
#pragma unroll
        for (int k = 0; k < CV_THREADS / 64; ++k) {
            add += wc[k][tid];
            wc[k][tid] = 0;
        }
        run[tid] += add;
        __syncthreads();
    }
}

static inline int cv_bitlen(uint64_t v) {
    int b = 0;
    while (v) { ++b; v >>= 1; }
    return b;
}
static inline int cv_passes(int bits) { return (bits + CV_DIGIT_BITS - 1) / CV_DIGIT_BITS; }

// Sorts n keys of `bits` bits with their payloads.  The data starts in k[0], a[0], b[0] and ends in k[passes & 1], ...
template <typename KT, bool TWO>
static void cv_sort(hipStream_t st, KT* const k[2], int32_t* const a[2], int32_t* const b[2], int64_t n, int bits, uint32_t* hist,
                    uint32_t* scan_scratch) {
    const int64_t tiles = cv_tiles(n, CV_TILE);
    for (int p = 0; p < cv_passes(bits); ++p) {
        const int s = p & 1, shift = p * CV_DIGIT_BITS;
        cv_hist<KT><<<(unsigned)tiles, CV_THREADS, 0, st>>>(k[s], n, shift, hist, tiles);
        cv_scan<uint32_t>(st, hist, tiles * CV_DIGITS, scan_scratch, nullptr);
        cv_scatter<KT, TWO><<<(unsigned)tiles, CV_THREADS, 0, st>>>(k[s], a[s], TWO ? b[s] : nullptr, k[s ^ 1], a[s ^ 1], TWO ? b[s ^ 1] : nullptr, n,
                                                                    shift, hist, tiles);
    }
}

// ---- the count phase -----------------------------------------------------------------------------------------------------------------
// scalars (uint64 [8] at the head of the count workspace): 0 free observations, 1 duplicates, 2 P, 3 index errors
template <typename KT>
__global__ __launch_bounds__(CV_THREADS) void cv_obs_keys(const int32_t* obs_pose, const int32_t* obs_point, const uint8_t* fixed, int64_t O, int K,
                                                          int L, int pb, KT* keys, int32_t* idx, cv_u64* scal, unsigned int* index_errors) {
    const int64_t o = (int64_t)blockIdx.x * CV_THREADS + threadIdx.x;
    if (o >= O) return;
    const int p = obs_pose[o], l = obs_point[o];
    KT key;
    if (p < 0 || p >= K || l < 0 || l >= L) {                 // counted, never dereferenced: sorted behind every point
        key = (KT)L << (pb + 1);
        atomicAdd(&scal[3], 1ull);
        atomicAdd(index_errors, 1u);
    } else {
        key = (KT)l << (pb + 1) | (KT)(fixed && fixed[p] ? 1 : 0) << pb | (KT)p;
    }
    keys[o] = key;
    idx[o] = (int32_t)o;
}

// the first slot of every point that has observations, the end of its free observations, and the duplicates
template <typename KT>
__global__ __launch_bounds__(CV_THREADS) void cv_point_runs(const KT* keys, int64_t O, int L, int pb, int32_t* pt_start, int32_t* pt_end,
                                                            cv_u64* scal) {
    const int64_t i = (int64_t)blockIdx.x * CV_THREADS + threadIdx.x;
    if (i >= O) return;
    const KT key = keys[i];
    const int64_t l = (int64_t)(key >> (pb + 1));
    if (l >= L) return;
    if (i == 0 || (int64_t)(keys[i - 1] >> (pb + 1)) != l) pt_start[l] = (int32_t)i;
    if (i > 0 && keys[i - 1] == key) atomicAdd(&scal[1], 1ull);
    if (!((key >> pb) & 1) && (i + 1 == O || (keys[i + 1] >> pb) != (key >> pb))) pt_end[l] = (int32_t)(i + 1);
}

__global__ __launch_bounds__(CV_THREADS) void cv_point_pairs(const int32_t* pt_start, const int32_t* pt_end, int L, cv_u64* pairs, cv_u64* scal) {
    const int64_t l = (int64_t)blockIdx.x * CV_THREADS + threadIdx.x;
    cv_u64 n = 0;
    if (l < L) {
        const int s = pt_start[l], e = pt_end[l];             // a point seen by fixed poses only has no end: e = 0 <= s
        n = e > s ? (cv_u64)(e - s) : 0;
    }
    if (l <= L) pairs[l] = n * (n ? n - 1 : 0) / 2;
    cv_u64 sum = n;                                           // one atomic a wave
#pragma unroll
    for (int off = 32; off; off >>= 1) sum += __shfl_xor(sum, off, 64);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(&scal[0], sum);
}

// ---- the pair phase ------------------------------------------------------------------------------------------------------------------
// the first slot of row i of the strict upper triangle of an n x n table, rows in order: i (2n - i - 1) / 2
__device__ __forceinline__ cv_u64 cv_row_start(cv_u64 i, cv_u64 n) { return i * (2 * n - i - 1) / 2; }

template <typename OK, typename PK>
__global__ __launch_bounds__(CV_THREADS) void cv_emit(const cv_u64* pairs, int L, const int32_t* pt_start, const int32_t* pt_end, const OK* okeys,
                                                      const int32_t* oidx, int64_t O, int pb, int K, int64_t P, PK* keys, int32_t* pa, int32_t* pb_out) {
    const int64_t t = (int64_t)blockIdx.x * CV_THREADS + threadIdx.x;
    if (t >= P) return;
    int lo = 0, hi = L;                                       // the last l with pairs[l] <= t: pairs[0] = 0 <= t < P = pairs[L]
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (pairs[mid] <= (cv_u64)t) lo = mid; else hi = mid;
    }
    const int l = lo;
    const cv_u64 r = (cv_u64)t - pairs[l];
    const int64_t s = pt_start[l];
    if (s < 0 || pt_end[l] - s < 2 || pt_end[l] > O) return;  // holds by construction; never load outside
    const cv_u64 n = (cv_u64)(pt_end[l] - s);
    cv_u64 ilo = 0, ihi = n - 1;                              // the last row i with row_start(i) <= r, i in [0, n - 2]
    while (ihi - ilo > 1) {
        const cv_u64 mid = ilo + (ihi - ilo) / 2;
        if (cv_row_start(mid, n) <= r) ilo = mid; else ihi = mid;
    }
    const int64_t i = s + (int64_t)ilo, j = i + 1 + (int64_t)(r - cv_row_start(ilo, n));
    if (j >= s + (int64_t)n) return;
    const PK mask = ((PK)1 << pb) - 1;
    keys[t] = ((PK)okeys[i] & mask) * (PK)K + ((PK)okeys[j] & mask);
    pa[t] = oidx[i];
    pb_out[t] = oidx[j];
}

template <typename PK>
__global__ __launch_bounds__(CV_THREADS) void cv_heads(const PK* keys, int64_t P, uint32_t* flag) {
    const int64_t i = (int64_t)blockIdx.x * CV_THREADS + threadIdx.x;
    if (i < P) flag[i] = i == 0 || keys[i] != keys[i - 1];
}

template <typename PK>
__global__ __launch_bounds__(CV_THREADS) void cv_edges(const PK* keys, const uint32_t* rank, int64_t P, int64_t E, int K, int32_t* edges,
                                                       int32_t* pair_ptr) {
    const int64_t i = (int64_t)blockIdx.x * CV_THREADS + threadIdx.x;
    if (i == 0) pair_ptr[E] = (int32_t)P;
    if (i >= P) return;
    const PK key = keys[i];
    if (i && keys[i - 1] == key) return;
    const int64_t r = rank[i];
    if (r >= E) return;
    edges[2 * r] = (int32_t)(key / (PK)K);
    edges[2 * r + 1] = (int32_t)(key % (PK)K);
    pair_ptr[r] = (int32_t)i;
}

__global__ __launch_bounds__(CV_THREADS) void cv_weights(const int32_t* pair_ptr, int64_t E, int32_t* weights) {
    const int64_t e = (int64_t)blockIdx.x * CV_THREADS + threadIdx.x;
    if (e < E) weights[e] = pair_ptr[e + 1] - pair_ptr[e];
}

// a point's slot -> (pose, point) arrays: the point of slot s is the last m with offsets[m] <= s
__global__ __launch_bounds__(CV_THREADS) void cv_rows(const int64_t* offsets, const int32_t* obs, int64_t M, int64_t nnz, int32_t* obs_pose,
                                                      int32_t* obs_point) {
    const int64_t s = (int64_t)blockIdx.x * CV_THREADS + threadIdx.x;
    if (s >= nnz) return;
    int64_t lo = 0, hi = M;
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (offsets[mid] <= s) lo = mid; else hi = mid;
    }
    obs_pose[s] = obs[2 * s];
    obs_point[s] = (int32_t)lo;
}

// ---- layouts -------------------------------------------------------------------------------------------------------------------------
struct cv_layout {
    int pb, obits, pbits;              // bits of a pose index, of an observation key, of a pair key
    bool o64, p64;                     // 64-bit observation keys, 64-bit pair keys
    uint64_t ok[2], oi[2], ohist, oscan, pt_start, pt_end, pairs, pscan, count_bytes;     // the count workspace (byte offsets)
    uint64_t pk[2], ta, tb, phist, pscan2, pair_bytes;                                      // the pair workspace
};

static cv_layout cv_lay(int64_t K, int64_t L, int64_t O, int64_t P) {
    cv_layout y = {};
    y.pb = cv_bitlen((uint64_t)K - 1);
    y.obits = y.pb + 1 + cv_bitlen((uint64_t)L);             // the point field holds L too: where entries out of range go
    y.pbits = cv_bitlen((uint64_t)K * (uint64_t)K - 1);
    y.o64 = y.obits > 32;
    y.p64 = y.pbits > 32;
    const uint64_t o = (uint64_t)(O > 0 ? O : 1), p = (uint64_t)(P > 0 ? P : 1), l = (uint64_t)L;
    uint64_t n = CV_SCAL_BYTES;
    auto take = [&](uint64_t b) { const uint64_t at = n; n += slam_align_up(b); return at; };
    y.ok[0] = take(o * (y.o64 ? 8 : 4)); y.ok[1] = take(o * (y.o64 ? 8 : 4));
    y.oi[0] = take(o * 4); y.oi[1] = take(o * 4);
    y.ohist = take((uint64_t)cv_tiles(o, CV_TILE) * CV_DIGITS * 4);
    y.oscan = take(cv_scan_scratch(cv_tiles(o, CV_TILE) * CV_DIGITS) * 4);
    y.pt_start = take(l * 4); y.pt_end = take(l * 4);
    y.pairs = take((l + 1) * 8);
    y.pscan = take(cv_scan_scratch(L + 1) * 8);
    y.count_bytes = n;
    n = CV_SCAL_BYTES;
    y.pk[0] = take(p * (y.p64 ? 8 : 4)); y.pk[1] = take(p * (y.p64 ? 8 : 4));       // the one the sort leaves free holds the head ranks
    y.ta = take(p * 4); y.tb = take(p * 4);
    y.phist = take((uint64_t)cv_tiles(p, CV_TILE) * CV_DIGITS * 4);
    const uint64_t s1 = cv_scan_scratch(cv_tiles(p, CV_TILE) * CV_DIGITS), s2 = cv_scan_scratch(p);
    y.pscan2 = take((s1 > s2 ? s1 : s2) * 4);
    y.pair_bytes = n;
    return y;
}

static int cv_sizes(const char* who, int64_t K, int64_t L, int64_t O, int64_t P) {
    SLAM_REQUIRE(K >= 1 && K <= SLAM_PG_MAX_VERTICES && L >= 1 && L <= SLAM_BAS_MAX_POINTS && O >= 0 && O <= SLAM_BAS_MAX_OBS && P >= 0 &&
                     P <= SLAM_BAS_MAX_PAIRS,
                 "%s: bad sizes (K=%lld, L=%lld, O=%lld, P=%lld)", who, (long long)K, (long long)L, (long long)O, (long long)P);
    return SLAM_OK;
}

#define CV_AT(T, ws, off) ((T*)((char*)(ws) + (off)))

extern "C" int slam_covis_limits(int32_t* h_limits) {
    SLAM_REQUIRE(h_limits, "slam_covis_limits: null limits");
    h_limits[0] = CV_THREADS;
    h_limits[1] = CV_TILE;
    h_limits[2] = CV_DIGIT_BITS;
    h_limits[3] = CV_SCAN_TILE;
    h_limits[4] = 64;                                         // lanes a ballot ranks at once
    h_limits[5] = 65536;                                      // the largest K with 32-bit pair keys
    h_limits[6] = 0;                                          // list lengths at which the kernels change: none (a thread per pair)
    h_limits[7] = CV_SCAL_BYTES;
    return SLAM_OK;
}

extern "C" int slam_covis_plan(int64_t K, int64_t L, int64_t O, int64_t P, int32_t* h_plan) {
    SLAM_REQUIRE(h_plan, "slam_covis_plan: null plan");
    if (int rc = cv_sizes("slam_covis_plan", K, L, O, P)) return rc;
    const cv_layout y = cv_lay(K, L, O, P);
    h_plan[0] = y.obits;
    h_plan[1] = cv_passes(y.obits);
    h_plan[2] = y.o64 ? 8 : 4;
    h_plan[3] = (int32_t)cv_tiles(O, CV_TILE);
    h_plan[4] = y.pbits;
    h_plan[5] = P ? cv_passes(y.pbits) : 0;
    h_plan[6] = y.p64 ? 8 : 4;
    h_plan[7] = (int32_t)cv_tiles(P, CV_TILE);
    return SLAM_OK;
}

extern "C" int slam_covis_workspace(int64_t K, int64_t L, int64_t O, int64_t P, uint64_t* h_bytes) {
    SLAM_REQUIRE(h_bytes, "slam_covis_workspace: null bytes");
    if (int rc = cv_sizes("slam_covis_workspace", K, L, O, P)) return rc;
    const cv_layout y = cv_lay(K, L, O, P);
    h_bytes[0] = y.count_bytes;
    h_bytes[1] = y.pair_bytes;
    return SLAM_OK;
}

static unsigned cv_grid(int64_t n) { return (unsigned)cv_tiles(n > 0 ? n : 1, CV_THREADS); }

template <typename OK>
static void cv_count_run(slam_ctx* ctx, const cv_layout& y, int64_t K, int64_t L, int64_t O, const int32_t* op, const int32_t* ol,
                         const uint8_t* fixed, void* ws) {
    hipStream_t st = ctx->stream;
    cv_u64* scal = (cv_u64*)ws;
    OK* const k[2] = {CV_AT(OK, ws, y.ok[0]), CV_AT(OK, ws, y.ok[1])};
    int32_t* const a[2] = {CV_AT(int32_t, ws, y.oi[0]), CV_AT(int32_t, ws, y.oi[1])};
    int32_t* const none[2] = {nullptr, nullptr};
    int32_t *ps = CV_AT(int32_t, ws, y.pt_start), *pe = CV_AT(int32_t, ws, y.pt_end);
    const int f = cv_passes(y.obits) & 1;
    if (O) {
        cv_obs_keys<OK><<<cv_grid(O), CV_THREADS, 0, st>>>(op, ol, fixed, O, (int)K, (int)L, y.pb, k[0], a[0], scal, slam_index_error_counter(ctx));
        cv_sort<OK, false>(st, k, a, none, O, y.obits, CV_AT(uint32_t, ws, y.ohist), CV_AT(uint32_t, ws, y.oscan));
        cv_point_runs<OK><<<cv_grid(O), CV_THREADS, 0, st>>>(k[f], O, (int)L, y.pb, ps, pe, scal);
    }
    cv_point_pairs<<<cv_grid(L + 1), CV_THREADS, 0, st>>>(ps, pe, (int)L, CV_AT(cv_u64, ws, y.pairs), scal);
    cv_scan<cv_u64>(st, CV_AT(cv_u64, ws, y.pairs), L + 1, CV_AT(cv_u64, ws, y.pscan), scal + 2);
}

extern "C" int slam_covis_count(slam_ctx* ctx, int64_t K, int64_t L, int64_t O, const int32_t* d_obs_pose, const int32_t* d_obs_point,
                                const uint8_t* d_fixed, void* d_count_ws, int64_t* h_scalars) {
    SLAM_REQUIRE(ctx && h_scalars, "slam_covis_count: null argument");
    if (int rc = cv_sizes("slam_covis_count", K, L, O, 0)) return rc;
    SLAM_REQUIRE(d_count_ws && (O == 0 || (d_obs_pose && d_obs_point)), "slam_covis_count: null device pointer");
    SLAM_HIP(hipSetDevice(ctx->device));
    const cv_layout y = cv_lay(K, L, O, 0);
    SLAM_HIP(hipMemsetAsync(d_count_ws, 0, CV_SCAL_BYTES, ctx->stream));
    SLAM_HIP(hipMemsetAsync(CV_AT(char, d_count_ws, y.pt_start), 0, y.pairs - y.pt_start, ctx->stream));       // pt_start and pt_end
    if (y.o64) cv_count_run<uint64_t>(ctx, y, K, L, O, d_obs_pose, d_obs_point, d_fixed, d_count_ws);
    else cv_count_run<uint32_t>(ctx, y, K, L, O, d_obs_pose, d_obs_point, d_fixed, d_count_ws);
    if (int rc = slam_launch_check("slam_covis_count")) return rc;
    uint64_t h[4];
    SLAM_HIP(hipMemcpyAsync(h, d_count_ws, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    SLAM_HIP(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < 4; ++i) h_scalars[i] = (int64_t)h[i];
    return SLAM_OK;
}

extern "C" int slam_covis_rows(slam_ctx* ctx, int64_t M, int64_t nnz, const int64_t* d_offsets, const int32_t* d_obs, int32_t* d_obs_pose,
                               int32_t* d_obs_point) {
    SLAM_REQUIRE(ctx, "slam_covis_rows: null ctx");
    SLAM_REQUIRE(M >= 1 && M <= SLAM_BAS_MAX_POINTS && nnz >= 0 && nnz <= SLAM_BAS_MAX_OBS, "slam_covis_rows: bad sizes (M=%lld, nnz=%lld)",
                 (long long)M, (long long)nnz);
    SLAM_REQUIRE(d_offsets && (nnz == 0 || (d_obs && d_obs_pose && d_obs_point)), "slam_covis_rows: null device pointer");
    SLAM_HIP(hipSetDevice(ctx->device));
    if (nnz) cv_rows<<<cv_grid(nnz), CV_THREADS, 0, ctx->stream>>>(d_offsets, d_obs, M, nnz, d_obs_pose, d_obs_point);
    return slam_launch_check("slam_covis_rows");
}

template <typename OK, typename PK>
static void cv_pairs_run(slam_ctx* ctx, const cv_layout& y, int64_t K, int64_t L, int64_t O, int64_t P, const void* cws, void* ws, int32_t* pair_a,
                         int32_t* pair_b) {
    hipStream_t st = ctx->stream;
    const int of = cv_passes(y.obits) & 1, passes = cv_passes(y.pbits), f = passes & 1;
    PK* const k[2] = {CV_AT(PK, ws, y.pk[0]), CV_AT(PK, ws, y.pk[1])};
    int32_t* a[2] = {CV_AT(int32_t, ws, y.ta), CV_AT(int32_t, ws, y.ta)};
    int32_t* b[2] = {CV_AT(int32_t, ws, y.tb), CV_AT(int32_t, ws, y.tb)};
    a[f] = pair_a;                                            // the last pass lands in the caller's tables
    b[f] = pair_b;
    cv_emit<OK, PK><<<cv_grid(P), CV_THREADS, 0, st>>>(CV_AT(const cv_u64, cws, y.pairs), (int)L, CV_AT(const int32_t, cws, y.pt_start),
                                                       CV_AT(const int32_t, cws, y.pt_end), CV_AT(const OK, cws, y.ok[of]),
                                                       CV_AT(const int32_t, cws, y.oi[of]), O, y.pb, (int)K, P, k[0], a[0], b[0]);
    cv_sort<PK, true>(st, k, a, b, P, y.pbits, CV_AT(uint32_t, ws, y.phist), CV_AT(uint32_t, ws, y.pscan2));
    uint32_t* rank = (uint32_t*)k[f ^ 1];
    cv_heads<PK><<<cv_grid(P), CV_THREADS, 0, st>>>(k[f], P, rank);
    cv_scan<uint32_t>(st, rank, P, CV_AT(uint32_t, ws, y.pscan2), (uint32_t*)ws);
}

extern "C" int slam_covis_pairs(slam_ctx* ctx, int64_t K, int64_t L, int64_t O, int64_t P, const void* d_count_ws, void* d_pair_ws,
                                int32_t* d_pair_a, int32_t* d_pair_b, int64_t* h_edges) {
    SLAM_REQUIRE(ctx && h_edges, "slam_covis_pairs: null argument");
    if (int rc = cv_sizes("slam_covis_pairs", K, L, O, P)) return rc;
    SLAM_REQUIRE(d_count_ws && d_pair_ws && (P == 0 || (d_pair_a && d_pair_b)), "slam_covis_pairs: null device pointer");
    *h_edges = 0;
    if (P == 0) return SLAM_OK;
    SLAM_REQUIRE(K >= 2 && O >= 2, "slam_covis_pairs: %lld pairs need two poses and two observations", (long long)P);
    SLAM_HIP(hipSetDevice(ctx->device));
    const cv_layout y = cv_lay(K, L, O, P);
    SLAM_HIP(hipMemsetAsync(d_pair_ws, 0, CV_SCAL_BYTES, ctx->stream));
    if (y.o64 && y.p64) cv_pairs_run<uint64_t, uint64_t>(ctx, y, K, L, O, P, d_count_ws, d_pair_ws, d_pair_a, d_pair_b);
    else if (y.o64) cv_pairs_run<uint64_t, uint32_t>(ctx, y, K, L, O, P, d_count_ws, d_pair_ws, d_pair_a, d_pair_b);
    else if (y.p64) cv_pairs_run<uint32_t, uint64_t>(ctx, y, K, L, O, P, d_count_ws, d_pair_ws, d_pair_a, d_pair_b);
    else cv_pairs_run<uint32_t, uint32_t>(ctx, y, K, L, O, P, d_count_ws, d_pair_ws, d_pair_a, d_pair_b);
    if (int rc = slam_launch_check("slam_covis_pairs")) return rc;
    uint32_t e = 0;
    SLAM_HIP(hipMemcpyAsync(&e, d_pair_ws, sizeof(e), hipMemcpyDeviceToHost, ctx->stream));
    SLAM_HIP(hipStreamSynchronize(ctx->stream));
    *h_edges = e;
    return SLAM_OK;
}

extern "C" int slam_covis_edges(slam_ctx* ctx, int64_t K, int64_t P, int64_t E, const void* d_pair_ws, int32_t* d_edges, int32_t* d_weights,
                                int32_t* d_pair_ptr) {
    SLAM_REQUIRE(ctx, "slam_covis_edges: null ctx");
    if (int rc = cv_sizes("slam_covis_edges", K, 1, 0, P)) return rc;
    SLAM_REQUIRE(E >= 0 && E <= P && E <= SLAM_PG_MAX_EDGES && (E > 0) == (P > 0), "slam_covis_edges: bad sizes (E=%lld, P=%lld)", (long long)E,
                 (long long)P);
    SLAM_REQUIRE(d_pair_ptr && (E == 0 || (d_pair_ws && d_edges && d_weights)), "slam_covis_edges: null device pointer");
    SLAM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (P == 0) {
        SLAM_HIP(hipMemsetAsync(d_pair_ptr, 0, 4, st));
        return SLAM_OK;
    }
    const cv_layout y = cv_lay(K, 1, 0, P);
    const int f = cv_passes(y.pbits) & 1;
    const uint32_t* rank = CV_AT(const uint32_t, d_pair_ws, y.pk[f ^ 1]);
    if (y.p64) cv_edges<uint64_t><<<cv_grid(P), CV_THREADS, 0, st>>>(CV_AT(const uint64_t, d_pair_ws, y.pk[f]), rank, P, E, (int)K, d_edges, d_pair_ptr);
    else cv_edges<uint32_t><<<cv_grid(P), CV_THREADS, 0, st>>>(CV_AT(const uint32_t, d_pair_ws, y.pk[f]), rank, P, E, (int)K, d_edges, d_pair_ptr);
    cv_weights<<<cv_grid(E), CV_THREADS, 0, st>>>(d_pair_ptr, E, d_weights);
    return slam_launch_check("slam_covis_edges");
}
