// bf_window.hip — window-constrained brute-force Hamming top-2 over 256-bit ORB descriptors on gfx950 (MI355X).  Replaces
// cv2.BFMatcher(NORM_HAMMING).knnMatch(query, train, k, mask=W) where W is the dense in-window matrix of a geometric search:
// train row j is a candidate for query i iff |qx_i - tx_j| <= r_j and |qy_i - ty_j| <= r_j (float32, inclusive) - the filled
// square the reference draws around each last-frame feature (utils.py:58-73, frontend.py:231-251), applied to the match of
// frontend.py:181-187 instead of to the detection.  The mask is never formed: the predicate is evaluated on the fly over the
// few train rows a cell grid leaves per query.
//
// Design, every step on the device, no read-back (the call is asynchronous on the ctx stream):
//   1. bounds   win_bounds_kernel: per block, the extent of the train centres and the largest radius over the rows that can
//               be binned (finite centre, finite radius >= 0); also clears the count tables and the merge slots.
//               win_grid_kernel (one block) turns them into the grid: square cells of side >= the largest radius, at most
//               `side` cells per axis (the cap of the plan), and the query tile edge T (cells per tile side, ~64 queries per
//               tile).  Rows with r = +inf (and a centre that is not NaN) are "wide": every query considers them.  Rows whose
//               predicate can never hold (NaN or negative radius, NaN centre, infinite centre with a finite radius) are dropped.
//   2. bin      win_count_kernel: train rows into their cell (wide rows into one extra bin), queries into their tile; one
//               exclusive scan over both histograms; win_scatter_kernel places the rows (order inside a bin is whatever the
//               atomics give: selection compares full (distance, index) keys, so it does not matter) and counts the work
//               items of every tile: ceil(queries / 64) x ceil(candidates / SLAM_WIN_CHUNK); a second scan over them.
//   3. scan     win_scan_kernel: every wave takes a contiguous range of items; an item is 64 queries of one tile (one per
//               lane) against one chunk of the tile's candidates - the train rows of the tile's cells grown by one cell on
//               every side, then the wide rows.  Candidates go through the wave's own LDS tile, 64 rows at a time (one row
//               per lane, the next tile's loads in flight while this one is read back as broadcasts).  Each lane
//               applies the exact predicate, XOR/popcount, and keeps a top-2 of keys dist << 23 | row; the pair is merged
//               into the query's slot with two 32-bit atomic minima (bf_top2_epilogue's merge): every key is distinct, so the
//               result does not depend on the order of the merges.
//   4. decode   win_decode_kernel: the slots to (idx, dist) [N, k] in the caller's query order.
// Cell indices are clamp(floor((x - x0) / cell), 0, n - 1) in double: an in-window pair is never more than one cell apart
// in either axis (cell >= r (1 + 2^-16) covers the rounding), and clamping keeps that for points outside the plane.
#include "bf_common.h"
#include <atomic>
#include <cmath>

#define SLAM_WIN_CHUNK 1024            // candidate rows per work item
#define SLAM_WIN_Q 64                  // queries per work item (one per lane)
#define SLAM_WIN_SIDE_MAX 1024         // cells per axis at most (the default cap: ceil(sqrt(M)), at most this)
#define SLAM_WIN_TILE_MAX 16           // cells per query tile side at most
#define SLAM_WIN_BOUND_BLOCKS 256      // blocks of win_bounds_kernel
#define SLAM_WIN_SCAN_PART 4096        // elements per block of the long scans
#define SLAM_WIN_WAVES_PER_CU 32       // waves of win_scan_kernel counted on per CU
#define SLAM_WIN_PLAN 10               // entries of slam_bf_window_plan_describe's h_plan

struct win_params {
    double x0, y0, cell;       // origin and side of the cells
    int nx, ny;                // cells per axis
    int tile;                  // cells per query tile side
    int ntx, nty;              // tiles per axis
    int ncell;                 // nx * ny: the wide bin's index
};

struct win_args {
    const uint4* q;            // [N] query rows (two uint4 each)
    const uint4* t;            // [M] train rows
    const float2* qxy;         // [N]
    const float2* txy;         // [M]
    const float* rad;          // [M] per-row radii, or null: rs
    float rs;
    int N, M;
    int side;                  // cells per axis at most
    int capc, capt;            // lengths of the cell and tile histograms (side^2 + 2, side^2 + 1)
    win_params* par;
    float* part;               // [SLAM_WIN_BOUND_BLOCKS][8] partial bounds
    int32_t* cnt;              // [capc + capt] counts, then their exclusive scan
    int32_t* cur;              // [capc + capt] scatter cursors
    int64_t* items;            // [capt + 1] work items per tile, then their exclusive scan
    uint4* tsd;                // [M] binned train rows
    float4* tsm;               // [M] binned (x, y, r, row as int bits)
    int32_t* qs;               // [N] query rows in tile order
    unsigned long long* best;  // [N] (1st key << 32 | 2nd key), ~0 = none
};

__device__ __forceinline__ float win_radius(const win_args& a, int j) { return a.rad ? a.rad[j] : a.rs; }

// 0 = dropped, 1 = binned, 2 = wide.  Dropped rows are those for which |q - t| <= r cannot hold for any query: r NaN or
// negative (-0.0 is not: it keeps exact positions), a NaN centre, or an infinite centre with a finite radius.
__device__ __forceinline__ int win_class(float x, float y, float r) {
    if (!(r >= 0.0f) || x != x || y != y) return 0;
    if (r == INFINITY) return 2;
    return (isfinite(x) && isfinite(y)) ? 1 : 0;
}

__device__ __forceinline__ int win_axis(float v, double v0, double cell, int n) {
    const double u = ((double)v - v0) / cell;
    if (!(u >= 0.0)) return 0;                                   // (NaN and below the plane)
    if (u >= (double)(n - 1)) return n - 1;
    return (int)u;
}

__global__ __launch_bounds__(256) void win_bounds_kernel(const win_args a, int zero_words) {
    __shared__ float red[4][5];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < zero_words; i += stride) a.cnt[i] = 0;       // cnt, then cur
    for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < a.N; i += stride) a.best[i] = ~0ull;
    float v[5] = {INFINITY, -INFINITY, INFINITY, -INFINITY, -1.0f};   // min x, max x, min y, max y, max r
    for (int64_t j = (int64_t)blockIdx.x * 256 + tid; j < a.M; j += stride) {
        const float2 c = a.txy[j];
        const float r = win_radius(a, (int)j);
        if (win_class(c.x, c.y, r) == 1) {
            v[0] = fminf(v[0], c.x); v[1] = fmaxf(v[1], c.x);
            v[2] = fminf(v[2], c.y); v[3] = fmaxf(v[3], c.y);
            v[4] = fmaxf(v[4], r);
        }
    }
#pragma unroll
    for (int k = 0; k < 5; k++) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float o = __shfl_xor(v[k], off, 64);
            v[k] = (k & 1) || k == 4 ? fmaxf(v[k], o) : fminf(v[k], o);
        }
        if (lane == 0) red[wave][k] = v[k];
    }
    __syncthreads();
    if (tid < 5) {
        float x = red[0][tid];
        for (int w = 1; w < 4; w++) x = (tid & 1) || tid == 4 ? fmaxf(x, red[w][tid]) : fminf(x, red[w][tid]);
        a.part[blockIdx.x * 8 + tid] = x;
    }
}

__global__ __launch_bounds__(64) void win_grid_kernel(const win_args a, int parts) {
    float v[5] = {INFINITY, -INFINITY, INFINITY, -INFINITY, -1.0f};
    for (int b = threadIdx.x; b < parts; b += 64) {              // (one lane alone: 45 us at 256 parts, dependent loads)
        const float* p = a.part + b * 8;
        v[0] = fminf(v[0], p[0]); v[1] = fmaxf(v[1], p[1]);
        v[2] = fminf(v[2], p[2]); v[3] = fmaxf(v[3], p[3]);
        v[4] = fmaxf(v[4], p[4]);
    }
#pragma unroll
    for (int k = 0; k < 5; k++) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float o = __shfl_xor(v[k], off, 64);
            v[k] = (k & 1) || k == 4 ? fmaxf(v[k], o) : fminf(v[k], o);
        }
    }
    if (threadIdx.x != 0) return;
    win_params g;
    if (v[4] < 0.0f) {                                           // nothing binned: one cell, only wide rows are candidates
        g.x0 = g.y0 = 0.0;
        g.cell = 1.0;
        g.nx = g.ny = 1;
    } else {
        const double ex = (double)v[1] - (double)v[0], ey = (double)v[3] - (double)v[2];
        double cell = fmax((double)v[4] * (1.0 + 1.0 / 65536.0), fmax(ex, ey) / (double)a.side);
        if (!(cell > 0.0)) cell = 1.0;                           // every binned centre at one point, radius 0
        g.x0 = v[0];
        g.y0 = v[2];
        g.cell = cell;
        g.nx = (int)fmin((double)a.side, floor(ex / cell) + 1.0);
        g.ny = (int)fmin((double)a.side, floor(ey / cell) + 1.0);
    }
    g.ncell = g.nx * g.ny;
    // tiles of about SLAM_WIN_Q queries if the queries spread like the cells
    const double per = a.N > 0 ? (double)SLAM_WIN_Q * g.ncell / (double)a.N : 1.0;
    int T = (int)floor(sqrt(per) + 0.5);
    g.tile = T < 1 ? 1 : (T > SLAM_WIN_TILE_MAX ? SLAM_WIN_TILE_MAX : T);
    g.ntx = (g.nx + g.tile - 1) / g.tile;
    g.nty = (g.ny + g.tile - 1) / g.tile;
    *a.par = g;
}

__device__ __forceinline__ int win_train_bin(const win_args& a, const win_params& g, int j) {
    const float2 c = a.txy[j];
    const int k = win_class(c.x, c.y, win_radius(a, j));
    if (k == 0) return -1;
    if (k == 2) return g.ncell;
    return win_axis(c.y, g.y0, g.cell, g.ny) * g.nx + win_axis(c.x, g.x0, g.cell, g.nx);
}

__device__ __forceinline__ int win_query_tile(const win_args& a, const win_params& g, int i) {
    const float2 c = a.qxy[i];
    const int cx = win_axis(c.x, g.x0, g.cell, g.nx), cy = win_axis(c.y, g.y0, g.cell, g.ny);
    return (cy / g.tile) * g.ntx + cx / g.tile;
}

__global__ __launch_bounds__(256) void win_count_kernel(const win_args a) {
    const win_params g = *a.par;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (int64_t)a.M + a.N; i += stride) {
        if (i < a.M) {
            const int c = win_train_bin(a, g, (int)i);
            if (c >= 0) atomicAdd(&a.cnt[c], 1);
        } else {
            atomicAdd(&a.cnt[a.capc + win_query_tile(a, g, (int)(i - a.M))], 1);
        }
    }
}

// The candidate rows of tile (tx, ty) are runs of the binned train array: for every cell row of the tile grown by one cell,
// the cells [xa, xb] of that row, then the wide bin.  Run r < nr: [S[row * nx + xa], S[row * nx + xb + 1]).
struct win_runs {
    int xa, xb, ya, yb;
};

__device__ __forceinline__ win_runs win_tile_runs(const win_params& g, int t) {
    const int tx = t % g.ntx, ty = t / g.ntx;
    win_runs r;
    r.xa = max(0, tx * g.tile - 1);
    r.xb = min(g.nx - 1, tx * g.tile + g.tile);
    r.ya = max(0, ty * g.tile - 1);
    r.yb = min(g.ny - 1, ty * g.tile + g.tile);
    return r;
}

__device__ __forceinline__ int64_t win_tile_candidates(const int32_t* S, const win_params& g, const win_runs& r) {
    int64_t c = (int64_t)S[g.ncell + 1] - S[g.ncell];
    for (int y = r.ya; y <= r.yb; y++) c += S[y * g.nx + r.xb + 1] - S[y * g.nx + r.xa];
    return c;
}

__global__ __launch_bounds__(256) void win_scatter_kernel(const win_args a) {
    const win_params g = *a.par;
    const int32_t* S = a.cnt;
    const int32_t* QS = a.cnt + a.capc;
    const int32_t qbase = QS[0];
    const int ntiles = g.ntx * g.nty;
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int64_t all = (int64_t)a.M + a.N + a.capt + 1;            // (items beyond the used tiles: 0, the scan's total lands there)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < all; i += stride) {
        if (i < a.M) {
            const int j = (int)i;
            const int c = win_train_bin(a, g, j);
            if (c < 0) continue;
            const int p = S[c] + atomicAdd(&a.cur[c], 1);
            const float2 xy = a.txy[j];
            a.tsd[2 * (size_t)p] = a.t[2 * (size_t)j];
            a.tsd[2 * (size_t)p + 1] = a.t[2 * (size_t)j + 1];
            a.tsm[p] = make_float4(xy.x, xy.y, win_radius(a, j), __int_as_float(j));
        } else if (i < (int64_t)a.M + a.N) {
            const int q = (int)(i - a.M);
            const int t = win_query_tile(a, g, q);
            a.qs[QS[t] - qbase + atomicAdd(&a.cur[a.capc + t], 1)] = q;
        } else {
            const int t = (int)(i - a.M - a.N);
            const int64_t nq = t < ntiles ? QS[t + 1] - QS[t] : 0;
            int64_t n = 0;
            if (nq > 0) {
                const int64_t c = win_tile_candidates(S, g, win_tile_runs(g, t));
                n = c > 0 ? ((nq + SLAM_WIN_Q - 1) / SLAM_WIN_Q) * ((c + SLAM_WIN_CHUNK - 1) / SLAM_WIN_CHUNK) : 0;
            }
            a.items[t] = n;
        }
    }
}

// ---- exclusive scans of the histograms and the item counts ---------------------------------------------------------

// one block: exclusive scan of d[0 .. n) in place (each thread a contiguous run), plus `add`
template <typename T>
__global__ __launch_bounds__(256) void win_scan_block_kernel(T* __restrict__ d, int64_t n) {
    __shared__ T lds4[4];
    const int64_t per = (n + 255) / 256;
    const int64_t b0 = min(n, (int64_t)threadIdx.x * per), b1 = min(n, b0 + per);
    T s = 0;
    for (int64_t i = b0; i < b1; i++) s += d[i];
    T all;
    T run = bf_block_excl_scan<T>(s, lds4, &all);
    for (int64_t i = b0; i < b1; i++) {
        const T v = d[i];
        d[i] = run;
        run += v;
    }
}

// long scans: the sum of every part of SLAM_WIN_SCAN_PART elements, then (after a block scan of the sums) each part again
template <typename T>
__global__ __launch_bounds__(256) void win_scan_sum_kernel(const T* __restrict__ d, int64_t n, T* __restrict__ bsum) {
    __shared__ T lds4[4];
    const int64_t p0 = (int64_t)blockIdx.x * SLAM_WIN_SCAN_PART;
    T s = 0;
    for (int64_t i = p0 + threadIdx.x; i < min(n, p0 + SLAM_WIN_SCAN_PART); i += 256) s += d[i];
    T all;
    (void)bf_block_excl_scan<T>(s, lds4, &all);
    if (threadIdx.x == 0) bsum[blockIdx.x] = all;
}

template <typename T>
__global__ __launch_bounds__(256) void win_scan_apply_kernel(T* __restrict__ d, int64_t n, const T* __restrict__ bsum) {
    __shared__ T lds4[4];
    constexpr int PER = SLAM_WIN_SCAN_PART / 256;
    const int64_t b0 = (int64_t)blockIdx.x * SLAM_WIN_SCAN_PART + threadIdx.x * PER;
    T v[PER];
    T s = 0;
#pragma unroll
    for (int k = 0; k < PER; k++) {
        v[k] = b0 + k < n ? d[b0 + k] : 0;
        s += v[k];
    }
    T all;
    T run = bsum[blockIdx.x] + bf_block_excl_scan<T>(s, lds4, &all);
#pragma unroll
    for (int k = 0; k < PER; k++) {
        if (b0 + k < n) d[b0 + k] = run;
        run += v[k];
    }
}

// ---- the search ----------------------------------------------------------------------------------------------------

// One wave per range of work items [it0, it1): 64 queries of one tile (a lane each) against one chunk of its candidates.
__global__ __launch_bounds__(256) void win_scan_kernel(const win_args a, int64_t capt) {
    __shared__ float4 s_m[4][SLAM_WIN_Q];
    __shared__ uint4 s_a[4][SLAM_WIN_Q], s_b[4][SLAM_WIN_Q];
    const win_params g = *a.par;
    const int lane = threadIdx.x & 63;
    float4* lm = s_m[threadIdx.x >> 6];
    uint4* la = s_a[threadIdx.x >> 6];
    uint4* lb = s_b[threadIdx.x >> 6];
    const int64_t waves = (int64_t)gridDim.x * 4;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t total = a.items[capt];
    const int64_t per = (total + waves - 1) / waves;
    const int64_t it0 = min(total, w * per), it1 = min(total, it0 + per);
    if (it0 >= it1) return;
    const int32_t* S = a.cnt;
    const int32_t* QS = a.cnt + a.capc;
    const int32_t qbase = QS[0];
    const int ntiles = g.ntx * g.nty;
    // the tile of item it0: the last t with items[t] <= it0 (items is an exclusive scan; empty tiles repeat values)
    int lo = 0, hi = ntiles - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.items[mid] <= it0) lo = mid;
        else hi = mid - 1;
    }
    int t = lo;
    for (int64_t it = it0; it < it1; it++) {
        while (a.items[t + 1] <= it) t++;                        // (tiles with no items in between)
        const win_runs rr = win_tile_runs(g, t);
        const int64_t c = win_tile_candidates(S, g, rr);
        const int64_t nchunk = (c + SLAM_WIN_CHUNK - 1) / SLAM_WIN_CHUNK;
        const int64_t local = it - a.items[t];
        const int64_t qc = local / nchunk, cc = local % nchunk;
        // this lane's query
        const int64_t qp = (int64_t)QS[t] - qbase + qc * SLAM_WIN_Q + lane;
        const bool valid = qp < (int64_t)QS[t + 1] - qbase;
        const int qi = valid ? a.qs[qp] : a.qs[(int64_t)QS[t] - qbase];   // (tail lanes: a duplicate that never merges)
        u32 qr[8];
        bf_load_query(a.q, qi, qr);
        const float2 qxy = a.qxy[qi];
        u32 b1 = SLAM_KEY_NONE, b2 = SLAM_KEY_NONE;
        // the candidate positions [cc * CHUNK, (cc + 1) * CHUNK) of the concatenated runs
        int64_t skip = cc * SLAM_WIN_CHUNK, left = min((int64_t)SLAM_WIN_CHUNK, c - skip);
        for (int y = rr.ya; y <= rr.yb + 1 && left > 0; y++) {
            int p0, p1;
            if (y <= rr.yb) {
                p0 = S[y * g.nx + rr.xa];
                p1 = S[y * g.nx + rr.xb + 1];
            } else {
                p0 = S[g.ncell];
                p1 = S[g.ncell + 1];
            }
            const int64_t len = p1 - p0;
            if (skip >= len) {
                skip -= len;
                continue;
            }
            const int s0 = __builtin_amdgcn_readfirstlane((int)(p0 + skip));
            const int s1 = __builtin_amdgcn_readfirstlane((int)min((int64_t)p1, p0 + skip + left));
            left -= s1 - s0;
            skip = 0;
            // tiles of 64 rows: one row per lane into the wave's LDS tile, the next tile's rows already in flight
            float4 nm = make_float4(0.f, 0.f, -1.f, 0.f);
            uint4 na = make_uint4(0, 0, 0, 0), nb = na;
            if (s0 + lane < s1) {
                nm = a.tsm[s0 + lane];
                na = a.tsd[2 * (size_t)(s0 + lane)];
                nb = a.tsd[2 * (size_t)(s0 + lane) + 1];
            }
            for (int base = s0; base < s1; base += SLAM_WIN_Q) {
                const int n = min(SLAM_WIN_Q, s1 - base);
                bf_wave_lds_sync();                                  // (the previous tile has been read)
                lm[lane] = nm;
                la[lane] = na;
                lb[lane] = nb;
                bf_wave_lds_sync();
                const int nx = base + SLAM_WIN_Q + lane;
                if (nx < s1) {
                    nm = a.tsm[nx];
                    na = a.tsd[2 * (size_t)nx];
                    nb = a.tsd[2 * (size_t)nx + 1];
                }
                for (int u = 0; u < n; u++) {
                    const float4 m = lm[u];
                    const uint4 ta = la[u], tb = lb[u];
                    const bool in = fabsf(qxy.x - m.x) <= m.z && fabsf(qxy.y - m.y) <= m.z;
                    u32 d = __popc(qr[0] ^ ta.x);
                    d = bcnt_acc(qr[1] ^ ta.y, d);
                    d = bcnt_acc(qr[2] ^ ta.z, d);
                    d = bcnt_acc(qr[3] ^ ta.w, d);
                    d = bcnt_acc(qr[4] ^ tb.x, d);
                    d = bcnt_acc(qr[5] ^ tb.y, d);
                    d = bcnt_acc(qr[6] ^ tb.z, d);
                    d = bcnt_acc(qr[7] ^ tb.w, d);
                    const u32 key = in ? (d << SLAM_KEY_IDX_BITS) | (u32)__float_as_int(m.w) : SLAM_KEY_NONE;
                    b2 = min(b2, max(b1, key));
                    b1 = min(b1, key);
                }
            }
        }
        // merge (bf_top2_epilogue): high half = the smallest key, low half = the second smallest, whatever the order
        if (valid && b1 != SLAM_KEY_NONE) {
            u32* half = (u32*)&a.best[qi];                       // little endian: [0] = 2nd key, [1] = 1st key
            const u32 o1 = atomicMin(half + 1, b1);
            const u32 push = min(max(o1, b1), b2);
            if (push != SLAM_KEY_NONE) atomicMin(half, push);
        }
    }
}

__global__ __launch_bounds__(256) void win_decode_kernel(const unsigned long long* __restrict__ best, int N, int k,
                                                         int32_t* __restrict__ idx, int32_t* __restrict__ dist) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= N) return;
    const unsigned long long v = best[q];
    const u32 key[2] = {(u32)(v >> 32), (u32)v};
    for (int s = 0; s < k; s++) {
        idx[(size_t)q * k + s] = bf_key_idx(key[s], 0);
        dist[(size_t)q * k + s] = bf_key_dist(key[s]);
    }
}

// ---- host side -----------------------------------------------------------

struct win_plan {
    int side;               // cells per axis at most
    int64_t capc, capt;     // histogram lengths
    int64_t parts_a;        // parts of the long scan of the histograms (0: one block)
    int64_t parts_b;        // parts of the long scan of the items (0: one block)
    int blocks;             // blocks of win_scan_kernel (4 waves each)
    // workspace layout
    uint64_t o_par, o_part, o_cnt, o_items, o_bsa, o_bsb, o_tsd, o_tsm, o_qs, o_best, bytes;
};

static int64_t win_parts(int64_t n) { return n <= 256 * 64 ? 0 : (n + SLAM_WIN_SCAN_PART - 1) / SLAM_WIN_SCAN_PART; }

// A pure function of the CU count, the shape and the cell cap (slam_bf_window_plan_describe exposes it without a device).
// cells = 0: the shipped cap, about one cell per train row (side = ceil(sqrt(M)), at most SLAM_WIN_SIDE_MAX).
static win_plan win_plan_core(int num_cu, int64_t N, int64_t M, int64_t cells) {
    win_plan p;
    int64_t side = cells > 0 ? (int64_t)std::floor(std::sqrt((double)cells)) : (int64_t)std::ceil(std::sqrt((double)M));
    while (cells > 0 && (side + 1) * (side + 1) <= cells) side++;
    while (side > 1 && side * side > (cells > 0 ? cells : side * side)) side--;
    if (side < 1) side = 1;
    if (side > SLAM_WIN_SIDE_MAX) side = SLAM_WIN_SIDE_MAX;
    p.side = (int)side;
    p.capc = side * side + 2;
    p.capt = side * side + 1;
    p.parts_a = win_parts(p.capc + p.capt);
    p.parts_b = win_parts(p.capt + 1);
    const int64_t by_items = (N + SLAM_WIN_Q - 1) / SLAM_WIN_Q + side * side;      // (at least as many items, most shapes)
    int64_t blocks = (int64_t)(num_cu > 0 ? num_cu : 1) * SLAM_WIN_WAVES_PER_CU / 4;
    const int64_t want = (by_items + 3) / 4;
    if (blocks > want) blocks = want;
    p.blocks = (int)(blocks < 1 ? 1 : blocks);
    p.o_par = 0;
    p.o_part = 256;
    p.o_cnt = p.o_part + slam_align_up(SLAM_WIN_BOUND_BLOCKS * 8 * 4);
    p.o_items = p.o_cnt + slam_align_up((uint64_t)(p.capc + p.capt) * 8);             // cnt and cur
    p.o_bsa = p.o_items + slam_align_up((uint64_t)(p.capt + 1) * 8);
    p.o_bsb = p.o_bsa + slam_align_up((uint64_t)(p.parts_a + 1) * 4);
    p.o_tsd = p.o_bsb + slam_align_up((uint64_t)(p.parts_b + 1) * 8);
    p.o_tsm = p.o_tsd + slam_align_up((uint64_t)M * SLAM_DESC_BYTES);
    p.o_qs = p.o_tsm + slam_align_up((uint64_t)M * 16);
    p.o_best = p.o_qs + slam_align_up((uint64_t)N * 4);
    p.bytes = p.o_best + slam_align_up((uint64_t)N * 8);
    return p;
}

#define SLAM_WIN_M_MAX ((1ll << SLAM_KEY_IDX_BITS) - 1)
#define SLAM_WIN_N_MAX (1ll << 28)

extern "C" int slam_bf_window_plan_describe(int num_cu, int64_t N, int64_t M, int64_t cells, int64_t* h_plan) {
    SLAM_REQUIRE(h_plan, "slam_bf_window_plan_describe: null h_plan");
    SLAM_REQUIRE(num_cu >= 1 && num_cu <= 65536, "num_cu=%d out of range", num_cu);
    SLAM_REQUIRE(N >= 0 && M >= 0 && cells >= 0, "negative size (N=%lld, M=%lld, cells=%lld)", (long long)N, (long long)M,
                 (long long)cells);
    SLAM_REQUIRE(N <= SLAM_WIN_N_MAX, "N=%lld exceeds 2^28 query rows per call", (long long)N);
    SLAM_REQUIRE(M <= SLAM_WIN_M_MAX, "M=%lld: the window search packs train rows into 23-bit keys (M < 2^23)", (long long)M);
    const win_plan p = win_plan_core(num_cu, N, M, cells);
    const int64_t v[SLAM_WIN_PLAN] = {p.side, (int64_t)p.side * p.side, p.capt - 1, SLAM_WIN_Q, SLAM_WIN_CHUNK, p.blocks,
                                      p.parts_a, p.parts_b, (int64_t)p.bytes, SLAM_WIN_TILE_MAX};
    memcpy(h_plan, v, sizeof(v));
    return SLAM_OK;
}

template <typename T>
static void win_scan(slam_ctx* ctx, T* d, int64_t n, int64_t parts, T* bsum) {
    if (parts == 0) {
        win_scan_block_kernel<T><<<1, 256, 0, ctx->stream>>>(d, n);
        return;
    }
    win_scan_sum_kernel<T><<<(unsigned)parts, 256, 0, ctx->stream>>>(d, n, bsum);
    win_scan_block_kernel<T><<<1, 256, 0, ctx->stream>>>(bsum, parts);
    win_scan_apply_kernel<T><<<(unsigned)parts, 256, 0, ctx->stream>>>(d, n, bsum);
}

static int win_check_args(slam_ctx* ctx, int64_t N, int64_t M, int k, int64_t cells, const char* fn) {
    SLAM_REQUIRE(ctx, "%s: null ctx", fn);
    SLAM_REQUIRE(N >= 0 && M >= 0 && cells >= 0, "%s: negative size (N=%lld, M=%lld, cells=%lld)", fn, (long long)N, (long long)M,
                 (long long)cells);
    SLAM_REQUIRE(N <= SLAM_WIN_N_MAX, "%s: N=%lld exceeds 2^28 query rows per call", fn, (long long)N);
    SLAM_REQUIRE(M <= SLAM_WIN_M_MAX, "%s: M=%lld: the window search packs train rows into 23-bit keys (M < 2^23)", fn,
                 (long long)M);
    SLAM_REQUIRE(k == 1 || k == 2, "%s: k=%d not in {1, 2}", fn, k);
    return SLAM_OK;
}

// slam_bf_window_knn_u256 without the call lock
static int window_search(slam_ctx* ctx, const void* d_query, int64_t N, const void* d_train, int64_t M,
                         const float* d_query_xy, const float* d_train_xy, const float* d_radius, float radius,
                         int k, int64_t cells, int32_t* d_idx, int32_t* d_dist) {
    if (int rc = win_check_args(ctx, N, M, k, cells, "slam_bf_window_knn_u256")) return rc;
    SLAM_REQUIRE(N == 0 || (d_query && d_query_xy && d_idx && d_dist), "slam_bf_window_knn_u256: null query or result pointer");
    SLAM_REQUIRE(N == 0 || M == 0 || (d_train && d_train_xy), "slam_bf_window_knn_u256: null train pointer");
    SLAM_REQUIRE(((uintptr_t)d_query & 15) == 0 && ((uintptr_t)d_train & 15) == 0, "descriptor pointers must be 16-byte aligned");
    SLAM_REQUIRE(((uintptr_t)d_query_xy & 7) == 0 && ((uintptr_t)d_train_xy & 7) == 0 && ((uintptr_t)d_radius & 3) == 0 &&
                     ((uintptr_t)d_idx & 3) == 0 && ((uintptr_t)d_dist & 3) == 0,
                 "positions must be 8-byte and radii / result pointers 4-byte aligned");
    if (N == 0) return SLAM_OK;
    SLAM_HIP(hipSetDevice(ctx->device));
    const win_plan p = win_plan_core(ctx->num_cu, N, M, cells);
    void* ws = nullptr;
    if (int rc = slam_workspace(ctx, p.bytes, &ws)) return rc;
    char* w = (char*)ws;
    win_args a;
    a.q = (const uint4*)d_query;
    a.t = (const uint4*)d_train;
    a.qxy = (const float2*)d_query_xy;
    a.txy = (const float2*)d_train_xy;
    a.rad = d_radius;
    a.rs = radius;
    a.N = (int)N;
    a.M = (int)M;
    a.side = p.side;
    a.capc = (int)p.capc;
    a.capt = (int)p.capt;
    a.par = (win_params*)(w + p.o_par);
    a.part = (float*)(w + p.o_part);
    a.cnt = (int32_t*)(w + p.o_cnt);
    a.cur = a.cnt + p.capc + p.capt;
    a.items = (int64_t*)(w + p.o_items);
    a.tsd = (uint4*)(w + p.o_tsd);
    a.tsm = (float4*)(w + p.o_tsm);
    a.qs = (int32_t*)(w + p.o_qs);
    a.best = (unsigned long long*)(w + p.o_best);
    const int64_t rows = M > N ? M : N;
    const unsigned bb = (unsigned)std::min<int64_t>(SLAM_WIN_BOUND_BLOCKS, std::max<int64_t>(1, (rows + 255) / 256));
    const int64_t zero_words = 2 * (p.capc + p.capt);
    const unsigned gb = (unsigned)std::min<int64_t>(4096, std::max<int64_t>(1, (M + N + p.capt + 255) / 256));
    SLAM_HIP(hipGetLastError());
    win_bounds_kernel<<<bb, 256, 0, ctx->stream>>>(a, (int)zero_words);
    win_grid_kernel<<<1, 64, 0, ctx->stream>>>(a, (int)bb);
    win_count_kernel<<<gb, 256, 0, ctx->stream>>>(a);
    win_scan<int32_t>(ctx, a.cnt, p.capc + p.capt, p.parts_a, (int32_t*)(w + p.o_bsa));
    win_scatter_kernel<<<gb, 256, 0, ctx->stream>>>(a);
    win_scan<int64_t>(ctx, a.items, p.capt + 1, p.parts_b, (int64_t*)(w + p.o_bsb));
    if (int rc = slam_launch_check("window binning")) return rc;
    if (int rc = slam_prof_begin(ctx)) return rc;
    win_scan_kernel<<<(unsigned)p.blocks, 256, 0, ctx->stream>>>(a, p.capt);
    if (int rc = slam_prof_end(ctx)) return rc;
    win_decode_kernel<<<(unsigned)((N + 255) / 256), 256, 0, ctx->stream>>>(a.best, (int)N, k, d_idx, d_dist);
    return slam_launch_check("window search");
}

extern "C" int slam_bf_window_knn_u256(slam_ctx* ctx, const void* d_query, int64_t N, const void* d_train, int64_t M,
                                       const float* d_query_xy, const float* d_train_xy, const float* d_radius, float radius,
                                       int k, int64_t cells, int32_t* d_idx, int32_t* d_dist) {
    if (int rc = win_check_args(ctx, N, M, k, cells, "slam_bf_window_knn_u256")) return rc;   // (before the context is touched)
    std::lock_guard<std::mutex> lk(ctx->call_mu);
    return window_search(ctx, d_query, N, d_train, M, d_query_xy, d_train_xy, d_radius, radius, k, cells, d_idx, d_dist);
}

// upload, search, download, one stream synchronisation (through the context's host-buffer arena)
extern "C" int slam_bf_window_knn_u256_host(slam_ctx* ctx, const uint8_t* h_query, int64_t N, const uint8_t* h_train, int64_t M,
                                            const float* h_query_xy, const float* h_train_xy, const float* h_radius, float radius,
                                            int k, int64_t cells, int32_t* h_idx, int32_t* h_dist) {
    if (int rc = win_check_args(ctx, N, M, k, cells, "slam_bf_window_knn_u256_host")) return rc;
    SLAM_REQUIRE(N == 0 || (h_query && h_query_xy && h_idx && h_dist), "slam_bf_window_knn_u256_host: null query or result pointer");
    SLAM_REQUIRE(M == 0 || (h_train && h_train_xy), "slam_bf_window_knn_u256_host: null train pointer");
    if (N == 0) return SLAM_OK;
    std::lock_guard<std::mutex> lk(ctx->call_mu);
    SLAM_HIP(hipSetDevice(ctx->device));
    const uint64_t qb = (uint64_t)N * SLAM_DESC_BYTES, tb = (uint64_t)M * SLAM_DESC_BYTES, qxb = (uint64_t)N * 8,
                   txb = (uint64_t)M * 8, rb = h_radius ? (uint64_t)M * 4 : 0, ob = (uint64_t)N * k * 4;
    const uint64_t o_t = slam_align_up(qb), o_qx = o_t + slam_align_up(tb), o_tx = o_qx + slam_align_up(qxb), o_r = o_tx + slam_align_up(txb),
                   in_bytes = o_r + rb, o_i = slam_align_up(in_bytes), o_d = o_i + slam_align_up(ob), total = o_d + slam_align_up(ob);
    void *dev = nullptr, *host = nullptr;
    if (int rc = slam_io_arena(ctx, total, total, &dev, &host)) return rc;
    uint8_t* hb = (uint8_t*)host;
    uint8_t* db = (uint8_t*)dev;
    memcpy(hb, h_query, qb);
    if (tb) memcpy(hb + o_t, h_train, tb);
    memcpy(hb + o_qx, h_query_xy, qxb);
    if (txb) memcpy(hb + o_tx, h_train_xy, txb);
    if (rb) memcpy(hb + o_r, h_radius, rb);
    ctx->io_h2d_bytes += qb + tb + qxb + txb + rb;
    SLAM_HIP(hipMemcpyAsync(db, hb, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (int rc = window_search(ctx, db, N, M ? db + o_t : nullptr, M, (const float*)(db + o_qx),
                                         M ? (const float*)(db + o_tx) : nullptr, rb ? (const float*)(db + o_r) : nullptr, radius,
                                         k, cells, (int32_t*)(db + o_i), (int32_t*)(db + o_d)))
        return rc;
    SLAM_HIP(hipMemcpyAsync(hb + o_i, db + o_i, o_d + ob - o_i, hipMemcpyDeviceToHost, ctx->stream));
    SLAM_HIP(hipStreamSynchronize(ctx->stream));
    ctx->io_d2h_bytes += 2 * ob;
    memcpy(h_idx, hb + o_i, ob);
    memcpy(h_dist, hb + o_d, ob);
    return SLAM_OK;
}
