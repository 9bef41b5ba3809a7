// bow.hip - bag-of-words place recognition for 256-bit descriptors: the descent of a k-ary vocabulary tree
// (DBoW2's TemplatedVocabulary::transform), the tf-idf vectors of a batch of images (TF_IDF, L1_NORM), the inverted index of
// a keyframe database and its L1 query in fixed point (TemplatedDatabase::queryL1), and the kernels of a deterministic
// hierarchical k-majority training (HKmeansStep with maximin seeding in place of k-means++).
//
// Every result is a function of its inputs alone: distances and scores are integers, ties are decided by index or by packed
// keys, all atomics are integer atomics whose sum, minimum or maximum does not depend on the order they land in, and the one
// floating-point sum (the L1 norm of a vector) is taken in a fixed order with contraction off (the pragma below, as in
// sim3.hip).  Nothing is kept between launches: every buffer is the caller's, so no entry point takes the context's call lock.
#include "bf_common.h"

#pragma clang fp contract(off)

typedef unsigned long long u64;

#define BOW_THREADS 256
#define BOW_STAGE_NODES 1152        // node rows of the tree's top staged in LDS by the transform: 36 KiB (k = 10: depths 0-3, 1111 rows)
#define BOW_K_MAX 32
#define BOW_DEPTH_MAX 10
#define BOW_IMAGE_MAX 8192          // descriptors of one image (the LDS sort of bow_vectors_kernel)
#define BOW_Q_THREADS 1024
#define BOW_Q_CAP 18432             // database entries per LDS pass of the query: two u32 tables of 72 KiB
#define BOW_RESULTS_MAX 64
#define BOW_MAJ_ROWS 512            // rows of one majority workgroup
#define BOW_LANES16_UP_TO 65536     // slam_bow_transform with lanes = 0: sixteen lanes per descriptor up to this many descriptors, one lane beyond
                                    // (k = 10, L = 6: 7.8 against 18.2 us at 2000, 10.1 against 20.9 at 16 000, level at 64 000, 43.7 against 39.7 at 128 000; profiles/bow_time.log)

// ------------------------------------------------------------------------------------------------ nearest child of a node
// The index (0-based, within the group) of the row nearest to q among rows[first .. first + count): the smallest Hamming
// distance, the lowest index on ties (DBoW2 scans the children in order with a strict <).  Rows are requested eight at a
// time before the first distance of the eight is formed.
template <bool LDS>
__device__ __forceinline__ int bow_nearest(const u32 (&q)[8], const uint4* rows, int first, int count) {
    u32 best = 0xFFFFFFFFu;
    int arg = 0;
    for (int c0 = 0; c0 < count; c0 += 8) {
        uint4 a[8], b[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const size_t r = (size_t)(first + min(c0 + u, count - 1));
            a[u] = rows[2 * r];
            b[u] = rows[2 * r + 1];
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const u32 d = bf_hamming256(q, a[u], b[u]);
            if (c0 + u < count && d < best) {
                best = d;
                arg = c0 + u;
            }
        }
    }
    return arg;
}

__device__ __forceinline__ u32 bow_distance(const u32 (&q)[8], const uint4* rows, size_t r) {
    const uint4 a = rows[2 * r], b = rows[2 * r + 1];
    return bf_hamming256(q, a, b);
}

// ------------------------------------------------------------------------------------------------------------ transform
// One lane per descriptor.  child[v] = (first child, child count) of node v; the rows of the first `staged` nodes are read
// from LDS (a breadth-first tree has its top levels there), every other group of children from memory.  The loop is bounded
// by the depth, and node ids are clamped, so that a malformed tree can neither spin nor read out of bounds.
__global__ __launch_bounds__(BOW_THREADS) void bow_transform_kernel(const uint4* __restrict__ desc, int n, const uint4* __restrict__ rows,
                                                                   const int2* __restrict__ child, const int* __restrict__ word_of_node,
                                                                   int n_nodes, int depth, int node_depth, int* __restrict__ words,
                                                                   int* __restrict__ nodes) {
    __shared__ uint4 s_rows[2 * BOW_STAGE_NODES];
    const int staged = min(n_nodes, BOW_STAGE_NODES);
    for (int i = threadIdx.x; i < 2 * staged; i += BOW_THREADS) s_rows[i] = rows[i];
    __syncthreads();
    const int i = blockIdx.x * BOW_THREADS + threadIdx.x;
    if (i >= n) return;
    u32 q[8];
    bf_load_query(desc, i, q);
    int cur = 0, at = 0;
    for (int d = 1; d <= depth; d++) {
        const int2 ch = child[cur];
        if (ch.y <= 0) break;
        const int first = min(max(ch.x, 0), n_nodes - 1), count = min(min(ch.y, BOW_K_MAX), n_nodes - first);
        cur = first + (first + count <= staged ? bow_nearest<true>(q, s_rows, first, count) : bow_nearest<false>(q, rows, first, count));
        if (d <= node_depth) at = cur;
    }
    words[i] = word_of_node[cur];
    nodes[i] = at;
}

// The second mapping: sixteen lanes per descriptor, one child per lane (two for k > 16), the minimum of (distance << 8 | child)
// taken across the sixteen lanes - the smallest distance, then the lowest child.  A step of the descent is then one coalesced
// read of the k contiguous child rows per descriptor instead of k reads per lane, and a batch of n descriptors spreads over
// n / 4 waves instead of n / 64.  Nothing is staged: 16 descriptors per workgroup would not repay 36 KiB.  All lanes of a wave
// walk the levels together (a group whose descriptor has reached its leaf idles), so the exchanges never meet a retired lane.
__global__ __launch_bounds__(BOW_THREADS) void bow_transform16_kernel(const uint4* __restrict__ desc, int n, const uint4* __restrict__ rows,
                                                                     const int2* __restrict__ child, const int* __restrict__ word_of_node,
                                                                     int n_nodes, int depth, int node_depth, int* __restrict__ words,
                                                                     int* __restrict__ nodes) {
    const int g = (int)(((size_t)blockIdx.x * BOW_THREADS + threadIdx.x) >> 4), c = threadIdx.x & 15;
    u32 q[8];
    bf_load_query(desc, min(g, n - 1), q);
    int cur = 0, at = 0;
    for (int d = 1; d <= depth; d++) {
        const int2 ch = child[cur];
        const bool moving = ch.y > 0;
        if (!__any(moving)) break;
        const int first = min(max(ch.x, 0), n_nodes - 1), count = moving ? min(min(ch.y, BOW_K_MAX), n_nodes - first) : 0;
        u32 key = 0xFFFFFFFFu;
        for (int c0 = c; c0 < count; c0 += 16) key = min(key, (bow_distance(q, rows, (size_t)(first + c0)) << 8) | (u32)c0);
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) key = min(key, (u32)__shfl_xor((int)key, off, 16));
        if (moving) {
            cur = first + (int)(key & 0xFFu);
            if (d <= node_depth) at = cur;
        }
    }
    if (c == 0 && g < n) {
        words[g] = word_of_node[cur];
        nodes[g] = at;
    }
}

// -------------------------------------------------------------------------------------------------------------- vectors
// One workgroup per image: bitonic sort of the word ids in LDS, runs of equal ids, tf-idf weights, the L1 norm in the order
// of the specification, the division and the fixed-point value.  Image b writes its K_b <= n_b entries at the offset of its
// first descriptor (one slot per descriptor: the worst case) and K_b into count[b]; bow_compact_kernel closes the gaps.
__global__ __launch_bounds__(BOW_THREADS) void bow_vectors_kernel(const int* __restrict__ words_in, const int64_t* __restrict__ offsets,
                                                                 const double* __restrict__ idf, int n_words, int* raw_words,
                                                                 double* raw_values, u32* raw_q, int* __restrict__ count) {
    __shared__ u32 s_w[BOW_IMAGE_MAX];
    __shared__ u32 s_uw[BOW_IMAGE_MAX];
    __shared__ u32 s_us[BOW_IMAGE_MAX + 1];
    __shared__ double s_p[64];
    __shared__ int s_scan[4];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int64_t base = offsets[b];
    const int n = (int)min((int64_t)BOW_IMAGE_MAX, offsets[b + 1] - base);
    if (n <= 0) {
        if (tid == 0) count[b] = 0;
        return;
    }
    int P = 2;
    while (P < n) P <<= 1;
    for (int i = tid; i < P; i += BOW_THREADS) s_w[i] = i < n ? (u32)words_in[base + i] : 0xFFFFFFFFu;
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (P >> 1); t += BOW_THREADS) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const u32 x = s_w[lo], y = s_w[hi];
                if ((x > y) == ((lo & size) == 0)) {
                    s_w[lo] = y;
                    s_w[hi] = x;
                }
            }
            __syncthreads();
        }
    // distinct words and where their runs start
    const int per = (n + BOW_THREADS - 1) / BOW_THREADS, j0 = min(n, tid * per), j1 = min(n, j0 + per);
    int heads = 0;
    for (int j = j0; j < j1; j++) heads += (j == 0 || s_w[j] != s_w[j - 1]) ? 1 : 0;
    int U;
    int pos = bf_block_excl_scan(heads, s_scan, &U);
    for (int j = j0; j < j1; j++)
        if (j == 0 || s_w[j] != s_w[j - 1]) {
            s_uw[pos] = s_w[j];
            s_us[pos] = (u32)j;
            pos++;
        }
    if (tid == 0) s_us[U] = (u32)n;
    __syncthreads();
    // weights; the words whose weight is not positive leave the list
    const int per2 = (U + BOW_THREADS - 1) / BOW_THREADS, u0 = min(U, tid * per2), u1 = min(U, u0 + per2);
    int kept = 0;
    for (int u = u0; u < u1; u++) {
        const u32 w = s_uw[u];
        const double t = w < (u32)n_words ? (double)(s_us[u + 1] - s_us[u]) * idf[w] : 0.0;
        kept += t > 0.0 ? 1 : 0;
    }
    int K;
    int kp = bf_block_excl_scan(kept, s_scan, &K);
    for (int u = u0; u < u1; u++) {
        const u32 w = s_uw[u];
        const double t = w < (u32)n_words ? (double)(s_us[u + 1] - s_us[u]) * idf[w] : 0.0;
        if (t > 0.0) {
            raw_words[base + kp] = (int)w;
            raw_values[base + kp] = t;
            kp++;
        }
    }
    __syncthreads();                                    // the weights written above are read back by other threads of this block
    if (tid < 64) {
        double p = 0.0;
        for (int j = tid; j < K; j += 64) p = p + raw_values[base + j];
        s_p[tid] = p;
    }
    __syncthreads();
    double S = s_p[0];
    for (int l = 1; l < 64; l++) S = S + s_p[l];
    for (int j = tid; j < K; j += BOW_THREADS) {
        const double v = raw_values[base + j] / S;
        raw_values[base + j] = v;
        raw_q[base + j] = (u32)(v * 2147483648.0);       // floor of a value in [0, 2^31]
    }
    if (tid == 0) count[b] = K;
}

// out_off[0 .. B] = exclusive scan of count[0 .. B) in int64 (one workgroup)
__global__ __launch_bounds__(BOW_THREADS) void bow_offsets_kernel(const int* __restrict__ count, int64_t B, int64_t* __restrict__ out_off) {
    __shared__ int64_t s_scan[4];
    int64_t carry = 0;
    for (int64_t t0 = 0; t0 < B; t0 += BOW_THREADS) {
        const int64_t i = t0 + threadIdx.x;
        const int64_t v = i < B ? (int64_t)count[i] : 0;
        int64_t total;
        const int64_t ex = bf_block_excl_scan(v, s_scan, &total);
        if (i < B) out_off[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) out_off[B] = carry;
}

__global__ __launch_bounds__(BOW_THREADS) void bow_compact_kernel(const int64_t* __restrict__ offsets, const int64_t* __restrict__ out_off,
                                                                 const int* __restrict__ raw_words, const double* __restrict__ raw_values,
                                                                 const u32* __restrict__ raw_q, int* __restrict__ words,
                                                                 double* __restrict__ values, u32* __restrict__ q) {
    const int b = blockIdx.x;
    const int64_t src = offsets[b], dst = out_off[b];
    const int K = (int)(out_off[b + 1] - dst);
    for (int j = threadIdx.x; j < K; j += BOW_THREADS) {
        words[dst + j] = raw_words[src + j];
        values[dst + j] = raw_values[src + j];
        q[dst + j] = raw_q[src + j];
    }
}

// -------------------------------------------------------------------------------------------------------- counting sort
// Items grouped by key (0 <= key < n_keys; any other key leaves the item out): a histogram by integer atomics, an exclusive
// scan, a scatter with atomic cursors.  The order of the items inside a key depends on the order the atomics land in; no
// caller relies on it.
__global__ __launch_bounds__(BOW_THREADS) void bow_hist_kernel(const int* __restrict__ keys, int64_t n, int n_keys, int* __restrict__ hist) {
    const int64_t i = (int64_t)blockIdx.x * BOW_THREADS + threadIdx.x;
    if (i >= n) return;
    const int k = keys[i];
    if ((u32)k < (u32)n_keys) atomicAdd(&hist[k], 1);
}

// in place: a[0 .. n) -> exclusive scan, a[n] = total (one workgroup, 16 consecutive elements per thread and tile)
__global__ __launch_bounds__(BOW_THREADS) void bow_scan_kernel(int* a, int n) {
    __shared__ int s_scan[4];
    int carry = 0;
    for (int t0 = 0; t0 < n; t0 += BOW_THREADS * 16) {
        const int j0 = t0 + threadIdx.x * 16;
        int v[16], sum = 0;
#pragma unroll
        for (int u = 0; u < 16; u++) {
            v[u] = j0 + u < n ? a[j0 + u] : 0;
            sum += v[u];
        }
        int total;
        int run = carry + bf_block_excl_scan(sum, s_scan, &total);
#pragma unroll
        for (int u = 0; u < 16; u++) {
            if (j0 + u < n) a[j0 + u] = run;
            run += v[u];
        }
        carry += total;
    }
    if (threadIdx.x == 0) a[n] = carry;
}

__global__ __launch_bounds__(BOW_THREADS) void bow_scatter_kernel(const int* __restrict__ keys, int64_t n, int n_keys,
                                                                 const int* __restrict__ key_off, int* __restrict__ cursor,
                                                                 int* __restrict__ perm) {
    const int64_t i = (int64_t)blockIdx.x * BOW_THREADS + threadIdx.x;
    if (i >= n) return;
    const int k = keys[i];
    if ((u32)k < (u32)n_keys) perm[key_off[k] + atomicAdd(&cursor[k], 1)] = (int)i;
}

__global__ __launch_bounds__(BOW_THREADS) void bow_postings_kernel(const int* __restrict__ perm, int64_t T, const int* __restrict__ entry,
                                                                  const u32* __restrict__ q, uint2* __restrict__ post) {
    const int64_t p = (int64_t)blockIdx.x * BOW_THREADS + threadIdx.x;
    if (p >= T) return;
    const int t = perm[p];
    post[p] = make_uint2((u32)entry[t], q[t]);
}

// ---------------------------------------------------------------------------------------------------------------- query
// One workgroup per query vector.  The entries are taken in ranges of BOW_Q_CAP; for one range the u32 tables s_acc (sum of
// min(q, p): at most 2^31, so no carry) and s_cnt (shared words) live in LDS, a wave takes every 16th query word and its lanes
// stride over the word's postings.  The best `R` of all ranges so far are kept as packed keys (s_int + 1) << 32 | ~id (0 = none:
// a larger key is a better score, then a lower id) and re-selected after every range by R block-wide maxima below the
// previous one.  Dense form (dense_s != null): the tables are written out instead.
__global__ __launch_bounds__(BOW_Q_THREADS) void bow_query_kernel(const int64_t* __restrict__ q_off, const int* __restrict__ q_words,
                                                                 const u32* __restrict__ q_q, const int* __restrict__ word_off,
                                                                 const uint2* __restrict__ post, int n_words, int E, int limit, int R,
                                                                 int* __restrict__ out_ids, u32* __restrict__ out_s,
                                                                 int* __restrict__ out_common, u32* __restrict__ dense_s,
                                                                 int* __restrict__ dense_c) {
    __shared__ u32 s_acc[BOW_Q_CAP];
    __shared__ u32 s_cnt[BOW_Q_CAP];
    __shared__ u64 s_prev[BOW_RESULTS_MAX], s_new[BOW_RESULTS_MAX], s_red[BOW_Q_THREADS / 64];
    __shared__ int s_prevc[BOW_RESULTS_MAX], s_newc[BOW_RESULTS_MAX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, qi = blockIdx.x;
    const int64_t qb = q_off[qi];
    const int nq = (int)(q_off[qi + 1] - qb);
    if (tid < BOW_RESULTS_MAX) {
        s_prev[tid] = 0;
        s_prevc[tid] = 0;
    }
    for (int lo = 0; lo < limit; lo += BOW_Q_CAP) {
        const int hi = min(limit, lo + BOW_Q_CAP), m = hi - lo;
        for (int j = tid; j < m; j += BOW_Q_THREADS) {
            s_acc[j] = 0;
            s_cnt[j] = 0;
        }
        __syncthreads();
        for (int i = wave; i < nq; i += BOW_Q_THREADS / 64) {
            const int w = q_words[qb + i];
            if ((u32)w >= (u32)n_words) continue;
            const u32 qv = q_q[qb + i];
            const int pe = word_off[w + 1];
            for (int p = word_off[w] + lane; p < pe; p += 64) {
                const uint2 e = post[p];
                if (e.x >= (u32)lo && e.x < (u32)hi) {
                    atomicAdd(&s_acc[e.x - lo], min(qv, e.y));
                    atomicAdd(&s_cnt[e.x - lo], 1u);
                }
            }
        }
        __syncthreads();
        if (dense_s) {
            for (int j = tid; j < m; j += BOW_Q_THREADS) {
                dense_s[(size_t)qi * E + lo + j] = s_acc[j];
                dense_c[(size_t)qi * E + lo + j] = (int)s_cnt[j];
            }
            __syncthreads();
            continue;
        }
        u64 bound = ~0ull;
        for (int r = 0; r < R; r++) {
            u64 best = 0;
            for (int j = tid; j < m; j += BOW_Q_THREADS)
                if (s_cnt[j]) {
                    const u64 key = ((u64)(s_acc[j] + 1u) << 32) | (u32)~(u32)(lo + j);
                    if (key < bound && key > best) best = key;
                }
            if (tid < BOW_RESULTS_MAX) {
                const u64 key = s_prev[tid];
                if (key < bound && key > best) best = key;
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const u64 o = __shfl_xor(best, off, 64);
                best = o > best ? o : best;
            }
            if (lane == 0) s_red[wave] = best;
            __syncthreads();
            best = s_red[0];
#pragma unroll
            for (int w = 1; w < BOW_Q_THREADS / 64; w++) best = s_red[w] > best ? s_red[w] : best;
            if (tid == 0) {
                int c = 0;
                if (best) {
                    const u32 id = ~(u32)best;
                    if (id >= (u32)lo && id < (u32)hi) c = (int)s_cnt[id - lo];
                    else
                        for (int t = 0; t < BOW_RESULTS_MAX; t++)
                            if (s_prev[t] == best) c = s_prevc[t];
                }
                s_new[r] = best;
                s_newc[r] = c;
            }
            bound = best;                                   // (best == 0: nothing is below it, the remaining slots come out empty)
            __syncthreads();
        }
        if (tid < BOW_RESULTS_MAX) {
            s_prev[tid] = tid < R ? s_new[tid] : 0;
            s_prevc[tid] = tid < R ? s_newc[tid] : 0;
        }
        __syncthreads();
    }
    if (!dense_s && tid < R) {
        const u64 key = s_prev[tid];
        out_ids[(size_t)qi * R + tid] = key ? (int)~(u32)key : -1;
        out_s[(size_t)qi * R + tid] = key ? (u32)(key >> 32) - 1u : 0u;
        out_common[(size_t)qi * R + tid] = key ? s_prevc[tid] : 0;
    }
}

// ------------------------------------------------------------------------------------------------------------- training
// All nodes of one depth at once.  row_node[i] is the node (index within the depth) that row i belongs to, or -1 once the row
// has reached a leaf; node f owns the k centre rows cent[f * k ..] of which cent_count[f] are in use.

__global__ __launch_bounds__(BOW_THREADS) void bow_first_row_kernel(const int* __restrict__ row_node, int n, u32* __restrict__ first) {
    const int i = blockIdx.x * BOW_THREADS + threadIdx.x;
    if (i >= n) return;
    const int f = row_node[i];
    if (f >= 0) atomicMin(&first[f], (u32)i);
}

__device__ __forceinline__ void bow_copy_row(uint4* dst, size_t d, const uint4* src, size_t s) {
    dst[2 * d] = src[2 * s];
    dst[2 * d + 1] = src[2 * s + 1];
}

__global__ __launch_bounds__(BOW_THREADS) void bow_seed_init_kernel(const uint4* __restrict__ desc, int n, const u32* __restrict__ first, int F,
                                                                   int k, uint4* __restrict__ cent, int* __restrict__ cent_count,
                                                                   int* __restrict__ alive, u64* __restrict__ best) {
    const int f = blockIdx.x * BOW_THREADS + threadIdx.x;
    if (f >= F) return;
    const bool has = first[f] < (u32)n;
    if (has) bow_copy_row(cent, (size_t)f * k, desc, first[f]);
    cent_count[f] = has ? 1 : 0;
    alive[f] = has ? 1 : 0;
    best[f] = 0;
}

// maximin step j >= 1, the rows' half: the distance to the centres so far (centre j - 1 is the new one), and the node's
// arg-max of it as an integer atomic maximum of (distance << 32 | ~row): the largest distance, then the first row
__global__ __launch_bounds__(BOW_THREADS) void bow_seed_far_kernel(const uint4* __restrict__ desc, int n, const int* __restrict__ row_node,
                                                                  const uint4* __restrict__ cent, const int* __restrict__ alive, int k, int j,
                                                                  u32* __restrict__ mind, u64* __restrict__ best) {
    const int i = blockIdx.x * BOW_THREADS + threadIdx.x;
    if (i >= n) return;
    const int f = row_node[i];
    if (f < 0 || !alive[f]) return;
    u32 q[8];
    bf_load_query(desc, i, q);
    u32 d = bow_distance(q, cent, (size_t)f * k + j - 1);
    if (j > 1) d = min(d, mind[i]);
    mind[i] = d;
    atomicMax(&best[f], ((u64)d << 32) | (u32)~(u32)i);
}

// the nodes' half: the farthest row becomes centre j unless it lies at distance 0, which ends the node's seeding
__global__ __launch_bounds__(BOW_THREADS) void bow_seed_pick_kernel(const uint4* __restrict__ desc, int F, int k, int j, uint4* __restrict__ cent,
                                                                   int* __restrict__ cent_count, int* __restrict__ alive,
                                                                   u64* __restrict__ best) {
    const int f = blockIdx.x * BOW_THREADS + threadIdx.x;
    if (f >= F || !alive[f]) return;
    const u64 key = best[f];
    best[f] = 0;
    if ((key >> 32) > 0) {
        bow_copy_row(cent, (size_t)f * k + j, desc, (size_t)~(u32)key);
        cent_count[f] = j + 1;
    } else {
        alive[f] = 0;
    }
}

// the transform restricted to one level: nearest of the node's centres, lowest index on ties; counts the rows that moved
__global__ __launch_bounds__(BOW_THREADS) void bow_assign_kernel(const uint4* __restrict__ desc, int n, const int* __restrict__ row_node,
                                                                const uint4* __restrict__ cent, const int* __restrict__ cent_count, int k,
                                                                int* __restrict__ assign, u32* __restrict__ changed) {
    const int i = blockIdx.x * BOW_THREADS + threadIdx.x;
    bool moved = false;
    if (i < n) {
        const int f = row_node[i];
        if (f >= 0) {
            u32 q[8];
            bf_load_query(desc, i, q);
            const int a = bow_nearest<false>(q, cent, f * k, min(max(cent_count[f], 1), k));
            moved = a != assign[i];
            assign[i] = a;
        }
    }
    const u64 votes = __ballot(moved);
    if ((threadIdx.x & 63) == 0 && votes) atomicAdd(changed, (u32)__popcll(votes));
}

// Bit counts per centre.  perm lists the live rows grouped by node; a workgroup takes BOW_MAJ_ROWS consecutive positions and
// walks the node segments inside them.  Thread b owns bit b (word b / 32, bit b % 32) of every centre's counters in LDS, so
// the counting needs no atomics; the partial counts go to memory by integer atomic adds.
__global__ __launch_bounds__(BOW_THREADS) void bow_majority_kernel(const u32* __restrict__ desc, const int* __restrict__ perm, int n_live,
                                                                  const int* __restrict__ row_node, const int* __restrict__ assign, int k,
                                                                  u32* __restrict__ bits, u32* __restrict__ rows_of) {
    __shared__ u32 s_cnt[BOW_K_MAX * 256];
    __shared__ u32 s_n[BOW_K_MAX];
    __shared__ int s_row[BOW_MAJ_ROWS], s_node[BOW_MAJ_ROWS], s_as[BOW_MAJ_ROWS];
    const int b = threadIdx.x, p0 = blockIdx.x * BOW_MAJ_ROWS, m = min(BOW_MAJ_ROWS, n_live - p0);
    for (int p = b; p < m; p += BOW_THREADS) {
        const int r = perm[p0 + p];
        s_row[p] = r;
        s_node[p] = row_node[r];
        s_as[p] = min(max(assign[r], 0), k - 1);
    }
    __syncthreads();
    int p = 0;
    while (p < m) {
        const int f = s_node[p];
        for (int c = 0; c < k; c++) s_cnt[c * 256 + b] = 0;
        if (b < k) s_n[b] = 0;
        __syncthreads();
        for (; p < m && s_node[p] == f; p++) {
            const u32 w = desc[(size_t)s_row[p] * 8 + (b >> 5)];
            s_cnt[s_as[p] * 256 + b] += (w >> (b & 31)) & 1u;
            if (b == 0) s_n[s_as[p]]++;
        }
        __syncthreads();
        for (int c = 0; c < k; c++) {
            const u32 v = s_cnt[c * 256 + b];
            if (v) atomicAdd(&bits[((size_t)f * k + c) * 256 + b], v);
        }
        if (b < k && s_n[b]) atomicAdd(&rows_of[(size_t)f * k + b], s_n[b]);
        __syncthreads();
    }
}

// one workgroup per centre: a bit is set iff 2 * count >= rows (DBoW2's meanValue); a centre without rows keeps its value
__global__ __launch_bounds__(BOW_THREADS) void bow_update_kernel(const u32* __restrict__ bits, const u32* __restrict__ rows_of,
                                                                u32* __restrict__ cent) {
    const int g = blockIdx.x, b = threadIdx.x;
    const u32 m = rows_of[g];
    if (m == 0) return;
    const u64 set = __ballot(2u * bits[(size_t)g * 256 + b] >= m);
    if ((b & 63) == 0) {
        cent[(size_t)g * 8 + 2 * (b >> 6)] = (u32)set;
        cent[(size_t)g * 8 + 2 * (b >> 6) + 1] = (u32)(set >> 32);
    }
}

__global__ __launch_bounds__(BOW_THREADS) void bow_own_kernel(const int* __restrict__ row_node, const int* __restrict__ assign, int n, int k,
                                                             u32* __restrict__ own) {
    const int i = blockIdx.x * BOW_THREADS + threadIdx.x;
    if (i >= n) return;
    const int f = row_node[i];
    if (f >= 0) atomicAdd(&own[(size_t)f * k + min(max(assign[i], 0), k - 1)], 1u);
}

__global__ __launch_bounds__(BOW_THREADS) void bow_relabel_kernel(int* __restrict__ row_node, const int* __restrict__ assign, int n, int k,
                                                                 const int* __restrict__ next_of) {
    const int i = blockIdx.x * BOW_THREADS + threadIdx.x;
    if (i >= n) return;
    const int f = row_node[i];
    if (f >= 0) row_node[i] = next_of[(size_t)f * k + min(max(assign[i], 0), k - 1)];
}

// =============================================================== entry points ================================================
static inline unsigned bow_blocks(int64_t n) { return (unsigned)((n + BOW_THREADS - 1) / BOW_THREADS); }

extern "C" int slam_bow_limits(int32_t* h_limits) {
    SLAM_REQUIRE(h_limits, "slam_bow_limits: null pointer");
    h_limits[0] = BOW_K_MAX;
    h_limits[1] = BOW_DEPTH_MAX;
    h_limits[2] = BOW_IMAGE_MAX;
    h_limits[3] = BOW_RESULTS_MAX;
    h_limits[4] = BOW_Q_CAP;
    h_limits[5] = BOW_STAGE_NODES;
    h_limits[6] = BOW_LANES16_UP_TO;
    return SLAM_OK;
}

extern "C" int slam_bow_transform(slam_ctx* ctx, const void* d_desc, int64_t n, const void* d_node_desc, const int32_t* d_child,
                                  const int32_t* d_word_of_node, int64_t n_nodes, int depth, int levels_up, int lanes, int32_t* d_words,
                                  int32_t* d_nodes) {
    SLAM_REQUIRE(ctx, "slam_bow_transform: null ctx");
    SLAM_REQUIRE(n >= 0 && n <= (1ll << 30), "n=%lld out of range [0, 2^30]", (long long)n);
    SLAM_REQUIRE(n_nodes >= 1 && n_nodes <= (1ll << 28), "n_nodes=%lld out of range [1, 2^28]", (long long)n_nodes);
    SLAM_REQUIRE(depth >= 1 && depth <= BOW_DEPTH_MAX && levels_up >= 0, "depth=%d (1..%d) or levels_up=%d (>= 0) out of range", depth,
                 BOW_DEPTH_MAX, levels_up);
    SLAM_REQUIRE(lanes == 0 || lanes == 1 || lanes == 16, "lanes=%d: 0 (auto), 1 or 16 lanes per descriptor", lanes);
    if (n == 0) return SLAM_OK;
    SLAM_REQUIRE(d_desc && d_node_desc && d_child && d_word_of_node && d_words && d_nodes, "slam_bow_transform: null device pointer");
    SLAM_HIP(hipSetDevice(ctx->device));
    const int node_depth = levels_up >= depth ? 0 : depth - levels_up;
    if (lanes == 0) lanes = n <= BOW_LANES16_UP_TO ? 16 : 1;
    if (lanes == 16)
        bow_transform16_kernel<<<bow_blocks(16 * n), BOW_THREADS, 0, ctx->stream>>>((const uint4*)d_desc, (int)n, (const uint4*)d_node_desc,
                                                                                     (const int2*)d_child, d_word_of_node, (int)n_nodes,
                                                                                     depth, node_depth, d_words, d_nodes);
    else
        bow_transform_kernel<<<bow_blocks(n), BOW_THREADS, 0, ctx->stream>>>((const uint4*)d_desc, (int)n, (const uint4*)d_node_desc,
                                                                              (const int2*)d_child, d_word_of_node, (int)n_nodes, depth,
                                                                              node_depth, d_words, d_nodes);
    return slam_launch_check("bow transform");
}

extern "C" int slam_bow_vectors(slam_ctx* ctx, const int32_t* d_words_in, const int64_t* d_offsets, int64_t B, int64_t n,
                                const double* d_idf, int64_t n_words, void* d_ws, uint64_t ws_bytes, int64_t* d_out_offsets,
                                int32_t* d_out_words, double* d_out_values, uint32_t* d_out_q) {
    SLAM_REQUIRE(ctx, "slam_bow_vectors: null ctx");
    SLAM_REQUIRE(B >= 0 && B <= (1 << 24) && n >= 0 && n <= (1ll << 30), "bad sizes (B=%lld, n=%lld)", (long long)B, (long long)n);
    SLAM_REQUIRE(n_words >= 1 && n_words <= (1 << 24), "n_words=%lld out of range [1, 2^24]", (long long)n_words);
    SLAM_REQUIRE(d_out_offsets, "slam_bow_vectors: null device pointer");
    SLAM_HIP(hipSetDevice(ctx->device));
    if (B == 0) {
        SLAM_HIP(hipMemsetAsync(d_out_offsets, 0, 8, ctx->stream));
        return SLAM_OK;
    }
    const uint64_t slots = (uint64_t)(n > 0 ? n : 1);
    const uint64_t o_val = 0, o_words = slam_align_up(slots * 8), o_q = o_words + slam_align_up(slots * 4), o_cnt = o_q + slam_align_up(slots * 4);
    const uint64_t need = o_cnt + slam_align_up((uint64_t)B * 4);
    SLAM_REQUIRE(d_ws && ws_bytes >= need, "slam_bow_vectors: workspace of %llu bytes, %llu needed", (unsigned long long)ws_bytes,
                 (unsigned long long)need);
    SLAM_REQUIRE(d_offsets && d_idf && (n == 0 || (d_words_in && d_out_words && d_out_values && d_out_q)),
                 "slam_bow_vectors: null device pointer");
    char* ws = (char*)d_ws;
    double* raw_values = (double*)(ws + o_val);
    int* raw_words = (int*)(ws + o_words);
    u32* raw_q = (u32*)(ws + o_q);
    int* count = (int*)(ws + o_cnt);
    bow_vectors_kernel<<<(unsigned)B, BOW_THREADS, 0, ctx->stream>>>(d_words_in, d_offsets, d_idf, (int)n_words, raw_words, raw_values, raw_q, count);
    if (int rc = slam_launch_check("bow vectors")) return rc;
    bow_offsets_kernel<<<1, BOW_THREADS, 0, ctx->stream>>>(count, B, d_out_offsets);
    if (int rc = slam_launch_check("bow vector offsets")) return rc;
    bow_compact_kernel<<<(unsigned)B, BOW_THREADS, 0, ctx->stream>>>(d_offsets, d_out_offsets, raw_words, raw_values, raw_q, d_out_words,
                                                                     d_out_values, d_out_q);
    return slam_launch_check("bow vector compaction");
}

extern "C" int slam_bow_vectors_workspace(int64_t B, int64_t n, uint64_t* h_bytes) {
    SLAM_REQUIRE(h_bytes && B >= 0 && n >= 0, "slam_bow_vectors_workspace: bad arguments");
    const uint64_t slots = (uint64_t)(n > 0 ? n : 1);
    *h_bytes = slam_align_up(slots * 8) + 2 * slam_align_up(slots * 4) + slam_align_up((uint64_t)(B > 0 ? B : 1) * 4);
    return SLAM_OK;
}

extern "C" int slam_bow_group_keys(slam_ctx* ctx, const int32_t* d_keys, int64_t n, int64_t n_keys, int32_t* d_key_off, int32_t* d_cursor,
                                   int32_t* d_perm) {
    SLAM_REQUIRE(ctx, "slam_bow_group_keys: null ctx");
    SLAM_REQUIRE(n >= 0 && n < (1ll << 31) && n_keys >= 1 && n_keys <= (1ll << 28), "bad sizes (n=%lld, n_keys=%lld)", (long long)n,
                 (long long)n_keys);
    SLAM_REQUIRE(d_key_off && d_cursor && (n == 0 || (d_keys && d_perm)), "slam_bow_group_keys: null device pointer");
    SLAM_HIP(hipSetDevice(ctx->device));
    SLAM_HIP(hipMemsetAsync(d_key_off, 0, (size_t)(n_keys + 1) * 4, ctx->stream));
    SLAM_HIP(hipMemsetAsync(d_cursor, 0, (size_t)n_keys * 4, ctx->stream));
    if (n > 0) {
        bow_hist_kernel<<<bow_blocks(n), BOW_THREADS, 0, ctx->stream>>>(d_keys, n, (int)n_keys, d_key_off);
        if (int rc = slam_launch_check("bow histogram")) return rc;
    }
    bow_scan_kernel<<<1, BOW_THREADS, 0, ctx->stream>>>(d_key_off, (int)n_keys);
    if (int rc = slam_launch_check("bow scan")) return rc;
    if (n > 0) {
        bow_scatter_kernel<<<bow_blocks(n), BOW_THREADS, 0, ctx->stream>>>(d_keys, n, (int)n_keys, d_key_off, d_cursor, d_perm);
        if (int rc = slam_launch_check("bow scatter")) return rc;
    }
    return SLAM_OK;
}

extern "C" int slam_bow_index_build(slam_ctx* ctx, const int32_t* d_words, const int32_t* d_entry, const uint32_t* d_q, int64_t T,
                                    int64_t n_words, int32_t* d_word_off, int32_t* d_cursor, int32_t* d_perm, void* d_postings) {
    SLAM_REQUIRE(ctx, "slam_bow_index_build: null ctx");
    SLAM_REQUIRE(n_words >= 1 && n_words <= (1 << 24), "n_words=%lld out of range [1, 2^24]", (long long)n_words);
    SLAM_REQUIRE(T == 0 || (d_entry && d_q && d_postings), "slam_bow_index_build: null device pointer");
    if (int rc = slam_bow_group_keys(ctx, d_words, T, n_words, d_word_off, d_cursor, d_perm)) return rc;
    if (T == 0) return SLAM_OK;
    bow_postings_kernel<<<bow_blocks(T), BOW_THREADS, 0, ctx->stream>>>(d_perm, T, d_entry, d_q, (uint2*)d_postings);
    return slam_launch_check("bow postings");
}

extern "C" int slam_bow_query(slam_ctx* ctx, const int64_t* d_q_offsets, const int32_t* d_q_words, const uint32_t* d_q_q, int64_t Q,
                              const int32_t* d_word_off, const void* d_postings, int64_t n_words, int64_t E, int64_t max_id,
                              int max_results, int32_t* d_ids, uint32_t* d_s_int, int32_t* d_common, uint32_t* d_dense_s,
                              int32_t* d_dense_common) {
    SLAM_REQUIRE(ctx, "slam_bow_query: null ctx");
    SLAM_REQUIRE(Q >= 0 && Q <= (1 << 24) && E >= 0 && E < (1ll << 31), "bad sizes (Q=%lld, E=%lld)", (long long)Q, (long long)E);
    SLAM_REQUIRE(n_words >= 1 && n_words <= (1 << 24), "n_words=%lld out of range [1, 2^24]", (long long)n_words);
    const bool dense = d_dense_s != nullptr;
    SLAM_REQUIRE(dense == (d_dense_common != nullptr), "slam_bow_query: the dense tables come as a pair");
    SLAM_REQUIRE(dense || (max_results >= 1 && max_results <= BOW_RESULTS_MAX && max_id >= 0), "max_results=%d out of range [1, %d], or max_id < 0",
                 max_results, BOW_RESULTS_MAX);
    SLAM_REQUIRE(!dense || (uint64_t)Q * (uint64_t)E < (1ull << 40), "slam_bow_query: dense tables of more than 2^40 entries");
    if (Q == 0 || (dense && E == 0)) return SLAM_OK;
    SLAM_REQUIRE(d_q_offsets && d_q_words && d_q_q && d_word_off && (E == 0 || d_postings), "slam_bow_query: null device pointer");
    SLAM_REQUIRE(dense || (d_ids && d_s_int && d_common), "slam_bow_query: null device pointer");
    SLAM_HIP(hipSetDevice(ctx->device));
    const int limit = (int)(dense ? E : (max_id < E ? max_id : E));
    bow_query_kernel<<<(unsigned)Q, BOW_Q_THREADS, 0, ctx->stream>>>(d_q_offsets, d_q_words, d_q_q, d_word_off, (const uint2*)d_postings,
                                                                     (int)n_words, (int)E, limit, dense ? 0 : max_results, d_ids, d_s_int,
                                                                     d_common, d_dense_s, d_dense_common);
    return slam_launch_check("bow query");
}

// ---- training: one depth of the tree per round of calls (slamhip/bow.py train_vocabulary drives them) ----
static int bow_train_args(const char* who, slam_ctx* ctx, int64_t n, int64_t F, int k) {
    SLAM_REQUIRE(ctx, "%s: null ctx", who);
    SLAM_REQUIRE(n >= 1 && n < (1ll << 31) && F >= 1 && F <= n, "%s: bad sizes (n=%lld, F=%lld)", who, (long long)n, (long long)F);
    SLAM_REQUIRE(k >= 2 && k <= BOW_K_MAX && (uint64_t)F * (uint64_t)k < (1ull << 31), "%s: k=%d out of range [2, %d], or F * k >= 2^31", who, k,
                 BOW_K_MAX);
    return SLAM_OK;
}

extern "C" int slam_bow_train_seed(slam_ctx* ctx, const void* d_desc, int64_t n, const int32_t* d_row_node, int64_t F, int k, void* d_cent,
                                   int32_t* d_cent_count, void* d_ws, uint64_t ws_bytes) {
    if (int rc = bow_train_args("slam_bow_train_seed", ctx, n, F, k)) return rc;
    const uint64_t o_best = 0, o_first = slam_align_up((uint64_t)F * 8), o_alive = o_first + slam_align_up((uint64_t)F * 4),
                   o_mind = o_alive + slam_align_up((uint64_t)F * 4), need = o_mind + slam_align_up((uint64_t)n * 4);
    SLAM_REQUIRE(d_desc && d_row_node && d_cent && d_cent_count && d_ws && ws_bytes >= need,
                 "slam_bow_train_seed: null device pointer, or a workspace of %llu bytes where %llu are needed", (unsigned long long)ws_bytes,
                 (unsigned long long)need);
    SLAM_HIP(hipSetDevice(ctx->device));
    char* ws = (char*)d_ws;
    u64* best = (u64*)(ws + o_best);
    u32* first = (u32*)(ws + o_first);
    int* alive = (int*)(ws + o_alive);
    u32* mind = (u32*)(ws + o_mind);
    const uint4* desc = (const uint4*)d_desc;
    uint4* cent = (uint4*)d_cent;
    SLAM_HIP(hipMemsetAsync(first, 0xFF, (size_t)F * 4, ctx->stream));
    SLAM_HIP(hipMemsetAsync(d_cent, 0, (size_t)F * k * 32, ctx->stream));
    bow_first_row_kernel<<<bow_blocks(n), BOW_THREADS, 0, ctx->stream>>>(d_row_node, (int)n, first);
    if (int rc = slam_launch_check("bow first row")) return rc;
    bow_seed_init_kernel<<<bow_blocks(F), BOW_THREADS, 0, ctx->stream>>>(desc, (int)n, first, (int)F, k, cent, d_cent_count, alive, best);
    if (int rc = slam_launch_check("bow seed init")) return rc;
    for (int j = 1; j < k; j++) {
        bow_seed_far_kernel<<<bow_blocks(n), BOW_THREADS, 0, ctx->stream>>>(desc, (int)n, d_row_node, cent, alive, k, j, mind, best);
        if (int rc = slam_launch_check("bow seed distances")) return rc;
        bow_seed_pick_kernel<<<bow_blocks(F), BOW_THREADS, 0, ctx->stream>>>(desc, (int)F, k, j, cent, d_cent_count, alive, best);
        if (int rc = slam_launch_check("bow seed pick")) return rc;
    }
    return SLAM_OK;
}

extern "C" int slam_bow_train_seed_workspace(int64_t n, int64_t F, uint64_t* h_bytes) {
    SLAM_REQUIRE(h_bytes && n >= 0 && F >= 0, "slam_bow_train_seed_workspace: bad arguments");
    *h_bytes = slam_align_up((uint64_t)F * 8) + 2 * slam_align_up((uint64_t)F * 4) + slam_align_up((uint64_t)n * 4);
    return SLAM_OK;
}

extern "C" int slam_bow_train_step(slam_ctx* ctx, const void* d_desc, int64_t n, const int32_t* d_row_node, int64_t F, int k, void* d_cent,
                                   const int32_t* d_cent_count, int32_t* d_assign, const int32_t* d_perm, int64_t n_live, uint32_t* d_bits,
                                   uint32_t* d_rows_of, uint32_t* d_changed, int update, int64_t* h_changed) {
    if (int rc = bow_train_args("slam_bow_train_step", ctx, n, F, k)) return rc;
    SLAM_REQUIRE(d_desc && d_row_node && d_cent && d_cent_count && d_assign && d_changed && h_changed, "slam_bow_train_step: null pointer");
    SLAM_REQUIRE(!update || (d_perm && d_bits && d_rows_of && n_live >= 0 && n_live <= n), "slam_bow_train_step: null pointer or bad n_live");
    SLAM_HIP(hipSetDevice(ctx->device));
    SLAM_HIP(hipMemsetAsync(d_changed, 0, 4, ctx->stream));
    bow_assign_kernel<<<bow_blocks(n), BOW_THREADS, 0, ctx->stream>>>((const uint4*)d_desc, (int)n, d_row_node, (const uint4*)d_cent, d_cent_count,
                                                                      k, d_assign, d_changed);
    if (int rc = slam_launch_check("bow assign")) return rc;
    uint32_t changed = 0;
    SLAM_HIP(hipMemcpyAsync(&changed, d_changed, 4, hipMemcpyDeviceToHost, ctx->stream));
    SLAM_HIP(hipStreamSynchronize(ctx->stream));
    *h_changed = changed;
    if (!update || changed == 0 || n_live == 0) return SLAM_OK;
    SLAM_HIP(hipMemsetAsync(d_bits, 0, (size_t)F * k * 256 * 4, ctx->stream));
    SLAM_HIP(hipMemsetAsync(d_rows_of, 0, (size_t)F * k * 4, ctx->stream));
    bow_majority_kernel<<<(unsigned)((n_live + BOW_MAJ_ROWS - 1) / BOW_MAJ_ROWS), BOW_THREADS, 0, ctx->stream>>>(
        (const u32*)d_desc, d_perm, (int)n_live, d_row_node, d_assign, k, d_bits, d_rows_of);
    if (int rc = slam_launch_check("bow majority")) return rc;
    bow_update_kernel<<<(unsigned)(F * k), BOW_THREADS, 0, ctx->stream>>>(d_bits, d_rows_of, (u32*)d_cent);
    return slam_launch_check("bow centre update");
}

extern "C" int slam_bow_train_descend(slam_ctx* ctx, int32_t* d_row_node, const int32_t* d_assign, int64_t n, int64_t F, int k,
                                      uint32_t* d_own, const int32_t* d_next_of) {
    if (int rc = bow_train_args("slam_bow_train_descend", ctx, n, F, k)) return rc;
    SLAM_REQUIRE(d_row_node && d_assign && (d_own != nullptr) != (d_next_of != nullptr),
                 "slam_bow_train_descend: null device pointer, or not exactly one of d_own and d_next_of");
    SLAM_HIP(hipSetDevice(ctx->device));
    if (d_own) {
        SLAM_HIP(hipMemsetAsync(d_own, 0, (size_t)F * k * 4, ctx->stream));
        bow_own_kernel<<<bow_blocks(n), BOW_THREADS, 0, ctx->stream>>>(d_row_node, d_assign, (int)n, k, d_own);
        return slam_launch_check("bow owners");
    }
    bow_relabel_kernel<<<bow_blocks(n), BOW_THREADS, 0, ctx->stream>>>(d_row_node, d_assign, (int)n, k, d_next_of);
    return slam_launch_check("bow relabel");
}
