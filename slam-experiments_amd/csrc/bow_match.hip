// bow_match.hip - ORBmatcher::SearchByBoW over the direct index: the correspondences of candidate image pairs,
// comparing only the features that bow_transform(..., levels_up) put into the same vocabulary node.  A sort-merge join:
//   group   one workgroup per image sorts its rows by (node as u32, row) in LDS and gathers the descriptors into that order,
//           so that a node's rows are one contiguous segment (DBoW2's FeatureVector; built once per image, reused by every call);
//   scan    one side-1 row per lane: two binary searches for its node's segment in the pair's sorted side-2 list, XOR/popcount
//           over the segment, the top-2 of the packed keys dist << 23 | row in registers - one lane owns a row, no atomics;
//           a proposed row then claims its side-2 row by one 32-bit atomic minimum of (d0 << 13 | side-1 row);
//   finish  one workgroup per pair: the winners of the claims, the 32-bin rotation histogram and its three maxima in LDS,
//           matches12 and the count.
// Every comparison is between integers (or doubles that hold integers <= 256), the atomics are integer minima and LDS integer
// adds, so the result is the same bits on every run and for every launch geometry.
#include "node_walk.h"

#define BM_ROWS_MAX MF_ROWS_MAX     // rows of one image: the row fits the 13-bit field of the claim key and the LDS sort
#define BM_PAIRS_MAX MF_PAIRS_MAX   // pairs of one call (the pair table: 48 bytes each in the context's workspace)
#define BM_GROUP_THREADS 1024
#define BM_SCAN_LANES 64            // side-1 rows of one scan workgroup: one wave, so a lone pair of 2000 rows still spreads over 32 CUs
#define BM_FIN_THREADS MF_FIN_THREADS
#define BM_BINS MF_BINS
#define BM_NO_SECOND 256            // ORB-SLAM's initial bestDist2: what a missing second neighbour counts as in the ratio test

typedef unsigned long long u64;
typedef mf_pair bm_pair;

struct bm_set {
    const uint4* desc;              // rows in grouped order
    const int* nodes;               // node ids in grouped order
    const int* order;               // the row (local to its image) at each grouped position
    const int* inverse;             // the grouped position of each row
    const uint8_t* bins;            // orientation bins in row order, or null
};

// ---------------------------------------------------------------------------------------------------------------- group
// 64-bit keys (node as u32) << 32 | row: unsigned order puts the negative (masked) ids behind every real one, the row breaks
// ties, and the padding of the bitonic network (~0) stays behind both.  8192 keys are 64 KiB of the CU's 160 KiB.
__global__ __launch_bounds__(BM_GROUP_THREADS) void bm_group_kernel(const uint4* __restrict__ desc, const int* __restrict__ nodes,
                                                                   const int64_t* __restrict__ offsets, uint4* __restrict__ desc_sorted,
                                                                   int* __restrict__ nodes_sorted, int* __restrict__ order,
                                                                   int* __restrict__ inverse) {
    __shared__ u64 s_key[BM_ROWS_MAX];
    const int tid = threadIdx.x;
    const int64_t base = offsets[blockIdx.x];
    const int n = (int)min((int64_t)BM_ROWS_MAX, offsets[blockIdx.x + 1] - base);
    if (n <= 0) return;
    int P = 2;
    while (P < n) P <<= 1;
    for (int i = tid; i < P; i += BM_GROUP_THREADS) s_key[i] = i < n ? ((u64)(u32)nodes[base + i] << 32) | (u32)i : ~0ull;
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (P >> 1); t += BM_GROUP_THREADS) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const u64 x = s_key[lo], y = s_key[hi];
                if ((x > y) == ((lo & size) == 0)) {
                    s_key[lo] = y;
                    s_key[hi] = x;
                }
            }
            __syncthreads();
        }
    for (int i = tid; i < n; i += BM_GROUP_THREADS) {
        const u64 key = s_key[i];
        const int row = (int)(u32)key;
        order[base + i] = row;
        nodes_sorted[base + i] = (int)(u32)(key >> 32);
        inverse[base + row] = i;
    }
    for (int j = tid; j < 2 * n; j += BM_GROUP_THREADS) {
        const int row = (int)(u32)s_key[j >> 1];
        desc_sorted[2 * base + j] = desc[2 * (base + row) + (j & 1)];
    }
}

// ----------------------------------------------------------------------------------------------------------------- scan
// the selection of DESIGN.md 4k (b) on one row's top-2: the arithmetic of bf_select / filter_keep_kernel
__device__ __forceinline__ bool bm_proposed(int i0, int d0, int i1, int d1, int th_low, double ratio) {
    return i0 >= 0 && d0 <= th_low && (double)d0 < ratio * (double)(i1 >= 0 ? d1 : BM_NO_SECOND);
}

// One lane per side-1 row.  scan_order 0: lane t takes the row at grouped position t, so the lanes of a wave hold a few
// nodes and read the same side-2 segments (one address per node: a broadcast); 1: lane t takes row t, whatever its node
// (the A/B of profiles/bow_match_time.log).  The tables are written in row order either way.
template <bool SELECT>
__global__ __launch_bounds__(BM_SCAN_LANES) void bm_scan_kernel(const bm_set s1, const bm_set s2, const bm_pair* __restrict__ pairs, int P,
                                                               int scan_order, int th_low, double ratio, int2* __restrict__ idx,
                                                               int2* __restrict__ dist, u32* __restrict__ owner) {
    const int bx = (int)blockIdx.x;
    const bm_pair pr = pairs[mf_pair_of(pairs, P, bx)];
    const int t = (bx - pr.blk0) * BM_SCAN_LANES + (int)threadIdx.x;
    if (t >= pr.n1) return;
    const int pos = scan_order == 0 ? t : s1.inverse[pr.base1 + t];
    const int node = s1.nodes[pr.base1 + pos], row = scan_order == 0 ? s1.order[pr.base1 + pos] : t;
    mf_top2 top;
    if (node >= 0 && pr.n2 > 0) {
        const int* nodes2 = s2.nodes + pr.base2;
        const int2 seg = make_int2(mf_bound<false>(nodes2, pr.n2, (u32)node), mf_bound<true>(nodes2, pr.n2, (u32)node));
        u32 q[8];
        bf_load_query(s1.desc + 2 * pr.base1, pos, q);
        nw_walk(s2.order + pr.base2, s2.desc + 2 * pr.base2, seg, q,
                [&](u32 d, int r, bool inside) { top.take(inside ? (d << SLAM_KEY_IDX_BITS) | (u32)r : SLAM_KEY_NONE); });
    }
    const int2 ix = top.idx(), ds = top.dist();
    idx[pr.out1 + row] = ix;
    dist[pr.out1 + row] = ds;
    if (SELECT && bm_proposed(ix.x, ds.x, ix.y, ds.y, th_low, ratio)) atomicMin(&owner[pr.own2 + ix.x], mf_claim_key(ds.x, row));
}

// --------------------------------------------------------------------------------------------------------------- finish
// One workgroup per pair: the claim check, the rotation histogram, matches12 and the count of match_finish.h under 4k (b)
struct bm_select {
    int th_low;
    double ratio;
    __device__ __forceinline__ bool proposed(const mf_pair&, int2 ix, int2 ds) const { return bm_proposed(ix.x, ds.x, ix.y, ds.y, th_low, ratio); }
};

__global__ __launch_bounds__(BM_FIN_THREADS) void bm_finish_kernel(const bm_set s1, const bm_set s2, const bm_pair* __restrict__ pairs,
                                                                  int th_low, double ratio, const int2* __restrict__ idx,
                                                                  const int2* __restrict__ dist, const u32* __restrict__ owner,
                                                                  int* __restrict__ matches12, int* __restrict__ count) {
    const bm_pair pr = pairs[blockIdx.x];
    mf_finish(bm_select{th_low, ratio}, pr, s1.bins, s2.bins, idx, dist, owner, matches12, count + blockIdx.x);
}

// =============================================================== entry points ================================================
extern "C" int slam_bow_match_limits(int32_t* h_limits) {
    SLAM_REQUIRE(h_limits, "slam_bow_match_limits: null pointer");
    h_limits[0] = BM_ROWS_MAX;
    h_limits[1] = BM_PAIRS_MAX;
    h_limits[2] = BM_GROUP_THREADS;
    h_limits[3] = BM_SCAN_LANES;
    h_limits[4] = BM_BINS;
    h_limits[5] = BM_NO_SECOND;
    return SLAM_OK;
}

extern "C" int slam_bow_match_plan_describe(int64_t B, int64_t n, int64_t* h_plan) {
    SLAM_REQUIRE(h_plan, "slam_bow_match_plan_describe: null h_plan");
    SLAM_REQUIRE(B >= 0 && B <= BM_PAIRS_MAX, "B=%lld out of range [0, %d]", (long long)B, BM_PAIRS_MAX);
    SLAM_REQUIRE(n >= 0 && n <= BM_ROWS_MAX, "n=%lld out of range [0, %d] rows per image", (long long)n, BM_ROWS_MAX);
    int64_t P2 = 2;
    while (P2 < n) P2 <<= 1;
    const int64_t per = (n + BM_SCAN_LANES - 1) / BM_SCAN_LANES;
    const mf_plan p = mf_layout(0, B, sizeof(bm_pair), B * n, B * n, true);
    const int64_t v[8] = {P2, (int64_t)(BM_ROWS_MAX * sizeof(u64)), B, B * per, B, (int64_t)p.bytes,
                          (int64_t)(BM_BINS * 4 + 8), (int64_t)slam_align_up((uint64_t)(B + 1) * 8)};
    memcpy(h_plan, v, sizeof(v));
    return SLAM_OK;
}

extern "C" int slam_bow_match_group(slam_ctx* ctx, const void* d_desc, const int32_t* d_nodes, const int64_t* h_offsets, int64_t B,
                                    void* d_desc_sorted, int32_t* d_nodes_sorted, int32_t* d_order, int32_t* d_inverse) {
    SLAM_REQUIRE(ctx, "slam_bow_match_group: null ctx");
    if (int rc = mf_check_offsets(h_offsets, B, "slam_bow_match_group", "image")) return rc;
    const int64_t n = h_offsets[B];
    if (n == 0) return SLAM_OK;
    SLAM_REQUIRE(d_desc && d_nodes && d_desc_sorted && d_nodes_sorted && d_order && d_inverse, "slam_bow_match_group: null device pointer");
    SLAM_REQUIRE(((uintptr_t)d_desc & 15) == 0 && ((uintptr_t)d_desc_sorted & 15) == 0, "descriptor pointers must be 16-byte aligned");
    std::lock_guard<std::mutex> lk(ctx->call_mu);       // the offsets travel through the context's workspace
    SLAM_HIP(hipSetDevice(ctx->device));
    void* ws = nullptr;
    if (int rc = slam_workspace(ctx, slam_align_up((uint64_t)(B + 1) * 8), &ws)) return rc;
    SLAM_HIP(hipMemcpyAsync(ws, h_offsets, (size_t)(B + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    bm_group_kernel<<<(unsigned)B, BM_GROUP_THREADS, 0, ctx->stream>>>((const uint4*)d_desc, d_nodes, (const int64_t*)ws, (uint4*)d_desc_sorted,
                                                                       d_nodes_sorted, d_order, d_inverse);
    return slam_launch_check("bow match group");
}

static int bm_check_groups(const slam_bow_groups* g, const char* who, bm_set* out) {
    SLAM_REQUIRE(g, "%s: null group set", who);
    if (int rc = mf_check_groups(g, who)) return rc;
    SLAM_REQUIRE(((uintptr_t)g->d_desc & 15) == 0, "%s: descriptor pointers must be 16-byte aligned", who);
    out->desc = (const uint4*)g->d_desc;
    out->nodes = g->d_nodes;
    out->order = g->d_order;
    out->inverse = g->d_inverse;
    out->bins = g->d_bins;
    return SLAM_OK;
}

// the common body of the node top-2 and the full search; `select`: claims, winners, rotation check, matches12 and counts
static int bm_run(slam_ctx* ctx, const slam_bow_groups* g1, const slam_bow_groups* g2, const int32_t* h_pairs, int64_t P, int scan_order,
                  bool select, int th_low, double ratio, int32_t* d_idx, int32_t* d_dist, int32_t* d_matches12, int32_t* d_count,
                  const char* who) {
    SLAM_REQUIRE(ctx, "%s: null ctx", who);
    bm_set s1, s2;
    if (int rc = bm_check_groups(g1, who, &s1)) return rc;
    if (int rc = bm_check_groups(g2, who, &s2)) return rc;
    SLAM_REQUIRE(P >= 0 && P <= BM_PAIRS_MAX, "%s: P=%lld pairs out of range [0, %d]", who, (long long)P, BM_PAIRS_MAX);
    SLAM_REQUIRE(scan_order == 0 || scan_order == 1, "%s: scan_order=%d not in {0, 1}", who, scan_order);
    SLAM_REQUIRE(!select || ratio == ratio, "%s: ratio is not a number", who);
    SLAM_REQUIRE((d_idx != nullptr) == (d_dist != nullptr), "%s: the top-2 tables come as a pair", who);
    SLAM_REQUIRE(select || d_idx, "%s: null result pointer", who);
    SLAM_REQUIRE((g1->d_bins != nullptr) == (g2->d_bins != nullptr), "%s: the orientation bins come for both sides or for neither", who);
    if (P == 0) return SLAM_OK;
    SLAM_REQUIRE(h_pairs, "%s: null pairs", who);
    std::vector<bm_pair> table((size_t)P);
    mf_totals t{0, 0, 0};
    for (int64_t p = 0; p < P; p++)
        if (int rc = mf_pair_next(table[(size_t)p], g1->h_offsets, g1->B, h_pairs[2 * p], g2->h_offsets, g2->B, h_pairs[2 * p + 1], BM_SCAN_LANES,
                                  t, who, p))
            return rc;
    const int64_t out1 = t.out1, own2 = select ? t.own2 : 0, blocks = t.blocks;     // (the top-2 alone claims nothing)
    SLAM_REQUIRE(!select || (d_count && (out1 == 0 || d_matches12)), "%s: null result pointer", who);
    SLAM_REQUIRE(select || out1 == 0 || d_idx, "%s: null result pointer", who);
    if (!select && out1 == 0) return SLAM_OK;
    std::lock_guard<std::mutex> lk(ctx->call_mu);       // the pair table, the claim words and the tables nobody asked for: the workspace
    SLAM_HIP(hipSetDevice(ctx->device));
    const mf_plan pl = mf_layout(0, P, sizeof(bm_pair), out1, own2, d_idx == nullptr);
    void* ws = nullptr;
    if (int rc = slam_workspace(ctx, pl.bytes, &ws)) return rc;
    char* w = (char*)ws;
    if (int rc = mf_stage(ctx, pl, w, table.data(), own2)) return rc;
    const bm_pair* d_pairs = (const bm_pair*)(w + pl.o_pairs);
    int2* idx = d_idx ? (int2*)d_idx : (int2*)(w + pl.o_idx);
    int2* dist = d_dist ? (int2*)d_dist : (int2*)(w + pl.o_dist);
    u32* owner = (u32*)(w + pl.o_owner);
    if (blocks > 0) {
        if (int rc = slam_prof_begin(ctx)) return rc;
        if (select)
            bm_scan_kernel<true><<<(unsigned)blocks, BM_SCAN_LANES, 0, ctx->stream>>>(s1, s2, d_pairs, (int)P, scan_order, th_low, ratio, idx, dist, owner);
        else
            bm_scan_kernel<false><<<(unsigned)blocks, BM_SCAN_LANES, 0, ctx->stream>>>(s1, s2, d_pairs, (int)P, scan_order, th_low, ratio, idx, dist, owner);
        if (int rc = slam_prof_end(ctx)) return rc;
        if (int rc = slam_launch_check("bow match scan")) return rc;
    }
    if (!select) return SLAM_OK;
    bm_finish_kernel<<<(unsigned)P, BM_FIN_THREADS, 0, ctx->stream>>>(s1, s2, d_pairs, th_low, ratio, idx, dist, owner, d_matches12, d_count);
    return slam_launch_check("bow match finish");
}

extern "C" int slam_bow_match_top2(slam_ctx* ctx, const slam_bow_groups* g1, const slam_bow_groups* g2, const int32_t* h_pairs, int64_t P,
                                   int scan_order, int32_t* d_idx, int32_t* d_dist) {
    return bm_run(ctx, g1, g2, h_pairs, P, scan_order, false, 0, 0.0, d_idx, d_dist, nullptr, nullptr, "slam_bow_match_top2");
}

extern "C" int slam_bow_match_search(slam_ctx* ctx, const slam_bow_groups* g1, const slam_bow_groups* g2, const int32_t* h_pairs, int64_t P,
                                     int th_low, double ratio, int scan_order, int32_t* d_matches12, int32_t* d_count, int32_t* d_idx,
                                     int32_t* d_dist) {
    return bm_run(ctx, g1, g2, h_pairs, P, scan_order, true, th_low, ratio, d_idx, d_dist, d_matches12, d_count, "slam_bow_match_search");
}
