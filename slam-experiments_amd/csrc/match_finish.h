// match_finish.h - what the four pair-table searches share around their scans (bow_match.hip: SearchByBoW, proj_match.hip:
// SearchByProjection, tri_match.hip: SearchForTriangulation, fuse.hip: Fuse).  Device: the pair record, the pair of a workgroup,
// the register top-2 of a lane, the claim key of the one-to-one step, and the finish step - the winners of the claims, the 32-bin rotation histogram with its three maxima,
// matches12 and the count; the searches differ in which rows their selection proposes:
// SEL::proposed(pr, top-2 rows, top-2 distances).  Host (at the end): the offsets and group-set checks, the head of a pair
// record, the workspace layout and the staging of the host block ("The host side").
#pragma once
#include "bf_common.h"

#define MF_PAIRS_MAX 4096           // pairs of one call
#define MF_ROWS_MAX 8192            // rows of one image: the row fits the 13-bit field of the claim key
#define MF_ROW_BITS 13
#define MF_BINS 32
#define MF_FIN_THREADS 256

struct mf_pair {
    int64_t base1, base2;           // first row of the two images in their sets
    int64_t out1, own2;             // where the pair's side-1 results and side-2 claim words start
    int n1, n2, blk0, pad;          // rows, and the pair's first scan workgroup
};

static_assert(sizeof(mf_pair) == 48, "the pair table is laid out by the host");

// the head of a pair record: the record itself, or the mf_pair m it starts with
__device__ __forceinline__ const mf_pair& mf_head(const mf_pair& r) { return r; }
template <class REC>
__device__ __forceinline__ const mf_pair& mf_head(const REC& r) { return r.m; }

// the pair of workgroup bx of a kernel launched over the table of P pairs: the last one whose first workgroup is not behind it
template <class REC>
__device__ __forceinline__ int mf_pair_of(const REC* __restrict__ pairs, int P, int bx) {
    int lo = 0, hi = P - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (mf_head(pairs[mid]).blk0 <= bx) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// the two smallest of the keys dist << 23 | row a lane has taken, in registers, and what they say: rows and distances
struct mf_top2 {
    u32 b1 = SLAM_KEY_NONE, b2 = SLAM_KEY_NONE;
    __device__ __forceinline__ void take(u32 key) {
        b2 = min(b2, max(b1, key));
        b1 = min(b1, key);
    }
    __device__ __forceinline__ int2 idx() const { return make_int2(bf_key_idx(b1, 0), bf_key_idx(b2, 0)); }
    __device__ __forceinline__ int2 dist() const { return make_int2(bf_key_dist(b1), bf_key_dist(b2)); }
};

// first position in a[0 .. n) whose id, as u32, is >= v (STRICT: > v): the ends of an id's segment in a grouped image
template <bool STRICT>
__device__ __forceinline__ int mf_bound(const int* __restrict__ a, int n, u32 v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const u32 x = (u32)a[mid];
        if (STRICT ? x <= v : x < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the word a proposed side-1 row puts on its side-2 row by atomic minimum: the smallest (d0, row) keeps it
__device__ __forceinline__ u32 mf_claim_key(int d0, int row) { return ((u32)d0 << MF_ROW_BITS) | (u32)row; }

// A proposed row survives iff the claim word of its side-2 row holds its own key (the smallest (d0, row) among the rows that
// named it; the others are dropped, they do not fall back to their second neighbour).
template <class SEL>
__device__ __forceinline__ int mf_survivor(const SEL& sel, const mf_pair& pr, int i, const int2* idx, const int2* dist, const u32* owner) {
    const int2 ix = idx[pr.out1 + i], ds = dist[pr.out1 + i];
    if (!sel.proposed(pr, ix, ds)) return -1;
    return owner[pr.own2 + ix.x] == mf_claim_key(ds.x, i) ? ix.x : -1;
}

// One workgroup of MF_FIN_THREADS threads per pair; bins1 / bins2: the orientation bins of the two sets in row order, or null.
template <class SEL>
__device__ __forceinline__ void mf_finish(const SEL& sel, const mf_pair& pr, const uint8_t* bins1, const uint8_t* bins2,
                                          const int2* __restrict__ idx, const int2* __restrict__ dist, const u32* __restrict__ owner,
                                          int* __restrict__ matches12, int* __restrict__ count) {
    __shared__ int s_hist[MF_BINS];
    __shared__ u32 s_keep;
    __shared__ int s_count;
    const int tid = threadIdx.x;
    const bool rot = bins1 && bins2;
    if (tid < MF_BINS) s_hist[tid] = 0;
    if (tid == 0) {
        s_keep = 0xFFFFFFFFu;
        s_count = 0;
    }
    __syncthreads();
    if (rot) {
        for (int i = tid; i < pr.n1; i += MF_FIN_THREADS) {
            const int j = mf_survivor(sel, pr, i, idx, dist, owner);
            if (j >= 0) atomicAdd(&s_hist[((int)bins1[pr.base1 + i] - (int)bins2[pr.base2 + j]) & (MF_BINS - 1)], 1);
        }
        __syncthreads();
        if (tid == 0) {
            // the first three bins by (count descending, bin ascending); ComputeThreeMaxima's 0.1 rule in integers
            int b[3] = {-1, -1, -1};
            for (int s = 0; s < 3; s++)
                for (int v = 0; v < MF_BINS; v++) {
                    bool taken = false;
                    for (int t = 0; t < s; t++) taken |= v == b[t];
                    if (!taken && (b[s] < 0 || s_hist[v] > s_hist[b[s]])) b[s] = v;      // (strict: a tie stays with the lower bin)
                }
            const int c1 = s_hist[b[0]];
            u32 keep = 1u << b[0];
            for (int s = 1; s < 3; s++)
                if (s_hist[b[s]] > 0 && 10 * s_hist[b[s]] >= c1) keep |= 1u << b[s];
            s_keep = keep;
        }
        __syncthreads();
    }
    const u32 keep = s_keep;
    int mine = 0;
    for (int i = tid; i < pr.n1; i += MF_FIN_THREADS) {
        int j = mf_survivor(sel, pr, i, idx, dist, owner);
        if (rot && j >= 0 && !((keep >> (((int)bins1[pr.base1 + i] - (int)bins2[pr.base2 + j]) & (MF_BINS - 1))) & 1u)) j = -1;
        matches12[pr.out1 + i] = j;
        mine += j >= 0 ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);
    if ((tid & 63) == 0 && mine) atomicAdd(&s_count, mine);
    __syncthreads();
    if (tid == 0) *count = s_count;
}

// ======================================================================== host ===============================================
// What the entry points share in front of their launches.  Nothing here knows which search calls it: the sizes, the noun of
// an error text and a missing side 2 are arguments.

// the running out1 / own2 of a call stay below 2^31
static_assert((int64_t)MF_PAIRS_MAX * MF_ROWS_MAX < (1ll << 31), "the rows over the pairs of one call fit 31 bits");

// the offsets of B sets of at most MF_ROWS_MAX rows (what: the noun of the texts, "image", "frame", "point set")
static int mf_check_offsets(const int64_t* off, int64_t B, const char* who, const char* what) {
    SLAM_REQUIRE(B >= 0 && B <= (1 << 24), "%s: %lld %ss out of range [0, 2^24]", who, (long long)B, what);
    SLAM_REQUIRE(off && off[0] == 0, "%s: null %s offsets, or offsets that do not start at 0", who, what);
    for (int64_t b = 0; b < B; b++) {
        const int64_t n = off[b + 1] - off[b];
        SLAM_REQUIRE(n >= 0 && n <= MF_ROWS_MAX, "%s: %s %lld has %lld rows (0 .. %d)", who, what, (long long)b, (long long)n, MF_ROWS_MAX);
    }
    SLAM_REQUIRE(off[B] < (1ll << 31), "%s: more than 2^31 rows", who);
    return SLAM_OK;
}

// a non-null group set: its offsets, and its device arrays when it has rows
static int mf_check_groups(const slam_bow_groups* g, const char* who) {
    if (int rc = mf_check_offsets(g->h_offsets, g->B, who, "image")) return rc;
    SLAM_REQUIRE(g->h_offsets[g->B] == 0 || (g->d_desc && g->d_nodes && g->d_order && g->d_inverse), "%s: null device pointer in a group set", who);
    return SLAM_OK;
}

struct mf_totals {
    int64_t out1, own2, blocks;     // side-1 rows, side-2 rows and scan workgroups of the pairs so far
};

// The head of pair p = (a, b): set a of side 1, set b of side 2 (off2 null: no side 2, base2 = n2 = 0); block_rows: the side-1
// rows one workgroup of the kernel that reads the table takes.  The caller writes the rest of its record.
static int mf_pair_next(mf_pair& e, const int64_t* off1, int64_t B1, int64_t a, const int64_t* off2, int64_t B2, int64_t b, int block_rows,
                        mf_totals& t, const char* who, int64_t p) {
    SLAM_REQUIRE(a >= 0 && a < B1 && (!off2 || (b >= 0 && b < B2)), "%s: pair %lld = (%lld, %lld) lies outside the sets (%lld, %lld)", who,
                 (long long)p, (long long)a, (long long)b, (long long)B1, (long long)B2);
    e.base1 = off1[a];
    e.n1 = (int)(off1[a + 1] - e.base1);
    e.base2 = off2 ? off2[b] : 0;
    e.n2 = off2 ? (int)(off2[b + 1] - e.base2) : 0;
    e.out1 = t.out1;
    e.own2 = t.own2;
    e.blk0 = (int)t.blocks;
    e.pad = 0;
    t.out1 += e.n1;
    t.own2 += e.n2;
    t.blocks += (e.n1 + block_rows - 1) / block_rows;
    return SLAM_OK;
}

// The workspace of one call: the host block - head_bytes of parameters (0: none) and the table of P pair records, one copy -,
// the top-2 tables of n1_total rows when the caller keeps none, the claim words of n2_total side-2 rows.
struct mf_plan {
    uint64_t o_pairs, o_idx, o_dist, o_owner, bytes, block_bytes;
};

static mf_plan mf_layout(size_t head_bytes, int64_t P, size_t pair_bytes, int64_t n1_total, int64_t n2_total, bool own_tables) {
    mf_plan p;
    p.o_pairs = slam_align_up(head_bytes);
    p.block_bytes = p.o_pairs + (uint64_t)P * pair_bytes;
    p.o_idx = p.o_pairs + slam_align_up((uint64_t)(P > 0 ? P : 1) * pair_bytes);
    p.o_dist = p.o_idx + (own_tables ? slam_align_up((uint64_t)n1_total * 8) : 0);
    p.o_owner = p.o_dist + (own_tables ? slam_align_up((uint64_t)n1_total * 8) : 0);
    p.bytes = p.o_owner + slam_align_up((uint64_t)n2_total * 4);
    return p;
}

// Under the caller's call lock, into the workspace w of pl.bytes the caller has asked for (the call stays in the entry point:
// tests/ctx_poison_cases.py lists every site): the one copy of the host block, and the claim words of own2 side-2 rows set to
// "nobody" (0: no memset).
static int mf_stage(slam_ctx* ctx, const mf_plan& pl, char* w, const void* block, int64_t own2) {
    SLAM_HIP(hipMemcpyAsync(w, block, (size_t)pl.block_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (own2 > 0) SLAM_HIP(hipMemsetAsync(w + pl.o_owner, 0xFF, (size_t)own2 * 4, ctx->stream));
    return SLAM_OK;
}
