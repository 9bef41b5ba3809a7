// match_finish.h - what the pair searches share behind their scans (bow_match.hip: SearchByBoW, proj_match.hip:
// SearchByProjection): the pair record, the claim key of the one-to-one step, and the finish step - the winners of the claims,
// the 32-bin rotation histogram with its three maxima, matches12 and the count.  The searches differ
// in which rows their selection proposes: SEL::proposed(pr, top-2 rows, top-2 distances).
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
