// geometry_host.h — the one copy of what the extern "C" entry points of the four batched RANSAC estimators (two_view.hip, pnp.hip,
// homography.hip, sim3.hip) share in front of their launches: the argument checks with their texts, the vote block of a RANSAC
// call in the context's workspace, and the launch shapes.  Each entry point keeps its own checks, its slam_workspace call (the
// call lock is the entry point's) and its launch statements.
//
// For hipcc alone: the four files include it inside their #ifndef ..._HOST_ONLY sections, where internal.h is visible; the host
// twins of the test suite never see it.  The checks are macros because SLAM_REQUIRE returns from the function it stands in, and
// they name that function (__func__ of an extern "C" function is its plain name) as the texts always have; each is several
// statements, for the top level of an entry point only.
#pragma once
#include "internal.h"
#include "geometry_common.h"

// the context and the sizes of a RANSAC call: B candidates (blockIdx.y), M correspondences, H hypotheses per candidate
#define GEO_RANSAC_SIZES(ctx, B, M, H)                                                                                           \
    SLAM_REQUIRE(ctx, "%s: null ctx", __func__);                                                                                 \
    SLAM_REQUIRE(B >= 0 && B <= 65535 && M >= 0 && M <= (1 << 28), "bad sizes (B=%lld, M=%lld; B <= 65535)", (long long)(B),     \
                 (long long)(M));                                                                                                \
    SLAM_REQUIRE(H >= 1 && H <= GEO_H_MAX, "H=%d out of range [1, 2^20]", H)
// of a call with one block per candidate
#define GEO_CANDIDATE_SIZES(ctx, B, B_max, M)                                                                                    \
    SLAM_REQUIRE(ctx, "%s: null ctx", __func__);                                                                                 \
    SLAM_REQUIRE(B >= 0 && B <= (B_max) && M >= 0 && M <= (1 << 28), "bad sizes (B=%lld, M=%lld)", (long long)(B), (long long)(M))
// of a minimal-solver call on S samples
#define GEO_SAMPLE_SIZES(ctx, S)                                                                                                 \
    SLAM_REQUIRE(ctx, "%s: null ctx", __func__);                                                                                 \
    SLAM_REQUIRE(S >= 0 && S <= (1 << 24), "S=%lld out of range [0, 2^24]", (long long)(S))
// a call of n == 0 items is done and reads no pointer; any other needs `pointers`
#define GEO_POINTERS(n, pointers)                                                                                                \
    if ((n) == 0) return SLAM_OK;                                                                                                \
    SLAM_REQUIRE(pointers, "%s: null device pointer", __func__)

// The vote block of a RANSAC call, behind `front_bytes` of the caller's own (the two-view normalised points): one key (8 bytes)
// and one model count (4 bytes) per candidate, the counts directly behind the keys.
static inline uint64_t geo_vote_bytes(uint64_t front_bytes, int64_t B) { return front_bytes + (uint64_t)B * 8 + (uint64_t)B * 4; }
// Hands back the keys and the counts of the block at `ws` (geo_vote_bytes of workspace, the call lock held), cleared unless a
// kernel of the caller's clears them (`clear` false), and clears the M bytes of the call's mask.
static inline int geo_vote_block(slam_ctx* ctx, void* ws, uint64_t front_bytes, int64_t B, bool clear, int64_t M, uint8_t* d_inlier,
                                 unsigned long long** keys, int** models) {
    *keys = (unsigned long long*)((char*)ws + front_bytes);
    *models = (int*)(*keys + B);
    if (clear) SLAM_HIP(hipMemsetAsync(*keys, 0, (size_t)geo_vote_bytes(0, B), ctx->stream));
    if (M > 0) SLAM_HIP(hipMemsetAsync(d_inlier, 0, (size_t)M, ctx->stream));
    return SLAM_OK;
}

// launch shapes: one thread per item, and `threads` hypotheses per block of every candidate
static inline unsigned geo_blocks(int64_t n, int threads) { return (unsigned)((n + threads - 1) / threads); }
static inline dim3 geo_vote_grid(int H, int threads, int64_t B) { return dim3(geo_blocks(H, threads), (unsigned)B); }
