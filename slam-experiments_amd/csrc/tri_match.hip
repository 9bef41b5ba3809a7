// tri_match.hip - ORBmatcher::SearchForTriangulation and the per-match half of LocalMapping::CreateNewMapPoints:
// the features of keyframe pairs that have no map point yet, matched inside one vocabulary node under the epipolar constraint of
// the two known poses, and every match triangulated and checked.
//   scan         bow_match.hip's mapping - one side-1 row per lane, its node's segment of the pair's grouped side-2 list by two
//                binary searches, XOR/popcount four rows ahead - with the gates of tri_point.h in front of the top-2 update: a
//                row whose key could enter the top-2 fetches its pixel and level through order2 and is kept only off the
//                epipole and on the epipolar line; then the claim of the first neighbour by one atomic minimum;
//   finish       the claim check and rotation histogram of match_finish.h; a row is proposed iff it has a first neighbour;
//   triangulate  the rows with a match packed to the front of a 256-row workgroup, one lane each: tp_triangulate, the point's
//                position, normal, range and status.
// The gates are f64 with contraction off; everything else is a comparison of integers, an integer minimum or an integer add:
// the same bits on every run and for every launch geometry.
#include "match_finish.h"
#include "tri_point.h"

#define TM_ROWS_MAX MF_ROWS_MAX
#define TM_PAIRS_MAX MF_PAIRS_MAX
#define TM_SCAN_LANES 64            // side-1 rows of one scan workgroup: one wave
#define TM_TRI_ROWS 256             // side-1 rows of one triangulation workgroup

struct tm_pair {
    mf_pair m;
    double F[9], ex, ey;            // F12 row-major; the epipole of camera 1 in image 2 (a NaN: that gate is off)
};

struct tt_pair {
    mf_pair m;
    double T1[12], T2[12], O1[3], O2[3];
};

static_assert(sizeof(tm_pair) == 136 && sizeof(tt_pair) == 288, "the pair tables are laid out by the host");

struct tm_set {
    const uint4* desc;              // rows in grouped order
    const int* nodes;               // node ids in grouped order
    const int* order;               // the row (local to its image) at each grouped position
    const int* inverse;             // the grouped position of each row
    const uint8_t* bins;            // orientation bins in row order, or null
    const float2* xy;               // level-0 pixels in row order
    const int* level;               // pyramid levels in row order
    const uint8_t* taken;           // non-zero: the row has a map point already; row order, or null
};

struct tm_views {
    const float2* xy;
    const int* level;
};

// ----------------------------------------------------------------------------------------------------------------- scan
// (The segment walk below is the second copy of nw_walk of node_walk.h, kept because the kernel built on the template missed
// two lines of its timing rule; node_walk.h and DESIGN.md 7, item 7, say which.)
__global__ __launch_bounds__(TM_SCAN_LANES) void tm_scan_kernel(const tm_set s1, const tm_set s2, const tm_pair* __restrict__ pairs, int P,
                                                               const tp_params* __restrict__ prm, int scan_order, int2* __restrict__ idx,
                                                               int2* __restrict__ dist, u32* __restrict__ owner) {
    const int bx = (int)blockIdx.x;
    int lo = 0, hi = P - 1;
    while (lo < hi) {                                   // the last pair whose first workgroup is not behind this one
        const int mid = (lo + hi + 1) >> 1;
        if (pairs[mid].m.blk0 <= bx) lo = mid;
        else hi = mid - 1;
    }
    const tm_pair* pp = pairs + lo;
    const mf_pair pr = pp->m;
    const int t = (bx - pr.blk0) * TM_SCAN_LANES + (int)threadIdx.x;
    if (t >= pr.n1) return;
    const int pos = scan_order == 0 ? t : s1.inverse[pr.base1 + t];
    const int node = s1.nodes[pr.base1 + pos], row = scan_order == 0 ? s1.order[pr.base1 + pos] : t;
    u32 b1 = SLAM_KEY_NONE, b2 = SLAM_KEY_NONE;
    if (node >= 0 && pr.n2 > 0 && !(s1.taken && s1.taken[pr.base1 + row])) {
        const int* nodes2 = s2.nodes + pr.base2;
        const int* order2 = s2.order + pr.base2;
        const uint4* rows2 = s2.desc + 2 * pr.base2;
        const float2* xy2 = s2.xy + pr.base2;
        const int* level2 = s2.level + pr.base2;
        const uint8_t* taken2 = s2.taken ? s2.taken + pr.base2 : nullptr;
        const int j0 = mf_bound<false>(nodes2, pr.n2, (u32)node), j1 = mf_bound<true>(nodes2, pr.n2, (u32)node);
        const float2 p1 = s1.xy[pr.base1 + row];
        const tp_line line = tp_epiline(pp->F, (double)p1.x, (double)p1.y);
        const double ex = pp->ex, ey = pp->ey;
        const u32 th_low = (u32)prm->th_low;
        const int top = prm->n_levels - 1;
        u32 q[8];
        bf_load_query(s1.desc + 2 * pr.base1, pos, q);
        for (int j = j0; j < j1; j += 4) {              // four rows requested before the first distance is formed
            uint4 a[4], b[4];
            int r[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int jj = min(j + u, j1 - 1);
                a[u] = rows2[2 * (size_t)jj];
                b[u] = rows2[2 * (size_t)jj + 1];
                r[u] = order2[jj];
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                u32 d = bcnt_acc(q[0] ^ a[u].x, 0);
                d = bcnt_acc(q[1] ^ a[u].y, d);
                d = bcnt_acc(q[2] ^ a[u].z, d);
                d = bcnt_acc(q[3] ^ a[u].w, d);
                d = bcnt_acc(q[4] ^ b[u].x, d);
                d = bcnt_acc(q[5] ^ b[u].y, d);
                d = bcnt_acc(q[6] ^ b[u].z, d);
                d = bcnt_acc(q[7] ^ b[u].w, d);
                const u32 key = (d << SLAM_KEY_IDX_BITS) | (u32)r[u];
                // only a row that would enter the top-2 pays for its pixel, its level and the f64 gates
                if (!(j + u < j1 && d <= th_low && key < b2)) continue;
                if (taken2 && taken2[r[u]]) continue;
                const float2 p2 = xy2[r[u]];
                const int l = min(max(level2[r[u]], 0), top);
                if (!tp_off_epipole(ex, ey, (double)p2.x, (double)p2.y, prm->epi_lim[l])) continue;
                if (!tp_on_line(line, (double)p2.x, (double)p2.y, prm->line_lim[l])) continue;
                b2 = min(b2, max(b1, key));
                b1 = min(b1, key);
            }
        }
    }
    const int i0 = bf_key_idx(b1, 0), d0 = bf_key_dist(b1), i1 = bf_key_idx(b2, 0), d1 = bf_key_dist(b2);
    idx[pr.out1 + row] = make_int2(i0, i1);
    dist[pr.out1 + row] = make_int2(d0, d1);
    if (i0 >= 0) atomicMin(&owner[pr.own2 + i0], mf_claim_key(d0, row));
}

// --------------------------------------------------------------------------------------------------------------- finish
struct tm_select {
    __device__ __forceinline__ bool proposed(const mf_pair&, int2 ix, int2) const { return ix.x >= 0; }
};

__global__ __launch_bounds__(MF_FIN_THREADS) void tm_finish_kernel(const uint8_t* bins1, const uint8_t* bins2, const tm_pair* __restrict__ pairs,
                                                                  const int2* __restrict__ idx, const int2* __restrict__ dist,
                                                                  const u32* __restrict__ owner, int* __restrict__ matches12,
                                                                  int* __restrict__ count) {
    const mf_pair pr = pairs[blockIdx.x].m;
    mf_finish(tm_select{}, pr, bins1, bins2, idx, dist, owner, matches12, count + blockIdx.x);
}

// ---------------------------------------------------------------------------------------------------------- triangulate
// TM_TRI_ROWS side-1 rows per workgroup.  The rows that hold a match are packed to the front of the workgroup (ballot, a
// prefix over the four waves, a list in LDS) before the geometry runs: at one match in five rows one wave does the Jacobi
// sweeps of the DLT for the block instead of four.  A row's result is a function of the row alone, so the packing cannot show.
__global__ __launch_bounds__(TM_TRI_ROWS) void tm_triangulate_kernel(const tm_views v1, const tm_views v2, const tt_pair* __restrict__ pairs, int P,
                                                                    const tp_params* __restrict__ prm, const int* __restrict__ matches12,
                                                                    double* __restrict__ X, double* __restrict__ normal,
                                                                    double* __restrict__ range, int* __restrict__ status,
                                                                    int* __restrict__ created) {
    __shared__ int s_row[TM_TRI_ROWS], s_match[TM_TRI_ROWS], s_wave[TM_TRI_ROWS / 64];
    const int bx = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = mf_pair_of(pairs, P, bx);
    const tt_pair* pp = pairs + p;
    const mf_pair pr = pp->m;
    const int first = (bx - pr.blk0) * TM_TRI_ROWS, i = first + tid;
    const double nan = __builtin_nan("");
    int j = -1;
    if (i < pr.n1) {
        j = matches12[pr.out1 + i];
        if (!(j >= 0 && j < pr.n2)) {                   // no match: the row's result is written here
            j = -1;
            const size_t g = (size_t)(pr.out1 + i);
            X[3 * g] = X[3 * g + 1] = X[3 * g + 2] = normal[3 * g] = normal[3 * g + 1] = normal[3 * g + 2] = nan;
            range[2 * g] = range[2 * g + 1] = nan;
            status[g] = 1;
        }
    }
    const unsigned long long mask = __ballot(j >= 0);
    if (lane == 0) s_wave[wave] = __popcll(mask);
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int k = 0; k < TM_TRI_ROWS / 64; k++) {
        base += k < wave ? s_wave[k] : 0;
        total += s_wave[k];
    }
    if (j >= 0) {
        const int slot = base + __popcll(mask & ((1ull << lane) - 1ull));
        s_row[slot] = tid;
        s_match[slot] = j;
    }
    __syncthreads();
    int made = 0;
    if (tid < total) {
        const int r = first + s_row[tid], m = s_match[tid];
        const float2 p1 = v1.xy[pr.base1 + r], p2 = v2.xy[pr.base2 + m];
        const tp_point o = tp_triangulate(*prm, pp->T1, pp->T2, pp->O1, pp->O2, (double)p1.x, (double)p1.y, (double)p2.x, (double)p2.y,
                                          v1.level[pr.base1 + r], v2.level[pr.base2 + m]);
        const size_t g = (size_t)(pr.out1 + r);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            X[3 * g + k] = o.X[k];
            normal[3 * g + k] = o.normal[k];
        }
        range[2 * g] = o.range[0];
        range[2 * g + 1] = o.range[1];
        status[g] = o.status;
        made = o.status == 0 ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) made += __shfl_xor(made, off, 64);
    if (lane == 0 && made) atomicAdd(&created[p], made);
}

// =============================================================== entry points ================================================
extern "C" int slam_tri_match_limits(int32_t* h_limits) {
    SLAM_REQUIRE(h_limits, "slam_tri_match_limits: null pointer");
    h_limits[0] = TM_ROWS_MAX;
    h_limits[1] = TM_PAIRS_MAX;
    h_limits[2] = TM_SCAN_LANES;
    h_limits[3] = TP_LEVELS_MAX;
    h_limits[4] = MF_BINS;
    h_limits[5] = (int32_t)sizeof(tm_pair);
    h_limits[6] = (int32_t)sizeof(tt_pair);
    h_limits[7] = (int32_t)sizeof(tp_params);
    return SLAM_OK;
}

extern "C" int slam_tri_match_plan_describe(int64_t P, int64_t n, int64_t* h_plan) {
    SLAM_REQUIRE(h_plan, "slam_tri_match_plan_describe: null h_plan");
    SLAM_REQUIRE(P >= 0 && P <= TM_PAIRS_MAX, "P=%lld out of range [0, %d]", (long long)P, TM_PAIRS_MAX);
    SLAM_REQUIRE(n >= 0 && n <= TM_ROWS_MAX, "n=%lld out of range [0, %d] rows per image", (long long)n, TM_ROWS_MAX);
    const int64_t per = (n + TM_SCAN_LANES - 1) / TM_SCAN_LANES;
    const mf_plan s = mf_layout(sizeof(tp_params), P, sizeof(tm_pair), P * n, P * n, true);
    const mf_plan t = mf_layout(sizeof(tp_params), P, sizeof(tt_pair), 0, 0, false);
    const int64_t v[6] = {P * per, P, P * ((n + TM_TRI_ROWS - 1) / TM_TRI_ROWS), (int64_t)s.bytes, (int64_t)t.bytes, (int64_t)(MF_BINS * 4 + 8)};
    memcpy(h_plan, v, sizeof(v));
    return SLAM_OK;
}

// a checked slam_bow_groups as kernel arguments, with the side's pixels, levels and marks
static int tm_check_side(const slam_bow_groups* g, const slam_tri_views* v, const char* who, tm_set* out) {
    SLAM_REQUIRE(g && v, "%s: null group set or views", who);
    if (int rc = mf_check_groups(g, who)) return rc;
    SLAM_REQUIRE(g->h_offsets[g->B] == 0 || (v->d_xy && v->d_level), "%s: null pixels or levels", who);
    SLAM_REQUIRE(((uintptr_t)g->d_desc & 15) == 0 && ((uintptr_t)v->d_xy & 7) == 0, "%s: misaligned descriptors or pixels", who);
    out->desc = (const uint4*)g->d_desc;
    out->nodes = g->d_nodes;
    out->order = g->d_order;
    out->inverse = g->d_inverse;
    out->bins = g->d_bins;
    out->xy = (const float2*)v->d_xy;
    out->level = v->d_level;
    out->taken = v->d_taken;
    return SLAM_OK;
}

static int tm_check_params(const slam_tri_params* p, const char* who, bool search, tp_params* out) {
    SLAM_REQUIRE(p, "%s: null parameters", who);
    SLAM_REQUIRE(p->n_levels >= 1 && p->n_levels <= TP_LEVELS_MAX, "%s: n_levels=%d outside [1, %d]", who, p->n_levels, TP_LEVELS_MAX);
    SLAM_REQUIRE(p->h_scale && p->h_sigma2, "%s: null level tables", who);
    SLAM_REQUIRE(!search || (p->th_low >= 0 && p->th_low <= 256), "%s: th_low=%d outside [0, 256]", who, p->th_low);
    SLAM_REQUIRE(!search || (p->chi2 == p->chi2 && p->epipole_r2 == p->epipole_r2), "%s: chi2 or epipole_r2 is not a number", who);
    SLAM_REQUIRE(search || (p->cos_max == p->cos_max && p->chi2_px == p->chi2_px && p->ratio_factor == p->ratio_factor),
                 "%s: cos_max, chi2_px or ratio_factor is not a number", who);
    memset(out, 0, sizeof(*out));
    out->fx = p->fx, out->fy = p->fy, out->cx = p->cx, out->cy = p->cy;
    out->cos_max = p->cos_max, out->chi2_px = p->chi2_px, out->ratio_factor = p->ratio_factor;
    out->n_levels = p->n_levels;
    out->th_low = p->th_low;
    for (int l = 0; l < p->n_levels; l++) {
        out->scale[l] = p->h_scale[l];
        out->sigma2[l] = p->h_sigma2[l];
        out->line_lim[l] = p->chi2 * p->h_sigma2[l];
        out->epi_lim[l] = p->epipole_r2 * p->h_scale[l];
    }
    return SLAM_OK;
}

extern "C" int slam_tri_match_search(slam_ctx* ctx, const slam_bow_groups* g1, const slam_bow_groups* g2, const slam_tri_views* views1,
                                     const slam_tri_views* views2, const int32_t* h_pairs, int64_t P, const double* h_F,
                                     const double* h_epipole, const slam_tri_params* params, int scan_order, int32_t* d_matches12,
                                     int32_t* d_count, int32_t* d_idx, int32_t* d_dist) {
    const char* who = "slam_tri_match_search";
    SLAM_REQUIRE(ctx, "%s: null ctx", who);
    tm_set s1, s2;
    tp_params prm;
    if (int rc = tm_check_side(g1, views1, who, &s1)) return rc;
    if (int rc = tm_check_side(g2, views2, who, &s2)) return rc;
    if (int rc = tm_check_params(params, who, true, &prm)) return rc;
    SLAM_REQUIRE(P >= 0 && P <= TM_PAIRS_MAX, "%s: P=%lld pairs out of range [0, %d]", who, (long long)P, TM_PAIRS_MAX);
    SLAM_REQUIRE(scan_order == 0 || scan_order == 1, "%s: scan_order=%d not in {0, 1}", who, scan_order);
    SLAM_REQUIRE((d_idx != nullptr) == (d_dist != nullptr), "%s: the top-2 tables come as a pair", who);
    SLAM_REQUIRE((g1->d_bins != nullptr) == (g2->d_bins != nullptr), "%s: the orientation bins come for both sides or for neither", who);
    if (P == 0) return SLAM_OK;
    SLAM_REQUIRE(h_pairs && h_F && h_epipole, "%s: null pair arrays", who);
    const size_t head = (size_t)slam_align_up(sizeof(tp_params));
    std::vector<char> block(head + (size_t)P * sizeof(tm_pair));
    memcpy(block.data(), &prm, sizeof(prm));
    tm_pair* table = (tm_pair*)(block.data() + head);
    mf_totals t{0, 0, 0};
    for (int64_t p = 0; p < P; p++) {
        tm_pair& e = table[(size_t)p];
        if (int rc = mf_pair_next(e.m, g1->h_offsets, g1->B, h_pairs[2 * p], g2->h_offsets, g2->B, h_pairs[2 * p + 1], TM_SCAN_LANES, t, who, p))
            return rc;
        memcpy(e.F, h_F + 9 * p, sizeof(e.F));
        e.ex = h_epipole[2 * p];
        e.ey = h_epipole[2 * p + 1];
    }
    const int64_t out1 = t.out1, own2 = t.own2, blocks = t.blocks;
    SLAM_REQUIRE(d_count && (out1 == 0 || d_matches12), "%s: null result pointer", who);
    std::lock_guard<std::mutex> lk(ctx->call_mu);       // the parameters, the pair table, the claim words and the tables nobody asked for
    SLAM_HIP(hipSetDevice(ctx->device));
    const mf_plan pl = mf_layout(sizeof(tp_params), P, sizeof(tm_pair), out1, own2, d_idx == nullptr);
    void* ws = nullptr;
    if (int rc = slam_workspace(ctx, pl.bytes, &ws)) return rc;
    char* w = (char*)ws;
    if (int rc = mf_stage(ctx, pl, w, block.data(), own2)) return rc;
    const tm_pair* d_pairs = (const tm_pair*)(w + pl.o_pairs);
    const tp_params* d_prm = (const tp_params*)w;
    int2* idx = d_idx ? (int2*)d_idx : (int2*)(w + pl.o_idx);
    int2* dist = d_dist ? (int2*)d_dist : (int2*)(w + pl.o_dist);
    u32* owner = (u32*)(w + pl.o_owner);
    if (blocks > 0) {
        if (int rc = slam_prof_begin(ctx)) return rc;
        tm_scan_kernel<<<(unsigned)blocks, TM_SCAN_LANES, 0, ctx->stream>>>(s1, s2, d_pairs, (int)P, d_prm, scan_order, idx, dist, owner);
        if (int rc = slam_prof_end(ctx)) return rc;
        if (int rc = slam_launch_check("tri match scan")) return rc;
    }
    tm_finish_kernel<<<(unsigned)P, MF_FIN_THREADS, 0, ctx->stream>>>(s1.bins, s2.bins, d_pairs, idx, dist, owner, d_matches12, d_count);
    return slam_launch_check("tri match finish");
}

extern "C" int slam_tri_match_triangulate(slam_ctx* ctx, const int64_t* h_offsets1, int64_t B1, const int64_t* h_offsets2, int64_t B2,
                                          const slam_tri_views* views1, const slam_tri_views* views2, const int32_t* h_pairs, int64_t P,
                                          const int32_t* d_matches12, const double* h_T1, const double* h_T2, const double* h_O1,
                                          const double* h_O2, const slam_tri_params* params, double* d_X, double* d_normal, double* d_range,
                                          int32_t* d_status, int32_t* d_created) {
    const char* who = "slam_tri_match_triangulate";
    SLAM_REQUIRE(ctx, "%s: null ctx", who);
    if (int rc = mf_check_offsets(h_offsets1, B1, who, "image")) return rc;
    if (int rc = mf_check_offsets(h_offsets2, B2, who, "image")) return rc;
    SLAM_REQUIRE(views1 && views2, "%s: null views", who);
    SLAM_REQUIRE((h_offsets1[B1] == 0 || (views1->d_xy && views1->d_level)) && (h_offsets2[B2] == 0 || (views2->d_xy && views2->d_level)),
                 "%s: null pixels or levels", who);
    SLAM_REQUIRE(((uintptr_t)views1->d_xy & 7) == 0 && ((uintptr_t)views2->d_xy & 7) == 0, "%s: pixel pointers must be 8-byte aligned", who);
    tp_params prm;
    if (int rc = tm_check_params(params, who, false, &prm)) return rc;
    SLAM_REQUIRE(P >= 0 && P <= TM_PAIRS_MAX, "%s: P=%lld pairs out of range [0, %d]", who, (long long)P, TM_PAIRS_MAX);
    if (P == 0) return SLAM_OK;
    SLAM_REQUIRE(h_pairs && h_T1 && h_T2 && h_O1 && h_O2, "%s: null pair arrays", who);
    const size_t head = (size_t)slam_align_up(sizeof(tp_params));
    std::vector<char> block(head + (size_t)P * sizeof(tt_pair));
    memcpy(block.data(), &prm, sizeof(prm));
    tt_pair* table = (tt_pair*)(block.data() + head);
    mf_totals t{0, 0, 0};
    for (int64_t p = 0; p < P; p++) {
        tt_pair& e = table[(size_t)p];
        if (int rc = mf_pair_next(e.m, h_offsets1, B1, h_pairs[2 * p], h_offsets2, B2, h_pairs[2 * p + 1], TM_TRI_ROWS, t, who, p)) return rc;
        memcpy(e.T1, h_T1 + 12 * p, sizeof(e.T1));
        memcpy(e.T2, h_T2 + 12 * p, sizeof(e.T2));
        memcpy(e.O1, h_O1 + 3 * p, sizeof(e.O1));
        memcpy(e.O2, h_O2 + 3 * p, sizeof(e.O2));
    }
    SLAM_REQUIRE(d_created && (t.out1 == 0 || (d_matches12 && d_X && d_normal && d_range && d_status)), "%s: null device pointer", who);
    std::lock_guard<std::mutex> lk(ctx->call_mu);       // the parameters and the pair table travel through the workspace
    SLAM_HIP(hipSetDevice(ctx->device));
    const mf_plan pl = mf_layout(sizeof(tp_params), P, sizeof(tt_pair), 0, 0, false);     // (no tables, no claim words)
    void* ws = nullptr;
    if (int rc = slam_workspace(ctx, pl.bytes, &ws)) return rc;
    char* w = (char*)ws;
    if (int rc = mf_stage(ctx, pl, w, block.data(), 0)) return rc;
    SLAM_HIP(hipMemsetAsync(d_created, 0, (size_t)P * 4, ctx->stream));
    if (t.blocks == 0) return SLAM_OK;
    const tm_views v1{(const float2*)views1->d_xy, views1->d_level}, v2{(const float2*)views2->d_xy, views2->d_level};
    if (int rc = slam_prof_begin(ctx)) return rc;
    tm_triangulate_kernel<<<(unsigned)t.blocks, TM_TRI_ROWS, 0, ctx->stream>>>(v1, v2, (const tt_pair*)(w + pl.o_pairs), (int)P,
                                                                              (const tp_params*)w, d_matches12, d_X, d_normal,
                                                                              d_range, d_status, d_created);
    if (int rc = slam_prof_end(ctx)) return rc;
    return slam_launch_check("tri match triangulate");
}
