// proj_match.hip - ORBmatcher::SearchByProjection: map points matched into frames by projecting them under a
// first pose estimate and comparing descriptors inside a pixel window, batched over (point set, frame, pose) pairs.
//   grid    per frame, once: the cell of every feature row (pm_cell_kernel), the LDS sort of bow_match.hip's group step with
//           cells as nodes (slam_bow_match_group), and the pixels and levels gathered into the sorted order (pm_gather_kernel);
//   scan    one map point per lane: the gates of proj_point.h in registers, then the grid rows its window touches - the run
//           of cells of one grid row is one contiguous segment, found by two binary searches - the top-2 of the packed keys
//           dist << 23 | row in registers, and the claim of the proposed row by one 32-bit atomic minimum;
//   finish  the claim check and rotation histogram of match_finish.h under this search's selection.
// The gates are f64 with contraction off; everything behind them is a comparison of doubles or integers, integer minima and LDS
// integer adds: the same bits on every run, for every launch geometry and every cell size.
#include "proj_search.h"

// ----------------------------------------------------------------------------------------------------------------- grid
__global__ __launch_bounds__(PM_ROW_THREADS) void pm_cell_kernel(const float2* __restrict__ xy, int64_t n, double cell, int gw, int gh,
                                                                int* __restrict__ cells) {
    const int64_t i = (int64_t)blockIdx.x * PM_ROW_THREADS + threadIdx.x;
    if (i >= n) return;
    const float2 p = xy[i];
    cells[i] = pm_cell_of((double)p.y, cell, gh) * gw + pm_cell_of((double)p.x, cell, gw);
}

__global__ __launch_bounds__(PM_ROW_THREADS) void pm_gather_kernel(const float2* __restrict__ xy, const int* __restrict__ level,
                                                                  const uint8_t* __restrict__ taken, const int64_t* __restrict__ offsets,
                                                                  const int* __restrict__ order, float2* __restrict__ xy_sorted,
                                                                  int* __restrict__ meta_sorted) {
    const int64_t base = offsets[blockIdx.x];           // (the frame on x: a call may hold more frames than a grid's y extent)
    const int n = (int)(offsets[blockIdx.x + 1] - base);
    const int p = (int)blockIdx.y * PM_ROW_THREADS + (int)threadIdx.x;
    if (p >= n) return;
    const int64_t row = base + order[base + p];
    xy_sorted[base + p] = xy[row];
    const int l = level[row];
    meta_sorted[base + p] = (taken && taken[row]) || l < 0 ? -1 : l;
}

// ----------------------------------------------------------------------------------------------------------------- scan
// the selection of DESIGN.md 4l (c): ORB-SLAM's rule - the ratio only between two neighbours of one level, a lone one passes
struct pm_select {
    const int* level2;
    int th_high;
    double ratio;
    __device__ __forceinline__ bool proposed(const mf_pair& pr, int2 ix, int2 ds) const {
        if (ix.x < 0 || ds.x > th_high) return false;
        return !(ix.y >= 0 && level2[pr.base2 + ix.x] == level2[pr.base2 + ix.y] && (double)ds.x > ratio * (double)ds.y);
    }
};

// One lane per map point.  SEARCH false: the gates alone (project_points).  (The grid walk below is the second copy of pm_walk
// of grid_walk.h, kept because the kernel built on the template missed one line of its timing rule; grid_walk.h and DESIGN.md
// 7, item 6, say which.)
template <bool SEARCH>
__global__ __launch_bounds__(PM_SCAN_LANES) void pm_scan_kernel(const pm_points s1, const pm_frames s2, const pm_pair* __restrict__ pairs, int P,
                                                               const pm_params* __restrict__ prm, int2* __restrict__ idx,
                                                               int2* __restrict__ dist, u32* __restrict__ owner, int* __restrict__ status,
                                                               double* __restrict__ tu, double* __restrict__ tv, int* __restrict__ tlp) {
    const int bx = (int)blockIdx.x;
    int lo = 0, hi = P - 1;
    while (lo < hi) {                                   // the last pair whose first workgroup is not behind this one
        const int mid = (lo + hi + 1) >> 1;
        if (pairs[mid].m.blk0 <= bx) lo = mid;
        else hi = mid - 1;
    }
    const pm_pair* pp = pairs + lo;
    const mf_pair pr = pp->m;
    const int i = (bx - pr.blk0) * PM_SCAN_LANES + (int)threadIdx.x;
    if (i >= pr.n1) return;
    const int64_t g = pr.base1 + i;
    const pp_result o = pp_gates(prm->cam, pp->A, pp->Ow, pp->th, s1.xyz + 3 * g, s1.range ? s1.range + 2 * g : nullptr,
                                 s1.normal ? s1.normal + 3 * g : nullptr, s1.level ? s1.level + g : nullptr);
    if (status) {
        status[pr.out1 + i] = o.status;
        tu[pr.out1 + i] = o.u;
        tv[pr.out1 + i] = o.v;
        tlp[pr.out1 + i] = o.lp;
    }
    if (!SEARCH) return;
    u32 b1 = SLAM_KEY_NONE, b2 = SLAM_KEY_NONE;
    if (o.status == 0 && pr.n2 > 0) {
        const double u = o.u, v = o.v, r = o.r;
        // the grid may only remove rows that are out of window: the cell of a coordinate is monotone in it, and the window's
        // ends are pushed out by far more than the rounding of x - u in the test below can move them
        const double pad_u = 1e-9 * (fabs(u) + r), pad_v = 1e-9 * (fabs(v) + r);
        const int cx0 = pm_cell_of((u - r) - pad_u, s2.cell, s2.gw), cx1 = pm_cell_of((u + r) + pad_u, s2.cell, s2.gw);
        const int cy0 = pm_cell_of((v - r) - pad_v, s2.cell, s2.gh), cy1 = pm_cell_of((v + r) + pad_v, s2.cell, s2.gh);
        const int l0 = prm->level_rule ? max(o.lp + prm->lo, 0) : 0, l1 = prm->level_rule ? o.lp + prm->hi : 0x7FFFFFFF;
        const int* cells2 = s2.cells + pr.base2;
        const int* order2 = s2.order + pr.base2;
        const int* meta2 = s2.meta + pr.base2;
        const float2* xy2 = s2.xy + pr.base2;
        const uint4* rows2 = s2.desc + 2 * pr.base2;
        u32 q[8];
        bf_load_query(s1.desc + 2 * pr.base1, i, q);
        for (int cy = cy0; cy <= cy1; cy++) {
            // the two ends of the run of cells [cx0, cx1] of this grid row, searched side by side: one load latency a step, not two
            const u32 c0 = (u32)(cy * s2.gw + cx0), c1 = (u32)(cy * s2.gw + cx1);
            int j0 = 0, h0 = pr.n2, j1 = 0, h1 = pr.n2;
            while (j0 < h0 || j1 < h1) {
                const int m0 = (j0 + h0) >> 1, m1 = (j1 + h1) >> 1;
                const u32 x0 = (u32)cells2[min(m0, pr.n2 - 1)], x1 = (u32)cells2[min(m1, pr.n2 - 1)];
                if (j0 < h0) {
                    if (x0 < c0) j0 = m0 + 1;
                    else h0 = m0;
                }
                if (j1 < h1) {
                    if (x1 <= c1) j1 = m1 + 1;
                    else h1 = m1;
                }
            }
            for (int j = j0; j < j1; j += 4) {          // the pixels and levels of four rows requested before the first test
                float2 p[4];
                int m[4];
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    const int jj = min(j + t, j1 - 1);
                    p[t] = xy2[jj];
                    m[t] = meta2[jj];
                }
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    if (!(j + t < j1 && m[t] >= l0 && m[t] <= l1 && fabs((double)p[t].x - u) < r && fabs((double)p[t].y - v) < r)) continue;
                    const uint4 a = rows2[2 * (size_t)(j + t)], b = rows2[2 * (size_t)(j + t) + 1];     // (only a row inside the window)
                    u32 d = bcnt_acc(q[0] ^ a.x, 0);
                    d = bcnt_acc(q[1] ^ a.y, d);
                    d = bcnt_acc(q[2] ^ a.z, d);
                    d = bcnt_acc(q[3] ^ a.w, d);
                    d = bcnt_acc(q[4] ^ b.x, d);
                    d = bcnt_acc(q[5] ^ b.y, d);
                    d = bcnt_acc(q[6] ^ b.z, d);
                    d = bcnt_acc(q[7] ^ b.w, d);
                    const u32 key = (d << SLAM_KEY_IDX_BITS) | (u32)order2[j + t];
                    b2 = min(b2, max(b1, key));
                    b1 = min(b1, key);
                }
            }
        }
    }
    const int2 ix = make_int2(bf_key_idx(b1, 0), bf_key_idx(b2, 0)), ds = make_int2(bf_key_dist(b1), bf_key_dist(b2));
    idx[pr.out1 + i] = ix;
    dist[pr.out1 + i] = ds;
    const pm_select sel{s2.level, prm->th_high, prm->ratio};
    if (sel.proposed(pr, ix, ds)) atomicMin(&owner[pr.own2 + ix.x], mf_claim_key(ds.x, i));
}

// --------------------------------------------------------------------------------------------------------------- finish
__global__ __launch_bounds__(MF_FIN_THREADS) void pm_finish_kernel(const uint8_t* bins1, const pm_frames s2, const pm_pair* __restrict__ pairs,
                                                                  const pm_params* __restrict__ prm, const int2* __restrict__ idx,
                                                                  const int2* __restrict__ dist, const u32* __restrict__ owner,
                                                                  int* __restrict__ matches12, int* __restrict__ count) {
    const mf_pair pr = pairs[blockIdx.x].m;
    mf_finish(pm_select{s2.level, prm->th_high, prm->ratio}, pr, bins1, s2.bins, idx, dist, owner, matches12, count + blockIdx.x);
}

// =============================================================== entry points ================================================
extern "C" int slam_proj_match_limits(int32_t* h_limits) {
    SLAM_REQUIRE(h_limits, "slam_proj_match_limits: null pointer");
    h_limits[0] = PM_ROWS_MAX;
    h_limits[1] = PM_PAIRS_MAX;
    h_limits[2] = PM_SCAN_LANES;
    h_limits[3] = PP_LEVELS_MAX;
    h_limits[4] = MF_BINS;
    h_limits[5] = (int32_t)sizeof(pm_pair);
    return SLAM_OK;
}

extern "C" int slam_proj_match_plan_describe(int64_t B, int64_t P, int64_t n, int64_t* h_plan) {
    SLAM_REQUIRE(h_plan, "slam_proj_match_plan_describe: null h_plan");
    SLAM_REQUIRE(B >= 0 && P >= 0 && P <= PM_PAIRS_MAX, "B=%lld, P=%lld out of range", (long long)B, (long long)P);
    SLAM_REQUIRE(n >= 0 && n <= PM_ROWS_MAX, "n=%lld out of range [0, %d] rows per image", (long long)n, PM_ROWS_MAX);
    const int64_t per = (n + PM_SCAN_LANES - 1) / PM_SCAN_LANES, row_blocks = (B * n + PM_ROW_THREADS - 1) / PM_ROW_THREADS;
    const mf_plan p = mf_layout(sizeof(pm_params), P, sizeof(pm_pair), P * n, P * n, true);
    const int64_t v[8] = {row_blocks, B, B * ((n + PM_ROW_THREADS - 1) / PM_ROW_THREADS), P * per, P, (int64_t)p.bytes,
                          (int64_t)(MF_BINS * 4 + 8), (int64_t)slam_align_up((uint64_t)(B + 1) * 8)};
    memcpy(h_plan, v, sizeof(v));
    return SLAM_OK;
}

extern "C" int slam_proj_match_grid(slam_ctx* ctx, const void* d_desc, const float* d_xy, const int32_t* d_level, const uint8_t* d_taken,
                                    const int64_t* h_offsets, int64_t B, int W, int H, int cell, int32_t* d_cells, void* d_desc_sorted,
                                    int32_t* d_cells_sorted, int32_t* d_order, int32_t* d_inverse, float* d_xy_sorted,
                                    int32_t* d_meta_sorted) {
    SLAM_REQUIRE(ctx, "slam_proj_match_grid: null ctx");
    if (int rc = mf_check_offsets(h_offsets, B, "slam_proj_match_grid", "frame")) return rc;
    int gw, gh;
    if (int rc = pm_check_grid(W, H, cell, "slam_proj_match_grid", &gw, &gh)) return rc;
    const int64_t n = h_offsets[B];
    if (n == 0) return SLAM_OK;
    SLAM_REQUIRE(d_desc && d_xy && d_level && d_cells && d_desc_sorted && d_cells_sorted && d_order && d_inverse && d_xy_sorted && d_meta_sorted,
                 "slam_proj_match_grid: null device pointer");
    SLAM_REQUIRE(((uintptr_t)d_desc & 15) == 0 && ((uintptr_t)d_desc_sorted & 15) == 0, "descriptor pointers must be 16-byte aligned");
    SLAM_REQUIRE(((uintptr_t)d_xy & 7) == 0 && ((uintptr_t)d_xy_sorted & 7) == 0, "pixel pointers must be 8-byte aligned");
    int64_t n_max = 0;
    for (int64_t b = 0; b < B; b++) n_max = std::max(n_max, h_offsets[b + 1] - h_offsets[b]);
    {
        std::lock_guard<std::mutex> lk(ctx->call_mu);
        SLAM_HIP(hipSetDevice(ctx->device));
        pm_cell_kernel<<<(unsigned)((n + PM_ROW_THREADS - 1) / PM_ROW_THREADS), PM_ROW_THREADS, 0, ctx->stream>>>((const float2*)d_xy, n, (double)cell,
                                                                                                                 gw, gh, d_cells);
        if (int rc = slam_launch_check("proj match cells")) return rc;
    }
    // cells as nodes: the sort and the descriptor gather of SearchByBoW's group step (it takes the call lock itself)
    if (int rc = slam_bow_match_group(ctx, d_desc, d_cells, h_offsets, B, d_desc_sorted, d_cells_sorted, d_order, d_inverse)) return rc;
    std::lock_guard<std::mutex> lk(ctx->call_mu);       // the offsets travel through the context's workspace
    void* ws = nullptr;
    if (int rc = slam_workspace(ctx, slam_align_up((uint64_t)(B + 1) * 8), &ws)) return rc;
    SLAM_HIP(hipMemcpyAsync(ws, h_offsets, (size_t)(B + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    pm_gather_kernel<<<dim3((unsigned)B, (unsigned)((n_max + PM_ROW_THREADS - 1) / PM_ROW_THREADS)), PM_ROW_THREADS, 0, ctx->stream>>>(
        (const float2*)d_xy, d_level, d_taken, (const int64_t*)ws, d_order, (float2*)d_xy_sorted, d_meta_sorted);
    return slam_launch_check("proj match gather");
}

// the common body of the projection alone (frames null) and the search
static int pm_run(slam_ctx* ctx, const slam_proj_points* pts, const slam_proj_frames* frames, const int32_t* h_a, const int32_t* h_b, int stride,
                  const double* h_poses, const double* h_centres, const double* h_th, int64_t P, const slam_proj_params* params,
                  int32_t* d_matches12, int32_t* d_count, int32_t* d_status, double* d_u, double* d_v, int32_t* d_lp, int32_t* d_idx,
                  int32_t* d_dist, const char* who) {
    const bool search = frames != nullptr;
    SLAM_REQUIRE(ctx, "%s: null ctx", who);
    pm_points s1;
    pm_frames s2;
    memset(&s2, 0, sizeof(s2));
    pm_params prm;
    if (int rc = pm_check_points(pts, who, &s1)) return rc;
    if (int rc = pm_check_params(params, who, search, &prm)) return rc;
    if (search) {
        if (int rc = pm_check_frames(frames, pts, who, &s2)) return rc;
    }
    SLAM_REQUIRE(P >= 0 && P <= PM_PAIRS_MAX, "%s: P=%lld pairs out of range [0, %d]", who, (long long)P, PM_PAIRS_MAX);
    const bool tables = d_status != nullptr;
    SLAM_REQUIRE((d_u != nullptr) == tables && (d_v != nullptr) == tables && (d_lp != nullptr) == tables,
                 "%s: the tables status, u, v, lp come together or not at all", who);
    SLAM_REQUIRE((d_idx != nullptr) == (d_dist != nullptr), "%s: the top-2 tables come as a pair", who);
    SLAM_REQUIRE(search || tables, "%s: null result pointer", who);
    if (P == 0) return SLAM_OK;
    SLAM_REQUIRE(h_a && h_poses && h_centres && h_th && (!search || h_b), "%s: null pair arrays", who);
    const size_t head = (size_t)slam_align_up(sizeof(pm_params));
    std::vector<char> block(head + (size_t)P * sizeof(pm_pair));
    memcpy(block.data(), &prm, sizeof(prm));
    pm_pair* table = (pm_pair*)(block.data() + head);
    mf_totals t{0, 0, 0};
    for (int64_t p = 0; p < P; p++) {
        pm_pair& e = table[(size_t)p];
        if (int rc = mf_pair_next(e.m, pts->h_offsets, pts->B, h_a[stride * p], search ? frames->h_offsets : nullptr, search ? frames->B : 0,
                                  search ? h_b[stride * p] : 0, PM_SCAN_LANES, t, who, p))
            return rc;
        SLAM_REQUIRE(h_th[p] > 0.0, "%s: th[%lld] is not positive", who, (long long)p);
        memcpy(e.A, h_poses + 12 * p, sizeof(e.A));
        memcpy(e.Ow, h_centres + 3 * p, sizeof(e.Ow));
        e.th = h_th[p];
    }
    const int64_t out1 = t.out1, own2 = t.own2, blocks = t.blocks;      // (own2 = 0 without a side 2)
    SLAM_REQUIRE(!search || (d_count && (out1 == 0 || d_matches12)), "%s: null result pointer", who);
    if (!search && out1 == 0) return SLAM_OK;
    std::lock_guard<std::mutex> lk(ctx->call_mu);       // the pair table, the parameters, the claim words and the tables nobody asked for
    SLAM_HIP(hipSetDevice(ctx->device));
    const mf_plan pl = mf_layout(sizeof(pm_params), P, sizeof(pm_pair), search ? out1 : 0, own2, search && d_idx == nullptr);
    void* ws = nullptr;
    if (int rc = slam_workspace(ctx, pl.bytes, &ws)) return rc;
    char* w = (char*)ws;
    if (int rc = mf_stage(ctx, pl, w, block.data(), own2)) return rc;
    const pm_pair* d_pairs = (const pm_pair*)(w + pl.o_pairs);
    const pm_params* d_prm = (const pm_params*)w;
    int2* idx = d_idx ? (int2*)d_idx : (int2*)(w + pl.o_idx);
    int2* dist = d_dist ? (int2*)d_dist : (int2*)(w + pl.o_dist);
    u32* owner = (u32*)(w + pl.o_owner);
    if (blocks > 0) {
        if (int rc = slam_prof_begin(ctx)) return rc;
        if (search)
            pm_scan_kernel<true><<<(unsigned)blocks, PM_SCAN_LANES, 0, ctx->stream>>>(s1, s2, d_pairs, (int)P, d_prm, idx, dist, owner, d_status, d_u,
                                                                                      d_v, d_lp);
        else
            pm_scan_kernel<false><<<(unsigned)blocks, PM_SCAN_LANES, 0, ctx->stream>>>(s1, s2, d_pairs, (int)P, d_prm, idx, dist, owner, d_status,
                                                                                       d_u, d_v, d_lp);
        if (int rc = slam_prof_end(ctx)) return rc;
        if (int rc = slam_launch_check("proj match scan")) return rc;
    }
    if (!search) return SLAM_OK;
    pm_finish_kernel<<<(unsigned)P, MF_FIN_THREADS, 0, ctx->stream>>>(s1.bins, s2, d_pairs, d_prm, idx, dist, owner, d_matches12, d_count);
    return slam_launch_check("proj match finish");
}

extern "C" int slam_proj_match_project(slam_ctx* ctx, const slam_proj_points* points, const int32_t* h_sets, const double* h_poses,
                                       const double* h_centres, const double* h_th, int64_t P, const slam_proj_params* params,
                                       int32_t* d_status, double* d_u, double* d_v, int32_t* d_lp) {
    return pm_run(ctx, points, nullptr, h_sets, nullptr, 1, h_poses, h_centres, h_th, P, params, nullptr, nullptr, d_status, d_u, d_v, d_lp,
                  nullptr, nullptr, "slam_proj_match_project");
}

extern "C" int slam_proj_match_search(slam_ctx* ctx, const slam_proj_points* points, const slam_proj_frames* frames, const int32_t* h_pairs,
                                      const double* h_poses, const double* h_centres, const double* h_th, int64_t P,
                                      const slam_proj_params* params, int32_t* d_matches12, int32_t* d_count, int32_t* d_status, double* d_u,
                                      double* d_v, int32_t* d_lp, int32_t* d_idx, int32_t* d_dist) {
    SLAM_REQUIRE(frames, "slam_proj_match_search: null frame set");
    return pm_run(ctx, points, frames, h_pairs, h_pairs ? h_pairs + 1 : nullptr, 2, h_poses, h_centres, h_th, P, params, d_matches12, d_count,
                  d_status, d_u, d_v, d_lp, d_idx, d_dist, "slam_proj_match_search");
}
