// fuse.hip - ORBmatcher::Fuse and the refresh of fused map points: LocalMapping::SearchInNeighbors' two steps,
// and LoopClosing::SearchAndFuse under a Sim(3) pose, batched.
//   search  one map point per lane: the binary search of its observation list for the pair's frame (status 5), the gates of
//           fuse_point.h in registers, the grid walk of grid_walk.h with the reprojection gate on every row inside the window,
//           the single nearest row as one packed key, and the claim of that row by one 32-bit atomic minimum;
//   finish  one workgroup per pair: the claim check (status 8 with the winner's id), the link (`other`) and the three counts;
//   refresh G lanes per map point, 256 / G points per workgroup, G in {16, 64, 256} by the length of the observation list: the
//           descriptors and views staged in LDS, lane i the median of row i of the distance table by counting
//           (fp_median), one LDS atomic minimum of (median, i) per lane, the normal summed in list order by the point's first lane.
// Everything behind the f64 gates is a comparison, an integer minimum or an integer add: the same bits on every run.
#include "grid_walk.h"
#include "fuse_point.h"

#define FZ_REFRESH_THREADS 256
#define FZ_POINTS_MAX (1ll << 24)   // map points of one observation table

struct fz_pair {
    mf_pair m;
    double A[12], Ow[3], th;
    int frame, pad;                 // the pair's frame, as the observation lists name it
};

static_assert(sizeof(fz_pair) == 184, "the pair table is laid out by the host");

struct fz_params {
    pm_params p;
    double m_lo2, m_hi2;
    double lim[FP_LEVELS_MAX];      // chi2 * sigma2[l]
    int th_low, pad;
};

struct fz_obs {
    const int64_t* offsets;         // [M + 1]
    const int2* obs;                // (frame, row), frames ascending inside a list
    int64_t nnz;
    int M;
};

// ----------------------------------------------------------------------------------------------------------------- search
__global__ __launch_bounds__(PM_SCAN_LANES) void fz_scan_kernel(const pm_points s1, const int* __restrict__ id1, const pm_frames s2, const fz_obs ob,
                                                               const fz_pair* __restrict__ pairs, int P, const fz_params* __restrict__ prm,
                                                               int* __restrict__ row, int* __restrict__ dist, int* __restrict__ status,
                                                               u32* __restrict__ owner, double* __restrict__ tu, double* __restrict__ tv,
                                                               int* __restrict__ tlp) {
    const int bx = (int)blockIdx.x;
    const fz_pair* pp = pairs + mf_pair_of(pairs, P, bx);
    const mf_pair pr = pp->m;
    const int i = (bx - pr.blk0) * PM_SCAN_LANES + (int)threadIdx.x;
    if (i >= pr.n1) return;
    const int64_t g = pr.base1 + i;
    // (a) a point the frame observes already is out: at most eight steps in its list
    const int id = id1[g];
    bool seen = false;
    if (id >= 0 && id < ob.M) {
        const int64_t a = max(ob.offsets[id], (int64_t)0), b = min(ob.offsets[id + 1], ob.nnz);
        const int n = (int)min(max(b - a, (int64_t)0), (int64_t)FP_OBS_MAX);
        int lo = 0, hi = n;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (ob.obs[a + mid].x < pp->frame) lo = mid + 1;
            else hi = mid;
        }
        seen = lo < n && ob.obs[a + lo].x == pp->frame;
    }
    pp_result o;
    if (seen) {
        o.u = o.v = o.r = __builtin_nan("");
        o.status = 5;
        o.lp = -1;
    } else {
        o = fp_gates(prm->p.cam, pp->A, pp->Ow, pp->th, s1.xyz + 3 * g, s1.range ? s1.range + 2 * g : nullptr,
                     s1.normal ? s1.normal + 3 * g : nullptr, s1.level ? s1.level + g : nullptr, prm->m_lo2, prm->m_hi2);
    }
    if (tu) {
        tu[pr.out1 + i] = o.u;
        tv[pr.out1 + i] = o.v;
        tlp[pr.out1 + i] = o.lp;
    }
    int st = o.status, r1 = -1, d1 = SLAM_NO_MATCH_DIST;
    if (st == 0) {
        u32 b1 = SLAM_KEY_NONE;
        if (pr.n2 > 0) {
            const double u = o.u, v = o.v;
            const double* lim = prm->lim;
            const int top = prm->p.cam.n_levels - 1;
            pm_walk(s2, pr, s1.desc + 2 * pr.base1, i, u, v, o.r, max(o.lp + prm->p.lo, 0), o.lp + prm->p.hi,
                    [&](float2 p, int l) { return fp_candidate(u, v, p.x, p.y, lim[min(l, top)]); }, [&](u32 key) { b1 = min(b1, key); });
        }
        r1 = bf_key_idx(b1, 0);
        d1 = bf_key_dist(b1);
        st = r1 < 0 ? 6 : (d1 > prm->th_low ? 7 : 0);
        if (st == 0) atomicMin(&owner[pr.own2 + r1], mf_claim_key(d1, i));
    }
    row[pr.out1 + i] = r1;
    dist[pr.out1 + i] = d1;
    status[pr.out1 + i] = st;
}

// One workgroup per pair: a proposed point keeps its row iff the row's claim word is its own (the smallest (d, i)).
__global__ __launch_bounds__(MF_FIN_THREADS) void fz_finish_kernel(const int* __restrict__ id1, const int* __restrict__ point2,
                                                                  const fz_pair* __restrict__ pairs, const int* __restrict__ row,
                                                                  const int* __restrict__ dist, const u32* __restrict__ owner,
                                                                  int* __restrict__ status, int* __restrict__ other, int* __restrict__ count) {
    __shared__ int s_count[3];
    const mf_pair pr = pairs[blockIdx.x].m;
    const int tid = threadIdx.x;
    if (tid < 3) s_count[tid] = 0;
    __syncthreads();
    int c0 = 0, c1 = 0, c2 = 0;
    for (int i = tid; i < pr.n1; i += MF_FIN_THREADS) {
        int ot = -1;
        if (status[pr.out1 + i] == 0) {
            const int r = row[pr.out1 + i];
            const u32 w = owner[pr.own2 + r];
            if (w == mf_claim_key(dist[pr.out1 + i], i)) {
                ot = point2[pr.base2 + r];
                c0 += ot < 0 ? 1 : 0;
                c1 += ot < 0 ? 0 : 1;
            } else {
                ot = id1[pr.base1 + (int)(w & (MF_ROWS_MAX - 1))];
                status[pr.out1 + i] = 8;
                c2++;
            }
        }
        other[pr.out1 + i] = ot;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        c0 += __shfl_xor(c0, off, 64);
        c1 += __shfl_xor(c1, off, 64);
        c2 += __shfl_xor(c2, off, 64);
    }
    if ((tid & 63) == 0) {
        if (c0) atomicAdd(&s_count[0], c0);
        if (c1) atomicAdd(&s_count[1], c1);
        if (c2) atomicAdd(&s_count[2], c2);
    }
    __syncthreads();
    if (tid < 3) count[3 * blockIdx.x + tid] = s_count[tid];
}

// ---------------------------------------------------------------------------------------------------------------- refresh
struct fz_job {
    int64_t start;                  // the list's first entry in the observation table
    int m, n, out, pad;             // the map point, the length of its list, its place in the outputs
};

static_assert(sizeof(fz_job) == 24, "the job table is laid out by the host");

struct fz_refresh {
    const double* xyz;
    const int2* obs;
    const uint4* desc;              // the frames' descriptors, in row order or (inverse given) in grid order
    const int* inverse;             // the grid position of each row, or null
    const int* level;               // levels in row order
    const int64_t* frame_offsets;   // [B + 1], on the device
    const double* centres;          // [B, 3]
    const int* ref;                 // [M] or null
    const double* scale;            // [n_levels], on the device
    int B, n_levels;
    int* best;
    u32* desc_out;
    double* normal;
    double* range;
};

// G lanes per map point, lane k its observation k; 256 / G points per workgroup.
template <int G>
__global__ __launch_bounds__(FZ_REFRESH_THREADS) void fz_refresh_kernel(const fz_refresh a, const fz_job* __restrict__ jobs, int n_jobs) {
    constexpr int PPB = FZ_REFRESH_THREADS / G;
    __shared__ uint4 s_desc[FZ_REFRESH_THREADS][2];
    __shared__ double s_view[FZ_REFRESH_THREADS][4];
    __shared__ int s_level[FZ_REFRESH_THREADS];
    __shared__ u32 s_key[PPB];
    const int tid = threadIdx.x, slot = tid / G, k = tid % G;
    const int j = (int)blockIdx.x * PPB + slot;
    const bool valid = j < n_jobs;
    fz_job job;
    job.start = 0;
    job.m = job.n = job.out = job.pad = 0;
    if (valid) job = jobs[j];
    const int n = min(job.n, G);
    if (k == 0) s_key[slot] = SLAM_KEY_NONE;
    if (k < n) {
        const int2 o = a.obs[job.start + k];
        const double nan = __builtin_nan("");
        uint4 da = make_uint4(0, 0, 0, 0), db = da;
        double t[4] = {nan, nan, nan, nan};
        int lv = 0;
        if (o.x >= 0 && o.x < a.B) {                    // (an entry outside the frames reads nothing: zero bytes and a NaN view)
            const int64_t base = a.frame_offsets[o.x];
            if (o.y >= 0 && o.y < a.frame_offsets[o.x + 1] - base) {
                const int64_t pos = base + (a.inverse ? a.inverse[base + o.y] : o.y);
                da = a.desc[2 * pos];
                db = a.desc[2 * pos + 1];
                lv = a.level[base + o.y];
                fp_view(a.xyz + 3 * (int64_t)job.m, a.centres + 3 * o.x, t);
            }
        }
        s_desc[tid][0] = da;
        s_desc[tid][1] = db;
        s_view[tid][0] = t[0];
        s_view[tid][1] = t[1];
        s_view[tid][2] = t[2];
        s_view[tid][3] = t[3];
        s_level[tid] = lv;
    }
    __syncthreads();
    if (k < n) {
        const uint4 qa = s_desc[tid][0], qb = s_desc[tid][1];
        const u32 q[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
        const int first = slot * G;
        const int med = fp_median(n, [&](int kk) { return (int)gw_hamming(q, s_desc[first + kk][0], s_desc[first + kk][1]); });
        atomicMin(&s_key[slot], fp_choice_key(med, k));
    }
    __syncthreads();
    if (!valid) return;
    const int best = n > 0 ? (int)(s_key[slot] & 255u) : -1;
    if (k < 8) a.desc_out[8 * (int64_t)job.out + k] = n > 0 ? ((const u32*)&s_desc[slot * G + best][0])[k] : 0u;
    if (k != 0) return;
    a.best[job.out] = best;
    const double nan = __builtin_nan("");
    double nr[3] = {nan, nan, nan}, rg[2] = {nan, nan};
    if (n > 0) {
        const int first = slot * G;
        double s[3] = {s_view[first][0], s_view[first][1], s_view[first][2]};
        for (int kk = 1; kk < n; kk++) {
            s[0] += s_view[first + kk][0];
            s[1] += s_view[first + kk][1];
            s[2] += s_view[first + kk][2];
        }
        const int r = a.ref ? min(max(a.ref[job.m], 0), n - 1) : 0;
        fp_normal_range(s, s_view[first + r][3], s_level[first + r], a.scale, a.n_levels, nr, rg);
    }
    a.normal[3 * (int64_t)job.out] = nr[0];
    a.normal[3 * (int64_t)job.out + 1] = nr[1];
    a.normal[3 * (int64_t)job.out + 2] = nr[2];
    a.range[2 * (int64_t)job.out] = rg[0];
    a.range[2 * (int64_t)job.out + 1] = rg[1];
}

// =============================================================== entry points ================================================
extern "C" int slam_fuse_limits(int32_t* h_limits) {
    SLAM_REQUIRE(h_limits, "slam_fuse_limits: null pointer");
    h_limits[0] = PM_ROWS_MAX;
    h_limits[1] = PM_PAIRS_MAX;
    h_limits[2] = PM_SCAN_LANES;
    h_limits[3] = FP_LEVELS_MAX;
    h_limits[4] = FP_OBS_MAX;
    h_limits[5] = (int32_t)sizeof(fz_pair);
    h_limits[6] = (int32_t)sizeof(fz_job);
    h_limits[7] = FZ_REFRESH_THREADS;
    return SLAM_OK;
}

// the observation table's offsets: ascending from 0, at most FP_OBS_MAX entries a point
static int fz_check_table(const int64_t* off, int64_t M, const char* who) {
    SLAM_REQUIRE(M >= 0 && M <= FZ_POINTS_MAX, "%s: M=%lld map points out of range [0, 2^24]", who, (long long)M);
    SLAM_REQUIRE(off && off[0] == 0, "%s: null observation offsets, or offsets that do not start at 0", who);
    int64_t sign = 0;                                   // one branch-free pass: the sign bit of n or of FP_OBS_MAX - n
    for (int64_t m = 0; m < M; m++) {
        const int64_t n = off[m + 1] - off[m];
        sign |= n | ((int64_t)FP_OBS_MAX - n);
    }
    for (int64_t m = 0; sign < 0 && m < M; m++) {
        const int64_t n = off[m + 1] - off[m];
        SLAM_REQUIRE(n >= 0, "%s: the observation offsets descend at point %lld", who, (long long)m);
        SLAM_REQUIRE(n <= FP_OBS_MAX, "%s: point %lld has %lld observations (at most %d)", who, (long long)m, (long long)n, FP_OBS_MAX);
    }
    SLAM_REQUIRE(off[M] < (1ll << 31), "%s: more than 2^31 observations", who);
    return SLAM_OK;
}

extern "C" int slam_fuse_search(slam_ctx* ctx, const slam_proj_points* points, const int32_t* d_id, const slam_proj_frames* frames,
                                const int32_t* d_point, const int64_t* h_obs_offsets, const int64_t* d_obs_offsets, const int32_t* d_obs,
                                int64_t M, const int32_t* h_pairs, const double* h_poses, const double* h_centres, const double* h_th, int64_t P,
                                const slam_proj_params* params, const slam_fuse_params* fuse, int32_t* d_row, int32_t* d_dist,
                                int32_t* d_status, int32_t* d_other, int32_t* d_count, double* d_u, double* d_v, int32_t* d_lp) {
    const char* who = "slam_fuse_search";               // (the arguments are checked before the context is looked at)
    SLAM_REQUIRE(frames && fuse, "%s: null frame set or fuse parameters", who);
    pm_points s1;
    pm_frames s2;
    memset(&s2, 0, sizeof(s2));
    fz_params prm;
    memset(&prm, 0, sizeof(prm));
    if (int rc = pm_check_points(points, who, &s1)) return rc;
    if (int rc = pm_check_params(params, who, true, &prm.p)) return rc;
    if (int rc = pm_check_frames(frames, points, who, &s2)) return rc;
    if (int rc = fz_check_table(h_obs_offsets, M, who)) return rc;
    SLAM_REQUIRE(fuse->m_lo2 > 0.0 && fuse->m_hi2 > 0.0, "%s: the margins (%g, %g) must be positive numbers", who, fuse->m_lo2, fuse->m_hi2);
    SLAM_REQUIRE(fuse->chi2 == fuse->chi2, "%s: chi2 is not a number", who);
    SLAM_REQUIRE(fuse->th_low >= 0 && fuse->th_low <= 256, "%s: th_low=%d outside [0, 256]", who, fuse->th_low);
    SLAM_REQUIRE(d_obs_offsets && (h_obs_offsets[M] == 0 || d_obs), "%s: null observation table", who);
    SLAM_REQUIRE(((uintptr_t)d_obs & 7) == 0 && ((uintptr_t)d_obs_offsets & 7) == 0, "%s: the observation table must be 8-byte aligned", who);
    SLAM_REQUIRE(points->h_offsets[points->B] == 0 || d_id, "%s: null point ids", who);
    SLAM_REQUIRE(frames->h_offsets[frames->B] == 0 || d_point, "%s: null map points of the frame rows", who);
    SLAM_REQUIRE(P >= 0 && P <= PM_PAIRS_MAX, "%s: P=%lld pairs out of range [0, %d]", who, (long long)P, PM_PAIRS_MAX);
    SLAM_REQUIRE((d_u != nullptr) == (d_v != nullptr) && (d_u != nullptr) == (d_lp != nullptr), "%s: the tables u, v, lp come together or not at all",
                 who);
    prm.m_lo2 = fuse->m_lo2;
    prm.m_hi2 = fuse->m_hi2;
    prm.th_low = fuse->th_low;
    for (int l = 0; l < params->n_levels; l++) prm.lim[l] = fuse->chi2 * params->h_scale2[l];
    SLAM_REQUIRE(ctx, "%s: null ctx", who);
    if (P == 0) return SLAM_OK;
    SLAM_REQUIRE(h_pairs && h_poses && h_centres && h_th, "%s: null pair arrays", who);
    const size_t head = (size_t)slam_align_up(sizeof(fz_params));
    std::vector<char> block(head + (size_t)P * sizeof(fz_pair));
    memcpy(block.data(), &prm, sizeof(prm));
    fz_pair* table = (fz_pair*)(block.data() + head);
    mf_totals t{0, 0, 0};
    for (int64_t p = 0; p < P; p++) {
        fz_pair& e = table[(size_t)p];
        if (int rc = mf_pair_next(e.m, points->h_offsets, points->B, h_pairs[2 * p], frames->h_offsets, frames->B, h_pairs[2 * p + 1],
                                  PM_SCAN_LANES, t, who, p))
            return rc;
        SLAM_REQUIRE(h_th[p] > 0.0, "%s: th[%lld] is not positive", who, (long long)p);
        memcpy(e.A, h_poses + 12 * p, sizeof(e.A));
        memcpy(e.Ow, h_centres + 3 * p, sizeof(e.Ow));
        e.th = h_th[p];
        e.frame = h_pairs[2 * p + 1];
        e.pad = 0;
    }
    const int64_t out1 = t.out1, own2 = t.own2, blocks = t.blocks;
    SLAM_REQUIRE(d_count && (out1 == 0 || (d_row && d_dist && d_status && d_other)), "%s: null result pointer", who);
    std::lock_guard<std::mutex> lk(ctx->call_mu);       // the parameters, the pair table and the claim words
    SLAM_HIP(hipSetDevice(ctx->device));
    const mf_plan pl = mf_layout(sizeof(fz_params), P, sizeof(fz_pair), 0, own2, false);    // (the scan keeps no top-2 tables)
    void* ws = nullptr;
    if (int rc = slam_workspace(ctx, pl.bytes, &ws)) return rc;
    char* w = (char*)ws;
    if (int rc = mf_stage(ctx, pl, w, block.data(), own2)) return rc;
    const fz_pair* d_pairs = (const fz_pair*)(w + pl.o_pairs);
    u32* owner = (u32*)(w + pl.o_owner);
    if (blocks > 0) {
        const fz_obs ob{d_obs_offsets, (const int2*)d_obs, h_obs_offsets[M], (int)M};
        if (int rc = slam_prof_begin(ctx)) return rc;
        fz_scan_kernel<<<(unsigned)blocks, PM_SCAN_LANES, 0, ctx->stream>>>(s1, d_id, s2, ob, d_pairs, (int)P, (const fz_params*)w, d_row, d_dist,
                                                                            d_status, owner, d_u, d_v, d_lp);
        if (int rc = slam_prof_end(ctx)) return rc;
        if (int rc = slam_launch_check("fuse scan")) return rc;
    }
    fz_finish_kernel<<<(unsigned)P, MF_FIN_THREADS, 0, ctx->stream>>>(d_id, d_point, d_pairs, d_row, d_dist, owner, d_status, d_other, d_count);
    return slam_launch_check("fuse finish");
}

extern "C" int slam_fuse_refresh(slam_ctx* ctx, const double* d_xyz, const int64_t* h_obs_offsets, const int32_t* d_obs, int64_t M,
                                 const int32_t* h_select, int64_t K, const void* d_desc, const int32_t* d_inverse, const int32_t* d_level,
                                 const int64_t* h_frame_offsets, int64_t B, const double* d_centres, const int32_t* d_ref, const double* h_scale,
                                 int n_levels, int32_t* d_best, void* d_desc_out, double* d_normal, double* d_range) {
    const char* who = "slam_fuse_refresh";              // (the arguments are checked before the context is looked at)
    SLAM_REQUIRE(M >= 0 && M <= FZ_POINTS_MAX, "%s: M=%lld map points out of range [0, 2^24]", who, (long long)M);
    SLAM_REQUIRE(h_obs_offsets && h_obs_offsets[0] == 0, "%s: null observation offsets, or offsets that do not start at 0", who);
    SLAM_REQUIRE(n_levels >= 1 && n_levels <= FP_LEVELS_MAX && h_scale, "%s: n_levels=%d outside [1, %d], or a null scale table", who, n_levels,
                 FP_LEVELS_MAX);
    if (int rc = mf_check_offsets(h_frame_offsets, B, who, "frame")) return rc;
    if (!h_select) K = M;
    SLAM_REQUIRE(K >= 0 && K <= FZ_POINTS_MAX, "%s: K=%lld selected points out of range", who, (long long)K);
    // the jobs by the length of their lists: G = 16, 64, 256 lanes a point
    int64_t cnt[3] = {0, 0, 0}, at[3];
    std::vector<fz_job> jobs((size_t)K);
    std::vector<uint8_t> cls((size_t)K);
    for (int64_t k = 0; k < K; k++) {
        const int64_t m = h_select ? h_select[k] : k;
        SLAM_REQUIRE(m >= 0 && m < M, "%s: select[%lld] = %lld names no map point", who, (long long)k, (long long)m);
        const int64_t n = h_obs_offsets[m + 1] - h_obs_offsets[m];
        SLAM_REQUIRE(n >= 0 && h_obs_offsets[m] >= 0, "%s: the observation offsets descend at point %lld", who, (long long)m);
        SLAM_REQUIRE(n <= FP_OBS_MAX, "%s: point %lld has %lld observations (at most %d)", who, (long long)m, (long long)n, FP_OBS_MAX);
        SLAM_REQUIRE(h_obs_offsets[m + 1] < (1ll << 31), "%s: more than 2^31 observations", who);
        cls[(size_t)k] = n <= 16 ? 0 : (n <= 64 ? 1 : 2);
        cnt[cls[(size_t)k]]++;
    }
    at[0] = 0, at[1] = cnt[0], at[2] = cnt[0] + cnt[1];
    const int64_t first[3] = {at[0], at[1], at[2]};
    for (int64_t k = 0; k < K; k++) {
        const int64_t m = h_select ? h_select[k] : k;
        fz_job& jb = jobs[(size_t)at[cls[(size_t)k]]++];
        jb.start = h_obs_offsets[m];
        jb.m = (int)m;
        jb.n = (int)(h_obs_offsets[m + 1] - h_obs_offsets[m]);
        jb.out = (int)k;
        jb.pad = 0;
    }
    SLAM_REQUIRE(ctx, "%s: null ctx", who);
    if (K == 0) return SLAM_OK;
    SLAM_REQUIRE(d_best && d_desc_out && d_normal && d_range, "%s: null result pointer", who);
    bool any = false;
    for (const fz_job& jb : jobs) any |= jb.n > 0;
    SLAM_REQUIRE(!any || (d_xyz && d_obs && d_desc && d_level && d_centres), "%s: null device pointer", who);
    SLAM_REQUIRE(((uintptr_t)d_desc & 15) == 0 && ((uintptr_t)d_obs & 7) == 0 && ((uintptr_t)d_desc_out & 3) == 0, "%s: misaligned pointer", who);
    std::lock_guard<std::mutex> lk(ctx->call_mu);       // the job table, the frame offsets and the scale table
    SLAM_HIP(hipSetDevice(ctx->device));
    const uint64_t o_off = slam_align_up((uint64_t)K * sizeof(fz_job)), o_scale = o_off + slam_align_up((uint64_t)(B + 1) * 8);
    void* ws = nullptr;
    if (int rc = slam_workspace(ctx, o_scale + slam_align_up(FP_LEVELS_MAX * 8), &ws)) return rc;
    char* w = (char*)ws;
    SLAM_HIP(hipMemcpyAsync(w, jobs.data(), (size_t)K * sizeof(fz_job), hipMemcpyHostToDevice, ctx->stream));
    SLAM_HIP(hipMemcpyAsync(w + o_off, h_frame_offsets, (size_t)(B + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    SLAM_HIP(hipMemcpyAsync(w + o_scale, h_scale, (size_t)n_levels * 8, hipMemcpyHostToDevice, ctx->stream));
    // (the three copies read pageable memory: they have left the host arrays when they return)
    fz_refresh a;
    a.xyz = d_xyz;
    a.obs = (const int2*)d_obs;
    a.desc = (const uint4*)d_desc;
    a.inverse = d_inverse;
    a.level = d_level;
    a.frame_offsets = (const int64_t*)(w + o_off);
    a.centres = d_centres;
    a.ref = d_ref;
    a.scale = (const double*)(w + o_scale);
    a.B = (int)B;
    a.n_levels = n_levels;
    a.best = d_best;
    a.desc_out = (u32*)d_desc_out;
    a.normal = d_normal;
    a.range = d_range;
    const fz_job* d_jobs = (const fz_job*)w;
    if (int rc = slam_prof_begin(ctx)) return rc;
    if (cnt[0] > 0)
        fz_refresh_kernel<16><<<(unsigned)((cnt[0] + 15) / 16), FZ_REFRESH_THREADS, 0, ctx->stream>>>(a, d_jobs + first[0], (int)cnt[0]);
    if (cnt[1] > 0)
        fz_refresh_kernel<64><<<(unsigned)((cnt[1] + 3) / 4), FZ_REFRESH_THREADS, 0, ctx->stream>>>(a, d_jobs + first[1], (int)cnt[1]);
    if (cnt[2] > 0) fz_refresh_kernel<256><<<(unsigned)cnt[2], FZ_REFRESH_THREADS, 0, ctx->stream>>>(a, d_jobs + first[2], (int)cnt[2]);
    if (int rc = slam_prof_end(ctx)) return rc;
    return slam_launch_check("fuse refresh");
}
