// stereo.hip - stereo matching on gfx950: ORB-SLAM's Frame::ComputeStereoMatches for P pairs of images whose
// keypoints, descriptors and pyramids the ORB extractor left on the device.
//
//   slam_stereo_workspace   bytes of the caller-owned workspace (the level table and the pair table), no device needed
//   slam_stereo_match       two copies into that workspace and three launches, whatever P is:
//     stereo_search_kernel  one lane per left row; the right rows of the pair pass through LDS in tiles of 256 as (uR, band,
//                           level); a lane tests every one and takes the Hamming distance of those that pass all three gates
//     stereo_sad_kernel     one wave per left row that found a descriptor match: the left patch and the right strip once into
//                           LDS, the 2 Ls + 1 SADs from there (each lane a share of the pixels, summed over the wave), parabola
//                           and disparity on lane 0
//     stereo_median_kernel  one workgroup per pair: the SAD at index n / 2 by three 256-bin histogram passes in LDS (a radix
//                           select over 24 bits; SAD <= 961 * 510), then the rejection and the two counts
//
// The per-row arithmetic is stereo_point.h, which tests/stereo_twin.cpp builds for the host from the same text.  The result is a
// pure function of the arguments: atomics only count (histogram bins, kept rows), and the best candidate is the minimum of the
// packed key (distance << 16 | row) that a lane keeps for itself.  No entry point takes memory from the context.
#include "internal.h"
#include "stereo_point.h"
#include <math.h>

#define ST_LANES 256
#define ST_WAVES 4                                                      // rows per workgroup of the SAD kernel
#define ST_SIDE_MAX (2 * ST_HALF_MAX + 1)                               // 31
#define ST_PATCH_BYTES 976                                              // >= 31 * 31, a multiple of 16
#define ST_STRIP_BYTES 1904                                             // >= 31 * (31 + 30), a multiple of 16
#define ST_TABLE_BYTES 512                                              // the level table at the head of the workspace

struct st_table {                       // what the kernels read of the level layout: one copy in the workspace
    uint64_t base, stride;
    uint64_t off[SLAM_STEREO_MAX_LEVELS];
    int32_t pitch[SLAM_STEREO_MAX_LEVELS], w[SLAM_STEREO_MAX_LEVELS], h[SLAM_STEREO_MAX_LEVELS];
    float scale[SLAM_STEREO_MAX_LEVELS];
    int32_t L, pad;
};
static_assert(sizeof(st_table) <= ST_TABLE_BYTES, "the level table outgrew its place in the workspace");

struct st_block {                       // one extractor's outputs
    const int32_t* count;
    const int4* kp;
    const uint4* desc;
    const uint8_t* ws;
};

struct st_params {
    double bf, min_d, max_d;
    int th_orb, w, Ls, reject, n_max;
};

struct st_out {
    int32_t* right;
    double* u_right;
    double* depth;
    int32_t* orb_dist;
    int32_t* sad;
    uint8_t* status;
    int32_t* counts;
};

__device__ __forceinline__ int st_count(const int32_t* count, int b, int n_max) {
    const int n = count[b];
    return n < 0 ? 0 : n > n_max ? n_max : n;
}

// grid (ceil(n_max / 256), P).  Every slot of the pair gets all six outputs: status 1, 2 or ST_PENDING.
__global__ __launch_bounds__(ST_LANES) void stereo_search_kernel(const st_table* __restrict__ T, const int32_t* __restrict__ pairs, st_block Lb,
                                                                 st_block Rb, st_params prm, st_out o) {
    __shared__ double s_u[ST_LANES];
    __shared__ int s_lo[ST_LANES], s_hi[ST_LANES], s_lev[ST_LANES];
    __shared__ float s_scale[SLAM_STEREO_MAX_LEVELS];
    const int tid = (int)threadIdx.x, p = (int)blockIdx.y, i = (int)blockIdx.x * ST_LANES + tid;
    const int a = pairs[2 * p], b = pairs[2 * p + 1], L = T->L;
    const int nL = st_count(Lb.count, a, prm.n_max), nR = st_count(Rb.count, b, prm.n_max);
    if (tid < SLAM_STEREO_MAX_LEVELS) s_scale[tid] = tid < L ? T->scale[tid] : 1.0f;
    __syncthreads();

    bool live = i < nL;
    int lL = 0, tv = 0;
    double min_u = 0.0, max_u = 0.0;
    uint4 d0 = make_uint4(0, 0, 0, 0), d1 = d0;
    if (live) {
        const size_t row = (size_t)a * prm.n_max + i;
        const int4 k = Lb.kp[row];
        lL = k.z;
        if (lL < 0 || lL >= L) {
            live = false;
        } else {
            const float s = s_scale[lL];
            const double uL = st_level0(k.x, s), vL = st_level0(k.y, s);
            tv = (int)vL;
            min_u = uL - prm.max_d;
            max_u = uL - prm.min_d;
            if (max_u < 0.0) live = false;
            d0 = Lb.desc[2 * row];
            d1 = Lb.desc[2 * row + 1];
        }
    }
    unsigned best = 0xFFFFFFFFu;
    if ((int)blockIdx.x * ST_LANES < nL) {                               // (the same for the whole workgroup)
        for (int t0 = 0; t0 < nR; t0 += ST_LANES) {
            const int j = t0 + tid;
            int lev = -4, lo = 1, hi = 0;                                // a row that passes no gate
            double u = 0.0;
            if (j < nR) {
                const int4 k = Rb.kp[(size_t)b * prm.n_max + j];
                if (k.z >= 0 && k.z < L) {
                    const float s = s_scale[k.z];
                    lev = k.z;
                    u = st_level0(k.x, s);
                    st_band(st_level0(k.y, s), s, &lo, &hi);
                }
            }
            __syncthreads();                                             // the tile before this one has been read
            s_u[tid] = u;
            s_lo[tid] = lo;
            s_hi[tid] = hi;
            s_lev[tid] = lev;
            __syncthreads();
            if (live) {
                const int cnt = nR - t0 < ST_LANES ? nR - t0 : ST_LANES;
                for (int jj = 0; jj < cnt; jj++) {
                    if (!st_candidate(tv, lL, min_u, max_u, s_lo[jj], s_hi[jj], s_lev[jj], s_u[jj])) continue;
                    const size_t row = (size_t)b * prm.n_max + t0 + jj;
                    const uint4 r0 = Rb.desc[2 * row], r1 = Rb.desc[2 * row + 1];
                    const int d = __popc(d0.x ^ r0.x) + __popc(d0.y ^ r0.y) + __popc(d0.z ^ r0.z) + __popc(d0.w ^ r0.w) + __popc(d1.x ^ r1.x) +
                                  __popc(d1.y ^ r1.y) + __popc(d1.z ^ r1.z) + __popc(d1.w ^ r1.w);
                    const unsigned key = ((unsigned)d << 16) | (unsigned)(t0 + jj);
                    best = key < best ? key : best;                      // smallest (distance, row): strict < over ascending rows
                }
            }
        }
    }
    if (i >= prm.n_max) return;
    const size_t slot = (size_t)p * prm.n_max + i;
    const bool found = best != 0xFFFFFFFFu;
    const int dist = found ? (int)(best >> 16) : ST_NO_DIST;
    o.right[slot] = found ? (int)(best & 0xFFFFu) : -1;
    o.orb_dist[slot] = dist;
    o.u_right[slot] = st_nan();
    o.depth[slot] = st_nan();
    o.sad[slot] = -1;
    o.status[slot] = (uint8_t)(!found ? ST_NO_CANDIDATE : dist >= prm.th_orb ? ST_ORB_DISTANCE : ST_PENDING);
}

// grid (ceil(n_max / 4), P), one wave per slot.  A pending row leaves with status 0, 3, 4 or 5.
__global__ __launch_bounds__(ST_LANES) void stereo_sad_kernel(const st_table* __restrict__ T, const int32_t* __restrict__ pairs, st_block Lb,
                                                              st_block Rb, st_params prm, st_out o) {
    __shared__ uint8_t s_patch[ST_WAVES][ST_PATCH_BYTES];
    __shared__ uint8_t s_strip[ST_WAVES][ST_STRIP_BYTES];
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63, p = (int)blockIdx.y, i = (int)blockIdx.x * ST_WAVES + wave;
    const int a = pairs[2 * p], b = pairs[2 * p + 1];
    const int nL = st_count(Lb.count, a, prm.n_max);
    if ((int)blockIdx.x * ST_WAVES >= nL) return;                        // (the whole workgroup)
    const size_t slot = (size_t)p * prm.n_max + (i < prm.n_max ? i : 0);
    bool live = i < nL && o.status[slot] == ST_PENDING;                  // (the same in every lane of the wave)
    const int w = prm.w, Ls = prm.Ls, side = 2 * w + 1, sw = side + 2 * Ls;
    int x = 0, y = 0, c0 = 0;
    float sL = 1.0f;
    double uL = 0.0;
    if (live) {
        const int4 kl = Lb.kp[(size_t)a * prm.n_max + i];
        const int4 kr = Rb.kp[(size_t)b * prm.n_max + o.right[slot]];
        const int lL = kl.z;                                             // in [0, L): the search left the row pending
        x = kl.x;
        y = kl.y;
        sL = T->scale[lL];
        uL = st_level0(x, sL);
        c0 = st_c0(st_level0(kr.x, T->scale[kr.z]), sL);
        if (!st_window_ok(x, y, c0, w, Ls, T->w[lL], T->h[lL])) {
            live = false;
            if (lane == 0) o.status[slot] = ST_WINDOW;
        } else {
            const ptrdiff_t pitch = T->pitch[lL];
            const uint8_t* il = Lb.ws + T->base + (uint64_t)a * T->stride + T->off[lL] + (ptrdiff_t)(y - w) * pitch;
            const uint8_t* ir = Rb.ws + T->base + (uint64_t)b * T->stride + T->off[lL] + (ptrdiff_t)(y - w) * pitch;
            for (int q = lane; q < side * side; q += 64) s_patch[wave][q] = il[(q / side) * pitch + (x - w) + q % side];
            for (int q = lane; q < side * sw; q += 64) s_strip[wave][q] = ir[(q / sw) * pitch + (c0 - Ls - w) + q % sw];
        }
    }
    __syncthreads();
    if (!live) return;
    const uint8_t* pl = &s_patch[wave][w * side + w];
    const uint8_t* pr = &s_strip[wave][w * sw + Ls + w];
    st_slide sl = st_slide_start();
    for (int inc = -Ls; inc <= Ls; inc++) {
        int s = st_sad(pl, side, pr + inc, sw, w, lane, 64);
        for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
        st_slide_push(&sl, inc, s);
    }
    if (lane != 0) return;
    o.sad[slot] = sl.best;
    if (sl.inc == -Ls || sl.inc == Ls) {
        o.status[slot] = ST_SLIDE_BORDER;
        return;
    }
    const st_depth r = st_disparity(uL, sL, c0, sl.inc, st_parabola(sl.d1, sl.best, sl.d3), prm.bf, prm.min_d, prm.max_d);
    o.u_right[slot] = r.u_right;
    o.depth[slot] = r.depth;
    o.status[slot] = (uint8_t)r.status;
}

// grid P.  m = the SAD at index n / 2 of the accepted rows in ascending order; rows with 10 SAD >= 21 m get status 6.
__global__ __launch_bounds__(ST_LANES) void stereo_median_kernel(const int32_t* __restrict__ pairs, st_block Lb, st_params prm, st_out o) {
    __shared__ int s_hist[256];
    __shared__ int s_prefix, s_k, s_n, s_kept;
    const int tid = (int)threadIdx.x, p = (int)blockIdx.x;
    const int nL = st_count(Lb.count, pairs[2 * p], prm.n_max);
    const size_t base = (size_t)p * prm.n_max;
    if (tid == 0) s_prefix = s_k = s_n = s_kept = 0;
    for (int pass = 0; pass < 3; pass++) {
        const int shift = 16 - 8 * pass;
        const int high = pass == 0 ? 0 : (0xFFFFFF >> (shift + 8)) << (shift + 8);      // the bits the passes before have fixed
        s_hist[tid] = 0;
        __syncthreads();
        const int prefix = s_prefix;
        for (int i = tid; i < nL; i += ST_LANES)
            if (o.status[base + i] == ST_MATCHED) {
                const int s = o.sad[base + i];
                if ((s & high) == prefix) atomicAdd(&s_hist[(s >> shift) & 255], 1);
            }
        __syncthreads();
        if (tid == 0) {
            int k = s_k;
            if (pass == 0) {
                int n = 0;
                for (int q = 0; q < 256; q++) n += s_hist[q];
                s_n = n;
                k = n / 2;
            }
            if (s_n > 0) {
                int q = 0;
                while (q < 255 && k >= s_hist[q]) k -= s_hist[q++];
                s_prefix = prefix | (q << shift);
                s_k = k;
            }
        }
        __syncthreads();
    }
    const int n = s_n, m = s_prefix;
    int kept = 0;
    if (prm.reject && n > 0) {
        for (int i = tid; i < nL; i += ST_LANES)
            if (o.status[base + i] == ST_MATCHED) {
                if (st_median_keeps(o.sad[base + i], m)) {
                    kept++;
                } else {
                    o.status[base + i] = ST_MEDIAN;
                    o.u_right[base + i] = st_nan();
                    o.depth[base + i] = st_nan();
                }
            }
        if (kept) atomicAdd(&s_kept, kept);
        __syncthreads();
        kept = s_kept;
    } else {
        kept = n;
    }
    if (tid == 0) {
        o.counts[2 * p] = kept;
        o.counts[2 * p + 1] = n;
    }
}

// ================================================================= entry points ==============================================
extern "C" int slam_stereo_workspace(int64_t P, int64_t n_max, uint64_t* bytes) {
    SLAM_REQUIRE(bytes, "slam_stereo_workspace: null bytes");
    SLAM_REQUIRE(P >= 0 && P <= SLAM_STEREO_MAX_PAIRS && n_max >= 0 && n_max <= SLAM_STEREO_MAX_ROWS,
                 "slam_stereo_workspace: bad sizes (P=%lld in [0, %d], n_max=%lld in [0, %d])", (long long)P, SLAM_STEREO_MAX_PAIRS, (long long)n_max,
                 SLAM_STEREO_MAX_ROWS);
    *bytes = ST_TABLE_BYTES + (((uint64_t)P * 8 + 15) & ~(uint64_t)15) + 16;
    return SLAM_OK;
}

static bool st_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

extern "C" int slam_stereo_match(slam_ctx* ctx, int64_t P, const int32_t* h_pairs, int64_t B_left, const int32_t* d_count_left, const int32_t* d_kp_left,
                                 const uint8_t* d_desc_left, const void* d_ws_left, int64_t B_right, const int32_t* d_count_right,
                                 const int32_t* d_kp_right, const uint8_t* d_desc_right, const void* d_ws_right, int64_t n_max, int L,
                                 uint64_t image_base, uint64_t image_stride, const uint64_t* h_level_offset, const int32_t* h_level_pitch,
                                 const int32_t* h_level_w, const int32_t* h_level_h, const float* h_scale, double bf, double min_d, double max_d,
                                 int th_orb, int w, int Ls, int reject, void* d_workspace, uint64_t workspace_bytes, int32_t* d_right,
                                 double* d_u_right, double* d_depth, int32_t* d_orb_dist, int32_t* d_sad, uint8_t* d_status, int32_t* d_counts) {
    SLAM_REQUIRE(ctx, "slam_stereo_match: null ctx");
    SLAM_REQUIRE(P >= 0 && P <= SLAM_STEREO_MAX_PAIRS, "slam_stereo_match: P=%lld must be in [0, %d]", (long long)P, SLAM_STEREO_MAX_PAIRS);
    SLAM_REQUIRE(n_max >= 0 && n_max <= SLAM_STEREO_MAX_ROWS, "slam_stereo_match: n_max=%lld must be in [0, %d]", (long long)n_max, SLAM_STEREO_MAX_ROWS);
    SLAM_REQUIRE(L >= 1 && L <= SLAM_STEREO_MAX_LEVELS, "slam_stereo_match: L=%d must be in [1, %d]", L, SLAM_STEREO_MAX_LEVELS);
    SLAM_REQUIRE(B_left >= 0 && B_left <= 65535 && B_right >= 0 && B_right <= 65535, "slam_stereo_match: a block of %lld / %lld images (at most 65535)",
                 (long long)B_left, (long long)B_right);
    SLAM_REQUIRE(th_orb >= 0 && th_orb <= 256, "slam_stereo_match: th_orb=%d must be in [0, 256]", th_orb);
    SLAM_REQUIRE(w >= 1 && w <= ST_HALF_MAX && Ls >= 1 && Ls <= ST_HALF_MAX, "slam_stereo_match: w=%d and Ls=%d must be in [1, %d]", w, Ls, ST_HALF_MAX);
    SLAM_REQUIRE(bf > 0.0 && bf <= 1.7976931348623157e308, "slam_stereo_match: bf must be positive and finite");
    SLAM_REQUIRE(fabs(min_d) <= 1.7976931348623157e308, "slam_stereo_match: min_d must be finite");
    SLAM_REQUIRE(max_d > min_d, "slam_stereo_match: max_d must be above min_d");
    SLAM_REQUIRE(h_level_offset && h_level_pitch && h_level_w && h_level_h && h_scale, "slam_stereo_match: null host pointer (level layout)");
    SLAM_REQUIRE(P == 0 || h_pairs, "slam_stereo_match: null host pointer (h_pairs)");
    st_table T;
    memset(&T, 0, sizeof(T));
    T.base = image_base;
    T.stride = image_stride;
    T.L = L;
    SLAM_REQUIRE(image_base <= ((uint64_t)1 << 40) && image_stride <= ((uint64_t)1 << 40), "slam_stereo_match: image base or stride above 2^40");
    for (int l = 0; l < L; l++) {
        SLAM_REQUIRE(h_level_w[l] >= 1 && h_level_h[l] >= 1 && h_level_w[l] <= SLAM_STEREO_MAX_SIDE && h_level_h[l] <= SLAM_STEREO_MAX_SIDE,
                     "slam_stereo_match: level %d is %d x %d (sides in [1, %d])", l, h_level_w[l], h_level_h[l], SLAM_STEREO_MAX_SIDE);
        SLAM_REQUIRE(h_level_pitch[l] >= h_level_w[l] && h_level_pitch[l] <= (1 << 20), "slam_stereo_match: the pitch of level %d is below its width (or above 2^20)", l);
        SLAM_REQUIRE(h_level_offset[l] <= ((uint64_t)1 << 40), "slam_stereo_match: the offset of level %d is above 2^40", l);
        SLAM_REQUIRE(h_scale[l] >= 1.0f && h_scale[l] <= 65536.0f, "slam_stereo_match: h_scale[%d] must be in [1, 65536]", l);
        T.off[l] = h_level_offset[l];
        T.pitch[l] = h_level_pitch[l];
        T.w[l] = h_level_w[l];
        T.h[l] = h_level_h[l];
        T.scale[l] = h_scale[l];
    }
    for (int64_t p = 0; p < P; p++)
        SLAM_REQUIRE(h_pairs[2 * p] >= 0 && h_pairs[2 * p] < B_left && h_pairs[2 * p + 1] >= 0 && h_pairs[2 * p + 1] < B_right,
                     "slam_stereo_match: pair %lld = (%d, %d) is outside its blocks of %lld and %lld images", (long long)p, h_pairs[2 * p],
                     h_pairs[2 * p + 1], (long long)B_left, (long long)B_right);
    if (P == 0 || n_max == 0) return SLAM_OK;
    uint64_t need = 0;
    slam_stereo_workspace(P, n_max, &need);
    SLAM_REQUIRE(d_workspace && st_aligned(d_workspace, 16) && workspace_bytes >= need,
                 "slam_stereo_match: the workspace must be a 16-byte aligned device pointer of at least %llu bytes (got %llu)", (unsigned long long)need,
                 (unsigned long long)workspace_bytes);
    SLAM_REQUIRE(d_count_left && d_kp_left && d_desc_left && d_ws_left && d_count_right && d_kp_right && d_desc_right && d_ws_right,
                 "slam_stereo_match: null device pointer (a block)");
    SLAM_REQUIRE(st_aligned(d_kp_left, 16) && st_aligned(d_kp_right, 16) && st_aligned(d_desc_left, 16) && st_aligned(d_desc_right, 16),
                 "slam_stereo_match: d_kp and d_desc must be aligned to 16 bytes");
    SLAM_REQUIRE(d_right && d_u_right && d_depth && d_orb_dist && d_sad && d_status && d_counts, "slam_stereo_match: null device pointer (an output)");
    SLAM_REQUIRE(st_aligned(d_u_right, 8) && st_aligned(d_depth, 8) && st_aligned(d_right, 4) && st_aligned(d_orb_dist, 4) && st_aligned(d_sad, 4) &&
                     st_aligned(d_counts, 4),
                 "slam_stereo_match: an output is misaligned");
    SLAM_HIP(hipSetDevice(ctx->device));
    uint8_t* ws = (uint8_t*)d_workspace;
    const st_table* d_T = (const st_table*)ws;
    const int32_t* d_pairs = (const int32_t*)(ws + ST_TABLE_BYTES);
    SLAM_HIP(hipMemcpyAsync(ws, &T, sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    SLAM_HIP(hipMemcpyAsync(ws + ST_TABLE_BYTES, h_pairs, (size_t)P * 8, hipMemcpyHostToDevice, ctx->stream));
    const st_block Lb = {d_count_left, (const int4*)d_kp_left, (const uint4*)d_desc_left, (const uint8_t*)d_ws_left};
    const st_block Rb = {d_count_right, (const int4*)d_kp_right, (const uint4*)d_desc_right, (const uint8_t*)d_ws_right};
    const st_params prm = {bf, min_d, max_d, th_orb, w, Ls, reject ? 1 : 0, (int)n_max};
    const st_out o = {d_right, d_u_right, d_depth, d_orb_dist, d_sad, d_status, d_counts};
    stereo_search_kernel<<<dim3((unsigned)((n_max + ST_LANES - 1) / ST_LANES), (unsigned)P), ST_LANES, 0, ctx->stream>>>(d_T, d_pairs, Lb, Rb, prm, o);
    SLAM_HIP(hipGetLastError());
    stereo_sad_kernel<<<dim3((unsigned)((n_max + ST_WAVES - 1) / ST_WAVES), (unsigned)P), ST_LANES, 0, ctx->stream>>>(d_T, d_pairs, Lb, Rb, prm, o);
    SLAM_HIP(hipGetLastError());
    stereo_median_kernel<<<(unsigned)P, ST_LANES, 0, ctx->stream>>>(d_pairs, Lb, prm, o);
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}
