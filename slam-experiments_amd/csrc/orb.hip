// orb.hip — batched ORB feature extraction (slam_orb_*): what the reference gets from cv2.ORB behind OrbFeatureDetector
// (feature_detectors.py:18-26), called per frame from Frontend._detect_features (frontend.py:245).
//
// The specification is DESIGN.md §4d: every step is integer arithmetic, so the result is a pure function of the inputs and is
// checked bit for bit against a numpy restatement.  PARITY UNPINNED against cv2.ORB (absent here; its learned pattern is not shipped).
//
// Four launches per call, whatever the batch size B and the number of levels L; each runs over (image, level, tile) or
// (image, level) or (image, slot) work items found from blockIdx and a level table passed by value:
//   1 orb_pyramid_kernel   level image (bilinear from level 0, 16.16 coordinates, 11-bit weights) and its 7x7 binomial blur from one
//                          LDS tile with a 3-pixel halo; rows are written as aligned dwords (the workspace pitch is a multiple of 4)
//   2 orb_fast_kernel      tile + 4-pixel halo staged in LDS by aligned dword loads; FAST-9/16 score, score map, strict 3x3
//                          non-maximum suppression, then one wave per survivor: Harris R from the same LDS tile, the mask, and an
//                          atomic append to the level's candidate list (capacity: one survivor per 2x2 block, which NMS guarantees)
//   3 orb_select_kernel    one block per (image, level): radix select of the quota-th key under (R desc, y asc, x asc) when the list
//                          is longer than the quota, then a rank by counting among the kept ones: the order of the append drops out
//   4 orb_describe_kernel  one wave per output slot: moments over the radius-15 disc, the 32-way bin by cross-product signs,
//                          256 steered comparisons on the blurred level gathered with four ballots; unused slots are zeroed
// slam_orb_extract_dist_u8 runs the same four launches with orb_distribute_kernel in the place of 3: FAST at the
// lower of two thresholds, candidates of cells without a strong corner kept, and the quota spread over the level by a quadtree.
#include "internal.h"

#define ORB_BORDER 16
#define ORB_TW 64
#define ORB_TH 16
#define ORB_THREADS 256
#define ORB_SEL_THREADS 1024

struct orb_plan {
    int L, W, H, n_max;
    int w[SLAM_ORB_MAX_LEVELS], h[SLAM_ORB_MAX_LEVELS], pitch[SLAM_ORB_MAX_LEVELS], tiles_x[SLAM_ORB_MAX_LEVELS];
    int cap[SLAM_ORB_MAX_LEVELS], quota[SLAM_ORB_MAX_LEVELS], tile0[SLAM_ORB_MAX_LEVELS + 1];
    unsigned long long img[SLAM_ORB_MAX_LEVELS], blur[SLAM_ORB_MAX_LEVELS], score[SLAM_ORB_MAX_LEVELS], cand[SLAM_ORB_MAX_LEVELS];
    unsigned long long counts_off, sel_off, image_base, image_stride;
};

struct orb_cand {           // 16 bytes: one FAST survivor of a level
    long long R;            // Harris response
    unsigned int xy;        // x | y << 16 (level coordinates)
    unsigned int pad;
};

struct orb_dist {           // what the quadtree selection adds to the plan (offsets inside an image block)
    int t_ini, adaptive;    // the upper threshold; whether the lower one differs from it
    int n_ini[SLAM_ORB_MAX_LEVELS], node_cap[SLAM_ORB_MAX_LEVELS];
    unsigned long long cn[SLAM_ORB_MAX_LEVELS], node[SLAM_ORB_MAX_LEVELS], fin[SLAM_ORB_MAX_LEVELS];
};

struct orb_node {           // 64 bytes: one cell of a level's quadtree, [x0, x1) x [y0, y1) in level coordinates
    unsigned long long best;    // the best R among its live candidates, sign bit flipped (atomicMax)
    unsigned bxy;               // x | y << 16 of the first candidate with that R (atomicMin)
    int count;                  // live candidates inside
    short x0, y0, x1, y1;
    int gain, split;            // this round: non-empty children - 1 (-1: not splittable); whether it is being split
    int cc[4], cm[4];           // this round: live candidates per child; the slot each non-empty child takes
};

static inline uint64_t orb_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

// Sizes, offsets and the tile table of one call.  Nothing here touches the device.
static int orb_make_plan(const char* who, int64_t B, int64_t H, int64_t W, int L, const int32_t* h_lw, const int32_t* h_lh, int64_t n_max,
                         orb_plan& P, uint64_t& total) {
    SLAM_REQUIRE(B >= 0 && B <= SLAM_ORB_MAX_BATCH, "%s: B=%lld out of range [0, %d]", who, (long long)B, SLAM_ORB_MAX_BATCH);
    SLAM_REQUIRE(H >= 1 && H <= SLAM_ORB_MAX_SIDE && W >= 1 && W <= SLAM_ORB_MAX_SIDE, "%s: image %lld x %lld out of range [1, %d]", who,
                 (long long)W, (long long)H, SLAM_ORB_MAX_SIDE);
    SLAM_REQUIRE(L >= 1 && L <= SLAM_ORB_MAX_LEVELS, "%s: L=%d out of range [1, %d]", who, L, SLAM_ORB_MAX_LEVELS);
    SLAM_REQUIRE(h_lw && h_lh, "%s: null level size array", who);
    SLAM_REQUIRE(n_max >= 0 && n_max <= SLAM_ORB_MAX_FEATURES, "%s: quota sum %lld out of range [0, %d]", who, (long long)n_max,
                 SLAM_ORB_MAX_FEATURES);
    SLAM_REQUIRE(B * (n_max > 0 ? n_max : 1) <= (1ll << 28), "%s: B * quota sum above 2^28", who);
    SLAM_REQUIRE(h_lw[0] == W && h_lh[0] == H, "%s: level 0 must have the size of the input", who);
    memset(&P, 0, sizeof(P));
    P.L = L; P.W = (int)W; P.H = (int)H; P.n_max = (int)n_max;
    uint64_t off = 0;
    for (int l = 0; l < L; l++) {
        SLAM_REQUIRE(h_lw[l] >= 1 && h_lh[l] >= 1 && (l == 0 || (h_lw[l] <= h_lw[l - 1] && h_lh[l] <= h_lh[l - 1])),
                     "%s: level %d size %d x %d is not in [1, size of the level before]", who, l, h_lw[l], h_lh[l]);
        const int w = h_lw[l], h = h_lh[l];
        P.w[l] = w; P.h[l] = h; P.pitch[l] = (w + 3) & ~3;
        P.tiles_x[l] = (w + ORB_TW - 1) / ORB_TW;
        P.tile0[l + 1] = P.tile0[l] + P.tiles_x[l] * ((h + ORB_TH - 1) / ORB_TH);
        const bool live = w >= 2 * ORB_BORDER + 1 && h >= 2 * ORB_BORDER + 1;
        P.cap[l] = live ? ((w - 2 * ORB_BORDER + 1) / 2) * ((h - 2 * ORB_BORDER + 1) / 2) : 0;
        const uint64_t plane = orb_up((uint64_t)P.pitch[l] * h, 16);
        P.img[l] = off; off += plane;
        P.blur[l] = off; off += plane;
        P.score[l] = off; off += plane;
        P.cand[l] = off; off += (uint64_t)P.cap[l] * sizeof(orb_cand);
    }
    P.image_stride = orb_up(off, 256);
    P.counts_off = 0;
    P.sel_off = orb_up((uint64_t)(B > 0 ? B : 1) * SLAM_ORB_MAX_LEVELS * 4, 256);
    P.image_base = P.sel_off + orb_up((uint64_t)(B > 0 ? B : 1) * (uint64_t)(n_max > 0 ? n_max : 1) * sizeof(orb_cand), 256);
    total = P.image_base + (uint64_t)(B > 0 ? B : 1) * P.image_stride;
    return SLAM_OK;
}

// ------------------------------------------------------------------------------------------------------------ device helpers
__device__ __forceinline__ int orb_level_of(const orb_plan& P, int item) {
    int l = 0;
    while (l + 1 < P.L && item >= P.tile0[l + 1]) l++;
    return l;
}

// pixel-centre source coordinate of destination index i (level -> level 0), 16.16, clamped: left tap, right tap, 11-bit weight
__device__ __forceinline__ int3 orb_axis_map(int i, int n_dst, int n_src) {
    long long f = ((long long)(2 * i + 1) * n_src * 32768) / n_dst - 32768;
    const long long top = (long long)(n_src - 1) << 16;
    f = f < 0 ? 0 : (f > top ? top : f);
    const int i0 = (int)(f >> 16);
    return make_int3(i0, i0 + 1 < n_src ? i0 + 1 : n_src - 1, (int)((f & 0xFFFF) >> 5));
}

__device__ __forceinline__ int orb_wave_sum(int v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

// 9 contiguous set bits on a circle of 16: duplicate to 32 bits, AND shifted copies (1, 2, 4, 1)
__device__ __forceinline__ unsigned orb_arc9(unsigned m16) {
    unsigned m = m16 | (m16 << 16);
    m &= m >> 1;
    m &= m >> 2;
    m &= m >> 4;
    m &= m >> 1;
    return m & 0xFFFFu;
}

__device__ __forceinline__ bool orb_fast_pass(const int (&ring)[16], int p, int th) {
    unsigned brighter = 0, darker = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        brighter |= (unsigned)(ring[i] > p + th) << i;
        darker |= (unsigned)(ring[i] < p - th) << i;
    }
    return (orb_arc9(brighter) | orb_arc9(darker)) != 0;
}

// ------------------------------------------------------------------------------------------------ 1: pyramid level + blur
__global__ __launch_bounds__(ORB_THREADS) void orb_pyramid_kernel(orb_plan P, const uint8_t* __restrict__ images, uint8_t* __restrict__ ws) {
    constexpr int PW = ORB_TW + 6, PH = ORB_TH + 6, PP = ORB_TW + 8;     // 70 x 22 pixels, LDS pitch 72
    __shared__ uint8_t s_px[PH * PP];
    __shared__ unsigned short s_hor[PH * ORB_TW];
    __shared__ int3 s_xmap[PW], s_ymap[PH];
    const int tid = threadIdx.x, b = blockIdx.y, item = blockIdx.x;
    const int l = orb_level_of(P, item);
    const int t = item - P.tile0[l], tx = t % P.tiles_x[l], ty = t / P.tiles_x[l];
    const int w = P.w[l], h = P.h[l], pitch = P.pitch[l], x0 = tx * ORB_TW, y0 = ty * ORB_TH;
    if (t == 0 && tid == 0) ((int*)(ws + P.counts_off))[b * SLAM_ORB_MAX_LEVELS + l] = 0;      // the candidate count of this (image, level)
    if (tid < PW) {
        int c = x0 - 3 + tid;
        c = c < 0 ? 0 : (c > w - 1 ? w - 1 : c);                        // replicate border of the blur = clamped level coordinate
        s_xmap[tid] = orb_axis_map(c, w, P.W);
    } else if (tid >= 128 && tid < 128 + PH) {
        int r = y0 - 3 + (tid - 128);
        r = r < 0 ? 0 : (r > h - 1 ? h - 1 : r);
        s_ymap[tid - 128] = orb_axis_map(r, h, P.H);
    }
    __syncthreads();
    const uint8_t* src = images + (size_t)b * P.H * P.W;
    for (int i = tid; i < PH * PW; i += ORB_THREADS) {
        const int r = i / PW, c = i - r * PW;
        const int3 my = s_ymap[r], mx = s_xmap[c];
        const uint8_t* r0 = src + (size_t)my.x * P.W;
        const uint8_t* r1 = src + (size_t)my.y * P.W;
        const int top = r0[mx.x] * (2048 - mx.z) + r0[mx.y] * mx.z;     // level 0 maps to itself with weight 0
        const int bot = r1[mx.x] * (2048 - mx.z) + r1[mx.y] * mx.z;
        s_px[r * PP + c] = (uint8_t)((top * (2048 - my.z) + bot * my.z + (1 << 21)) >> 22);
    }
    __syncthreads();
    uint8_t* base = ws + P.image_base + (size_t)b * P.image_stride;
    const int row = tid >> 4, col = (tid & 15) * 4, gx = x0 + col, gy = y0 + row;
    const bool store = gy < h && gx < pitch;                             // gx and pitch are multiples of 4: whole dwords stay in the row
    if (store) {
        unsigned v = 0;
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (gx + k < w) v |= (unsigned)s_px[(row + 3) * PP + col + 3 + k] << (8 * k);
        *(unsigned*)(base + P.img[l] + (size_t)gy * pitch + gx) = v;
    }
    for (int i = tid; i < PH * ORB_TW; i += ORB_THREADS) {
        const int r = i / ORB_TW, c = i - r * ORB_TW;
        const uint8_t* p = s_px + r * PP + c;
        s_hor[i] = (unsigned short)(p[0] + p[6] + 6 * (p[1] + p[5]) + 15 * (p[2] + p[4]) + 20 * p[3]);
    }
    __syncthreads();
    if (store) {
        unsigned v = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned short* p = s_hor + row * ORB_TW + col + k;
            const int s = p[0] + p[6 * ORB_TW] + 6 * (p[ORB_TW] + p[5 * ORB_TW]) + 15 * (p[2 * ORB_TW] + p[4 * ORB_TW]) + 20 * p[3 * ORB_TW];
            if (gx + k < w) v |= (unsigned)((s + 2048) >> 12) << (8 * k);
        }
        *(unsigned*)(base + P.blur[l] + (size_t)gy * pitch + gx) = v;
    }
}

// ------------------------------------------------------------------------- 2: FAST score, NMS, Harris, candidate append
__global__ __launch_bounds__(ORB_THREADS) void orb_fast_kernel(orb_plan P, const uint8_t* __restrict__ mask, unsigned long long mask_stride,
                                                               int threshold, uint8_t* __restrict__ ws) {
    constexpr int PP = ORB_TW + 8, PH = ORB_TH + 8, SW = ORB_TW + 2, SH = ORB_TH + 2, SP = ORB_TW + 4;   // pixels 72 x 24, scores 66 x 18
    __shared__ unsigned s_pxw[PH * PP / 4];
    __shared__ uint8_t s_sc[SH * SP];
    __shared__ unsigned s_list[ORB_THREADS];
    __shared__ int s_n;
    const uint8_t* s_px = (const uint8_t*)s_pxw;
    const int tid = threadIdx.x, b = blockIdx.y, item = blockIdx.x;
    const int l = orb_level_of(P, item);
    const int t = item - P.tile0[l], tx = t % P.tiles_x[l], ty = t / P.tiles_x[l];
    const int w = P.w[l], h = P.h[l], pitch = P.pitch[l], x0 = tx * ORB_TW, y0 = ty * ORB_TH;
    uint8_t* base = ws + P.image_base + (size_t)b * P.image_stride;
    const uint8_t* img = base + P.img[l];
    if (tid == 0) s_n = 0;
    for (int i = tid; i < PH * (PP / 4); i += ORB_THREADS) {             // x0 - 4 is a multiple of 4 and so is the pitch: aligned dwords
        const int r = i / (PP / 4), c4 = i - r * (PP / 4);
        const int gx = x0 - 4 + 4 * c4, gy = y0 - 4 + r;
        s_pxw[i] = (gy >= 0 && gy < h && gx >= 0 && gx < pitch) ? *(const unsigned*)(img + (size_t)gy * pitch + gx) : 0u;
    }
    __syncthreads();
    for (int i = tid; i < SH * SW; i += ORB_THREADS) {
        const int r = i / SW, c = i - r * SW;
        const int gx = x0 - 1 + c, gy = y0 - 1 + r;
        int score = 0;
        if (gx >= ORB_BORDER && gx < w - ORB_BORDER && gy >= ORB_BORDER && gy < h - ORB_BORDER) {
            const uint8_t* q = s_px + (r + 3) * PP + (c + 3);            // the pixel itself; LDS origin is (x0 - 4, y0 - 4)
            const int p = q[0];
            const int ring[16] = {q[-3 * PP], q[-3 * PP + 1], q[-2 * PP + 2], q[-PP + 3], q[3], q[PP + 3], q[2 * PP + 2], q[3 * PP + 1],
                                  q[3 * PP], q[3 * PP - 1], q[2 * PP - 2], q[PP - 3], q[-3], q[-PP - 3], q[-2 * PP - 2], q[-3 * PP - 1]};
            if (orb_fast_pass(ring, p, threshold)) {
                int lo = threshold, hi = 255;                            // the largest threshold that still passes: the test is monotone
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (orb_fast_pass(ring, p, mid)) lo = mid; else hi = mid - 1;
                }
                score = lo;
            }
        }
        s_sc[r * SP + c] = (uint8_t)score;
    }
    __syncthreads();
    const int row = tid >> 4, col = (tid & 15) * 4, gx = x0 + col, gy = y0 + row;
    if (gy < h && gx < pitch) {
        unsigned v = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint8_t* c = s_sc + (row + 1) * SP + col + 1 + k;
            const int s = c[0];
            v |= (unsigned)s << (8 * k);
            if (s > 0 && s > c[-1] && s > c[1] && s > c[-SP - 1] && s > c[-SP] && s > c[-SP + 1] && s > c[SP - 1] && s > c[SP] && s > c[SP + 1]) {
                const int at = atomicAdd(&s_n, 1);
                if (at < ORB_THREADS) s_list[at] = (unsigned)(gx + k) | ((unsigned)gy << 16);
            }
        }
        *(unsigned*)(base + P.score[l] + (size_t)gy * pitch + gx) = v;   // pixels at and past w are outside the scored region: 0
    }
    __syncthreads();
    const int n = s_n < ORB_THREADS ? s_n : ORB_THREADS, lane = tid & 63;
    for (int s = tid >> 6; s < n; s += ORB_THREADS / 64) {              // one wave per survivor
        const unsigned xy = s_list[s];
        const int x = (int)(xy & 0xFFFF), y = (int)(xy >> 16);
        int a = 0, bb = 0, c = 0;
        if (lane < 49) {
            const int dy = lane / 7 - 3, dx = lane - (lane / 7) * 7 - 3;
            const uint8_t* q = s_px + (y - y0 + 4 + dy) * PP + (x - x0 + 4 + dx);
            const int ix = (q[-PP + 1] + 2 * q[1] + q[PP + 1]) - (q[-PP - 1] + 2 * q[-1] + q[PP - 1]);
            const int iy = (q[PP - 1] + 2 * q[PP] + q[PP + 1]) - (q[-PP - 1] + 2 * q[-PP] + q[-PP + 1]);
            a = ix * ix; bb = ix * iy; c = iy * iy;
        }
        a = orb_wave_sum(a); bb = orb_wave_sum(bb); c = orb_wave_sum(c);
        if (lane == 0) {
            bool allowed = true;
            if (mask) {
                long long mx = (2ll * x * P.W + w) / (2ll * w), my = (2ll * y * P.H + h) / (2ll * h);
                mx = mx > P.W - 1 ? P.W - 1 : mx;
                my = my > P.H - 1 ? P.H - 1 : my;
                allowed = mask[(size_t)b * mask_stride + (size_t)my * P.W + mx] != 0;
            }
            if (allowed) {
                const long long A = a, Bq = bb, C = c;
                const int at = atomicAdd((int*)(ws + P.counts_off) + b * SLAM_ORB_MAX_LEVELS + l, 1);
                if (at < P.cap[l]) {
                    orb_cand* out = (orb_cand*)(base + P.cand[l]) + at;
                    out->R = 25 * (A * C - Bq * Bq) - (A + C) * (A + C);
                    out->xy = xy;
                    out->pad = 0;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------- 3: the best quota[l] of each (image, level)
struct orb_key { unsigned long long hi; unsigned lo; };                 // ascending key order = (R descending, y ascending, x ascending)
__device__ __forceinline__ orb_key orb_key_of(const orb_cand& c) { return {~((unsigned long long)c.R ^ (1ull << 63)), c.xy}; }
__device__ __forceinline__ bool orb_key_less(const orb_key& a, const orb_key& b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
__device__ __forceinline__ unsigned orb_key_digit(const orb_key& k, int d) {          // digit 0 is the most significant of 12
    return d < 8 ? (unsigned)(k.hi >> (56 - 8 * d)) & 255u : (k.lo >> (24 - 8 * (d - 8))) & 255u;
}
__device__ __forceinline__ bool orb_key_has_prefix(const orb_key& k, const orb_key& p, int d) {   // the first d digits agree
    if (d == 0) return true;
    if (d <= 8) return (k.hi >> (64 - 8 * d)) == (p.hi >> (64 - 8 * d));
    return k.hi == p.hi && (k.lo >> (32 - 8 * (d - 8))) == (p.lo >> (32 - 8 * (d - 8)));
}

__device__ __forceinline__ int orb_kept(const orb_plan& P, const int* counts, int l) {
    int n = counts[l];
    n = n < P.cap[l] ? n : P.cap[l];
    return n < P.quota[l] ? n : P.quota[l];
}

// The best m of the n candidates under the key, written to output rows slot0 .. slot0 + m - 1 in key order; sel holds m entries.
__device__ __forceinline__ void orb_rank_best(const orb_cand* cand, int n, int m, orb_cand* sel, size_t slot0, int l, int32_t* __restrict__ d_kp,
                                              long long* __restrict__ d_resp) {
    __shared__ int s_hist[256];
    __shared__ orb_key s_prefix;
    __shared__ int s_rank, s_taken;
    const int tid = threadIdx.x;
    if (tid == 0) { s_prefix = {0ull, 0u}; s_rank = m; s_taken = 0; }
    if (n > m) {                                                        // the m-th smallest key, digit by digit
        for (int d = 0; d < 12; d++) {
            if (tid < 256) s_hist[tid] = 0;
            __syncthreads();
            const orb_key prefix = s_prefix;
            for (int i = tid; i < n; i += ORB_SEL_THREADS) {
                const orb_key k = orb_key_of(cand[i]);
                if (orb_key_has_prefix(k, prefix, d)) atomicAdd(&s_hist[orb_key_digit(k, d)], 1);
            }
            __syncthreads();
            if (tid == 0) {
                int want = s_rank, g = 0;
                while (g < 255 && want > s_hist[g]) want -= s_hist[g++];
                s_rank = want;
                if (d < 8) s_prefix.hi |= (unsigned long long)g << (56 - 8 * d);
                else s_prefix.lo |= (unsigned)g << (24 - 8 * (d - 8));
            }
            __syncthreads();
        }
    }
    __syncthreads();
    const orb_key limit = s_prefix;
    for (int i = tid; i < n; i += ORB_SEL_THREADS) {
        const orb_cand c = cand[i];
        if (n <= m || !orb_key_less(limit, orb_key_of(c))) {
            const int at = atomicAdd(&s_taken, 1);
            if (at < m) sel[at] = c;                                    // keys are distinct (x, y are), so exactly m pass
        }
    }
    __threadfence_block();
    __syncthreads();
    for (int i = tid; i < m; i += ORB_SEL_THREADS) {                    // rank by counting: the arrival order drops out
        const orb_cand c = sel[i];
        const orb_key k = orb_key_of(c);
        int rank = 0;
        for (int j = 0; j < m; j++) rank += orb_key_less(orb_key_of(sel[j]), k) ? 1 : 0;
        const size_t slot = slot0 + rank;
        d_kp[4 * slot] = (int)(c.xy & 0xFFFF);
        d_kp[4 * slot + 1] = (int)(c.xy >> 16);
        d_kp[4 * slot + 2] = l;
        d_resp[slot] = c.R;
    }
}

__global__ __launch_bounds__(ORB_SEL_THREADS) void orb_select_kernel(orb_plan P, uint8_t* __restrict__ ws, int32_t* __restrict__ d_count,
                                                                     int32_t* __restrict__ d_kp, long long* __restrict__ d_resp) {
    const int tid = threadIdx.x, l = blockIdx.x, b = blockIdx.y;
    const int* counts = (const int*)(ws + P.counts_off) + b * SLAM_ORB_MAX_LEVELS;
    int offset = 0, total = 0;
    for (int j = 0; j < P.L; j++) {
        const int k = orb_kept(P, counts, j);
        if (j < l) offset += k;
        total += k;
    }
    if (l == 0 && tid == 0) d_count[b] = total;
    const int n = counts[l] < P.cap[l] ? counts[l] : P.cap[l], m = orb_kept(P, counts, l);
    if (m == 0) return;
    const orb_cand* cand = (const orb_cand*)(ws + P.image_base + (size_t)b * P.image_stride + P.cand[l]);
    orb_cand* sel = (orb_cand*)(ws + P.sel_off) + (size_t)b * P.n_max + offset;
    orb_rank_best(cand, n, m, sel, (size_t)b * P.n_max + offset, l, d_kp, d_resp);
}

// --------------------------------------------------- 3': adaptive threshold and quadtree distribution
#define ORB_STRONG_WORDS 2048                                           // one bit per 32 x 32 cell: at most 255 x 255 cells on a level

// values that atomics of this block have changed are read past the vector L1
__device__ __forceinline__ int orb_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned long long orb_ld(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned orb_ld(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int orb_root_x(int i, int w, int n_ini) { return ORB_BORDER + (int)((long long)i * w / n_ini); }

// ascending key order of the nodes of a round = (count descending, y0 ascending, x0 ascending)
__device__ __forceinline__ unsigned long long orb_node_key(int count, int x0, int y0) {
    return ((unsigned long long)~(unsigned)count << 32) | ((unsigned long long)(unsigned)y0 << 16) | (unsigned)x0;
}

// the child of a node that holds (x, y): bit 0 = right half, bit 1 = lower half; the halves are cut at x0 + ceil(width / 2)
__device__ __forceinline__ int orb_quadrant(const orb_node& nd, int x, int y) {
    const int xm = nd.x0 + ((nd.x1 - nd.x0 + 1) >> 1), ym = nd.y0 + ((nd.y1 - nd.y0 + 1) >> 1);
    return (x >= xm ? 1 : 0) + (y >= ym ? 2 : 0);
}

// The number of live candidates of level j of one image: those that score >= t_ini, and the weaker ones whose 32 x 32 cell holds no
// such candidate.  Returns early, with a smaller number that is still >= enough, once the strong ones alone reach `enough`; the
// strong count is read between two barriers, so that return is uniform across the block.
// With cn (the block's own level) nothing returns early, every candidate gets its root (or -1 if it is not live) and the
// roots count their live candidates.  All threads of the block call it and get the same value.
__device__ int orb_live(const orb_plan& P, const orb_dist& D, uint8_t* base, int j, int n, int enough, unsigned* s_strong, int* s_cnt,
                        int* cn, orb_node* nodes) {
    const int tid = threadIdx.x, w = P.w[j] - 2 * ORB_BORDER, cells_x = ((w - 1) >> 5) + 1, pitch = P.pitch[j], n_ini = D.n_ini[j];
    const orb_cand* cand = (const orb_cand*)(base + P.cand[j]);
    const uint8_t* score = base + P.score[j];
    __threadfence_block();
    __syncthreads();                                                    // the value of the call before has been read by everyone
    for (int i = tid; i < ORB_STRONG_WORDS; i += ORB_SEL_THREADS) s_strong[i] = 0u;
    if (tid == 0) *s_cnt = D.adaptive ? 0 : n;
    __syncthreads();
    if (D.adaptive) {
        int mine = 0;
        for (int i = tid; i < n; i += ORB_SEL_THREADS) {
            const unsigned xy = cand[i].xy;
            const int x = (int)(xy & 0xFFFF), y = (int)(xy >> 16);
            if (score[(size_t)y * pitch + x] >= D.t_ini) {
                const int c = ((y - ORB_BORDER) >> 5) * cells_x + ((x - ORB_BORDER) >> 5);
                atomicOr(&s_strong[c >> 5], 1u << (c & 31));
                mine++;
            }
        }
        if (mine) atomicAdd(s_cnt, mine);
        __syncthreads();
        const int strong = *s_cnt;                                      // read by everyone before pass two adds to it, so the
        __syncthreads();                                                // return below is taken by the whole block or by nobody
        if (!cn && strong >= enough) return strong;
    }
    if (D.adaptive || cn) {
        int mine = 0;
        for (int i = tid; i < n; i += ORB_SEL_THREADS) {
            const unsigned xy = cand[i].xy;
            const int x = (int)(xy & 0xFFFF), y = (int)(xy >> 16);
            const int c = ((y - ORB_BORDER) >> 5) * cells_x + ((x - ORB_BORDER) >> 5);
            const bool strong = !D.adaptive || score[(size_t)y * pitch + x] >= D.t_ini;
            const bool live = strong || !((s_strong[c >> 5] >> (c & 31)) & 1u);
            mine += !strong && live ? 1 : 0;
            if (cn) {
                int r = -1;
                if (live) {
                    r = (int)((long long)(x - ORB_BORDER) * n_ini / w);
                    r = r > n_ini - 1 ? n_ini - 1 : r;
                    while (r > 0 && orb_root_x(r, w, n_ini) > x) r--;
                    while (r + 1 < n_ini && orb_root_x(r + 1, w, n_ini) <= x) r++;
                    atomicAdd(&nodes[r].count, 1);
                }
                cn[i] = r;
            }
        }
        if (mine) atomicAdd(s_cnt, mine);
        __threadfence_block();
        __syncthreads();
    }
    return *s_cnt;
}

__global__ __launch_bounds__(ORB_SEL_THREADS) void orb_distribute_kernel(orb_plan P, orb_dist D, uint8_t* __restrict__ ws,
                                                                         int32_t* __restrict__ d_count, int32_t* __restrict__ d_kp,
                                                                         long long* __restrict__ d_resp) {
    __shared__ unsigned s_strong[ORB_STRONG_WORDS];
    __shared__ int s_hist[256];
    __shared__ unsigned long long s_cut;
    __shared__ int s_cnt, s_n, s_slots, s_split, s_gain, s_want, s_fin;
    const int tid = threadIdx.x, l = blockIdx.x, b = blockIdx.y;
    const int* counts = (const int*)(ws + P.counts_off) + b * SLAM_ORB_MAX_LEVELS;
    uint8_t* base = ws + P.image_base + (size_t)b * P.image_stride;
    int offset = 0;
    for (int j = 0; j < l; j++) {                                       // rows of the levels below: min(quota, live) each
        const int n = counts[j] < P.cap[j] ? counts[j] : P.cap[j], q = P.quota[j];
        int k = n < q ? n : q;
        if (D.adaptive && k > 0) {
            const int live = orb_live(P, D, base, j, n, q, s_strong, &s_cnt, nullptr, nullptr);
            k = live < q ? live : q;
        }
        offset += k;
    }
    const int n = counts[l] < P.cap[l] ? counts[l] : P.cap[l], N = P.quota[l], n_ini = D.n_ini[l], cap = D.node_cap[l];
    const int w = P.w[l] - 2 * ORB_BORDER, h = P.h[l] - 2 * ORB_BORDER;
    const orb_cand* cand = (const orb_cand*)(base + P.cand[l]);
    orb_node* nodes = (orb_node*)(base + D.node[l]);
    orb_cand* fin = (orb_cand*)(base + D.fin[l]);
    int* cn = (int*)(base + D.cn[l]);
    int live = 0;
    if (n > 0 && N > 0) {                                               // the roots: n_ini vertical strips of the scoreable rectangle
        for (int i = tid; i < n_ini; i += ORB_SEL_THREADS) {
            orb_node nd = {0ull, 0xFFFFFFFFu, 0, (short)orb_root_x(i, w, n_ini), (short)ORB_BORDER, (short)orb_root_x(i + 1, w, n_ini),
                           (short)(ORB_BORDER + h), -1, 0, {0, 0, 0, 0}, {0, 0, 0, 0}};
            nodes[i] = nd;
        }
        live = orb_live(P, D, base, l, n, 0, s_strong, &s_cnt, cn, nodes);
    }
    const int m = live < N ? live : N;
    if (l == P.L - 1 && tid == 0) d_count[b] = offset + m;
    if (m == 0) return;
    if (tid == 0) { s_n = 0; s_slots = n_ini; }
    __syncthreads();
    for (int i = tid; i < n_ini; i += ORB_SEL_THREADS)
        if (orb_ld(&nodes[i].count) > 0) atomicAdd(&s_n, 1);
    __syncthreads();
    for (int round = 0; round < 32; round++) {                          // split the fullest nodes until there are N; extents halve: <= 15 rounds
        const int n_nodes = s_n, slots = s_slots < cap ? s_slots : cap;
        if (n_nodes >= N) break;
        __syncthreads();
        if (tid == 0) { s_split = 0; s_gain = 0; s_cut = 0ull; s_want = N - n_nodes; }
        const bool in_lds = 4 * slots <= ORB_STRONG_WORDS;              // few nodes, many adds on each: the child counts go to the LDS,
        int* s_cc = (int*)s_strong;                                     // where the bitmap was, and are copied to the table below
        if (in_lds)
            for (int i = tid; i < 4 * slots; i += ORB_SEL_THREADS) s_cc[i] = 0;
        for (int j = tid; j < slots; j += ORB_SEL_THREADS) {
            if (orb_ld(&nodes[j].count) > 1) { nodes[j].cc[0] = 0; nodes[j].cc[1] = 0; nodes[j].cc[2] = 0; nodes[j].cc[3] = 0; }
            nodes[j].gain = -1;
            nodes[j].split = 0;
        }
        __threadfence_block();
        __syncthreads();
        for (int i = tid; i < n; i += ORB_SEL_THREADS) {                // live candidates per child of every splittable node
            const int j = cn[i];
            if (j >= 0 && orb_ld(&nodes[j].count) > 1) {
                const unsigned xy = cand[i].xy;
                const int q = orb_quadrant(nodes[j], (int)(xy & 0xFFFF), (int)(xy >> 16));
                if (in_lds) atomicAdd(&s_cc[4 * j + q], 1);
                else atomicAdd(&nodes[j].cc[q], 1);
            }
        }
        __syncthreads();
        for (int j = tid; j < slots; j += ORB_SEL_THREADS) {
            if (orb_ld(&nodes[j].count) > 1) {
                int g = -1;
                for (int q = 0; q < 4; q++) {
                    if (in_lds) nodes[j].cc[q] = s_cc[4 * j + q];
                    g += (in_lds ? s_cc[4 * j + q] : orb_ld(&nodes[j].cc[q])) > 0 ? 1 : 0;
                }
                nodes[j].gain = g;
                atomicAdd(&s_split, 1);
                if (g) atomicAdd(&s_gain, g);
            }
        }
        __threadfence_block();
        __syncthreads();
        if (s_split == 0) break;
        if (s_gain >= N - n_nodes) {                                    // the key at which the running sum of gains reaches N - n_nodes
            for (int d = 0; d < 8; d++) {
                if (tid < 256) s_hist[tid] = 0;
                __syncthreads();
                const unsigned long long prefix = s_cut;
                for (int j = tid; j < slots; j += ORB_SEL_THREADS) {
                    const int g = nodes[j].gain;
                    if (g > 0) {
                        const unsigned long long k = orb_node_key(orb_ld(&nodes[j].count), nodes[j].x0, nodes[j].y0);
                        if (d == 0 || (k >> (64 - 8 * d)) == (prefix >> (64 - 8 * d))) atomicAdd(&s_hist[(unsigned)(k >> (56 - 8 * d)) & 255u], g);
                    }
                }
                __syncthreads();
                if (tid == 0) {
                    int want = s_want, g = 0;
                    while (g < 255 && want > s_hist[g]) want -= s_hist[g++];
                    s_want = want;
                    s_cut |= (unsigned long long)g << (56 - 8 * d);
                }
                __syncthreads();
            }
        } else {
            if (tid == 0) s_cut = ~0ull;                                // the gains never reach it: every splittable node is split
            __syncthreads();
        }
        const unsigned long long cut = s_cut;
        for (int j = tid; j < slots; j += ORB_SEL_THREADS) {            // slots of the children: the first stays where its parent is
            if (nodes[j].gain < 0 || orb_node_key(orb_ld(&nodes[j].count), nodes[j].x0, nodes[j].y0) > cut) continue;
            bool first = true;
            for (int q = 0; q < 4; q++) {
                int at = -1;
                if (orb_ld(&nodes[j].cc[q]) > 0) {
                    at = first ? j : atomicAdd(&s_slots, 1);
                    first = false;
                }
                nodes[j].cm[q] = at < cap ? at : -1;                    // n_ini + N + 2 slots always suffice
            }
            nodes[j].split = 1;
            atomicAdd(&s_n, nodes[j].gain);
        }
        __threadfence_block();
        __syncthreads();
        for (int i = tid; i < n; i += ORB_SEL_THREADS) {                // candidates move to the child they lie in
            const int j = cn[i];
            if (j >= 0 && nodes[j].split) {
                const unsigned xy = cand[i].xy;
                cn[i] = nodes[j].cm[orb_quadrant(nodes[j], (int)(xy & 0xFFFF), (int)(xy >> 16))];
            }
        }
        __threadfence_block();
        __syncthreads();
        for (int j = tid; j < slots; j += ORB_SEL_THREADS) {            // the children are written over and behind the nodes of the round
            if (!nodes[j].split) continue;
            const orb_node nd = nodes[j];
            const int xm = nd.x0 + ((nd.x1 - nd.x0 + 1) >> 1), ym = nd.y0 + ((nd.y1 - nd.y0 + 1) >> 1);
            for (int q = 0; q < 4; q++) {
                if (nd.cm[q] < 0) continue;
                const int c = orb_ld(&nodes[j].cc[q]);                  // slot j itself is written last: child 0, or read before
                orb_node ch = {0ull, 0xFFFFFFFFu, c, (short)(q & 1 ? xm : nd.x0), (short)(q & 2 ? ym : nd.y0), (short)(q & 1 ? nd.x1 : xm),
                               (short)(q & 2 ? nd.y1 : ym), -1, 0, {0, 0, 0, 0}, {0, 0, 0, 0}};
                if (nd.cm[q] != j) nodes[nd.cm[q]] = ch;
            }
            for (int q = 0; q < 4; q++) {
                if (nd.cm[q] != j) continue;
                orb_node ch = {0ull, 0xFFFFFFFFu, orb_ld(&nodes[j].cc[q]), (short)(q & 1 ? xm : nd.x0), (short)(q & 2 ? ym : nd.y0),
                               (short)(q & 1 ? nd.x1 : xm), (short)(q & 2 ? nd.y1 : ym), -1, 0, {0, 0, 0, 0}, {0, 0, 0, 0}};
                nodes[j] = ch;
            }
        }
        __threadfence_block();
        __syncthreads();
    }
    __syncthreads();
    const int slots = s_slots < cap ? s_slots : cap;
    if (tid == 0) s_fin = 0;
    for (int i = tid; i < n; i += ORB_SEL_THREADS) {                    // the best live candidate of every node: R first ...
        const int j = cn[i];
        if (j >= 0) atomicMax(&nodes[j].best, (unsigned long long)cand[i].R ^ (1ull << 63));
    }
    __syncthreads();
    for (int i = tid; i < n; i += ORB_SEL_THREADS) {                    // ... then the smallest y, x among those that have it
        const int j = cn[i];
        if (j >= 0 && orb_ld(&nodes[j].best) == ((unsigned long long)cand[i].R ^ (1ull << 63))) atomicMin(&nodes[j].bxy, cand[i].xy);
    }
    __syncthreads();
    for (int j = tid; j < slots; j += ORB_SEL_THREADS) {
        if (orb_ld(&nodes[j].count) > 0) {
            const int at = atomicAdd(&s_fin, 1);
            orb_cand c = {(long long)(orb_ld(&nodes[j].best) ^ (1ull << 63)), orb_ld(&nodes[j].bxy), 0u};
            fin[at] = c;
        }
    }
    __threadfence_block();
    __syncthreads();
    orb_cand* sel = (orb_cand*)(ws + P.sel_off) + (size_t)b * P.n_max + offset;
    orb_rank_best(fin, s_fin, m, sel, (size_t)b * P.n_max + offset, l, d_kp, d_resp);
}

// ------------------------------------------------------------------------------------------ 4: orientation + descriptor
// boundary directions at (k + 1/2) 11.25 degrees, k = 0..7, as rint(2^14 cos), rint(2^14 sin); the other quadrants are exact rotations
__constant__ int orb_bound_x[8] = {16305, 15679, 14449, 12665, 10394, 7723, 4756, 1606};
__constant__ int orb_bound_y[8] = {1606, 4756, 7723, 10394, 12665, 14449, 15679, 16305};

__device__ __forceinline__ long long orb_cross(int k, long long m10, long long m01) {   // boundary k x (m10, m01)
    const int q = (k >> 3) & 3;
    long long dx = orb_bound_x[k & 7], dy = orb_bound_y[k & 7];
    for (int i = 0; i < q; i++) { const long long tmp = dx; dx = -dy; dy = tmp; }
    return dx * m01 - dy * m10;
}

__global__ __launch_bounds__(ORB_THREADS) void orb_describe_kernel(orb_plan P, int64_t slots, const uint8_t* __restrict__ ws,
                                                                   const int* __restrict__ table, const int32_t* __restrict__ d_count,
                                                                   int32_t* __restrict__ d_kp, long long* __restrict__ d_resp,
                                                                   unsigned long long* __restrict__ d_desc) {
    const int lane = threadIdx.x & 63;
    const int64_t slot = (int64_t)blockIdx.x * (ORB_THREADS / 64) + (threadIdx.x >> 6);
    if (slot >= slots) return;
    const int b = (int)(slot / P.n_max), i = (int)(slot - (int64_t)b * P.n_max);
    if (i >= d_count[b]) {                                               // an unused slot: all zero
        if (lane < 4) { d_kp[4 * slot + lane] = 0; d_desc[4 * slot + lane] = 0ull; }
        if (lane == 0) d_resp[slot] = 0;
        return;
    }
    const int x = d_kp[4 * slot], y = d_kp[4 * slot + 1], l = d_kp[4 * slot + 2], pitch = P.pitch[l];
    const uint8_t* base = ws + P.image_base + (size_t)b * P.image_stride;
    const uint8_t* img = base + P.img[l] + (size_t)y * pitch + x;        // BORDER = 16 keeps the radius-15 disc inside the level
    int m10 = 0, m01 = 0;
    for (int j = lane; j < 31 * 31; j += 64) {
        const int dy = j / 31 - 15, dx = j - (j / 31) * 31 - 15;
        if (dx * dx + dy * dy <= 225) {
            const int v = img[dy * pitch + dx];
            m10 += dx * v;
            m01 += dy * v;
        }
    }
    m10 = orb_wave_sum(m10);
    m01 = orb_wave_sum(m01);
    // bin k: at or past boundary k-1 and before boundary k; no lane answers for (0, 0): bin 0
    const bool mine = lane < 32 && orb_cross((lane + 31) & 31, m10, m01) >= 0 && orb_cross(lane, m10, m01) < 0;
    const unsigned long long vote = __ballot(mine);
    const int bin = vote ? __ffsll((long long)vote) - 1 : 0;
    if (lane == 0) d_kp[4 * slot + 3] = bin;
    const uint8_t* blurred = base + P.blur[l] + (size_t)y * pitch + x;
    const int* steer = table + bin * 256;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int e = steer[64 * k + lane];                              // int8 x 4: ax, ay, bx, by
        const int ax = (signed char)(e & 255), ay = (signed char)((e >> 8) & 255), bx = (signed char)((e >> 16) & 255), by = (signed char)(e >> 24);
        const unsigned long long bits = __ballot(blurred[ay * pitch + ax] < blurred[by * pitch + bx]);
        if (lane == 0) d_desc[4 * slot + k] = bits;                      // lane j of test 64 k + j: bit j % 8 of byte j / 8
    }
}

// ================================================================ entry points ================================================
extern "C" int slam_orb_workspace(int64_t B, int64_t H, int64_t W, int L, const int32_t* h_level_w, const int32_t* h_level_h, int64_t n_max,
                                  uint64_t* bytes, uint64_t* h_layout) {
    orb_plan P;
    uint64_t total = 0;
    if (int rc = orb_make_plan("slam_orb_workspace", B, H, W, L, h_level_w, h_level_h, n_max, P, total)) return rc;
    SLAM_REQUIRE(bytes, "slam_orb_workspace: null bytes");
    *bytes = total;
    if (h_layout) {
        h_layout[0] = P.image_base; h_layout[1] = P.image_stride; h_layout[2] = P.counts_off; h_layout[3] = P.sel_off;
        for (int l = 0; l < L; l++) {
            uint64_t* e = h_layout + 4 + 6 * l;
            e[0] = P.img[l]; e[1] = P.blur[l]; e[2] = P.score[l]; e[3] = P.cand[l]; e[4] = (uint64_t)P.pitch[l]; e[5] = (uint64_t)P.cap[l];
        }
    }
    return SLAM_OK;
}

// everything after the argument checks; the caller holds whatever lock its buffers need
static int orb_launch(slam_ctx* ctx, const orb_plan& P, int64_t B, const uint8_t* d_images, const uint8_t* d_mask, int mask_batched,
                      int fast_threshold, const int8_t* d_table, void* d_workspace, int32_t* d_count, int32_t* d_kp, int64_t* d_resp,
                      uint8_t* d_desc, const orb_dist* dist = nullptr) {
    const dim3 tiles((unsigned)P.tile0[P.L], (unsigned)B);
    orb_pyramid_kernel<<<tiles, ORB_THREADS, 0, ctx->stream>>>(P, d_images, (uint8_t*)d_workspace);
    SLAM_HIP(hipGetLastError());
    orb_fast_kernel<<<tiles, ORB_THREADS, 0, ctx->stream>>>(P, d_mask, mask_batched ? (unsigned long long)P.H * P.W : 0ull, fast_threshold,
                                                            (uint8_t*)d_workspace);
    SLAM_HIP(hipGetLastError());
    if (dist)
        orb_distribute_kernel<<<dim3((unsigned)P.L, (unsigned)B), ORB_SEL_THREADS, 0, ctx->stream>>>(P, *dist, (uint8_t*)d_workspace, d_count,
                                                                                                     d_kp, (long long*)d_resp);
    else
        orb_select_kernel<<<dim3((unsigned)P.L, (unsigned)B), ORB_SEL_THREADS, 0, ctx->stream>>>(P, (uint8_t*)d_workspace, d_count, d_kp,
                                                                                                 (long long*)d_resp);
    SLAM_HIP(hipGetLastError());
    if (P.n_max > 0) {
        const int64_t slots = B * P.n_max;
        orb_describe_kernel<<<(unsigned)((slots + ORB_THREADS / 64 - 1) / (ORB_THREADS / 64)), ORB_THREADS, 0, ctx->stream>>>(
            P, slots, (const uint8_t*)d_workspace, (const int*)d_table, d_count, d_kp, (long long*)d_resp, (unsigned long long*)d_desc);
        SLAM_HIP(hipGetLastError());
    }
    return SLAM_OK;
}

static int orb_checks(const char* who, slam_ctx* ctx, int64_t B, int64_t H, int64_t W, int L, const int32_t* h_level_w, const int32_t* h_level_h,
                      const int32_t* h_quota, int fast_threshold, orb_plan& P, uint64_t& total) {
    SLAM_REQUIRE(ctx, "%s: null ctx", who);
    SLAM_REQUIRE(L >= 1 && L <= SLAM_ORB_MAX_LEVELS, "%s: L=%d out of range [1, %d]", who, L, SLAM_ORB_MAX_LEVELS);
    SLAM_REQUIRE(h_quota, "%s: null quota array", who);
    SLAM_REQUIRE(fast_threshold >= 1 && fast_threshold <= 254, "%s: fast_threshold=%d out of range [1, 254]", who, fast_threshold);
    int64_t n_max = 0;
    for (int l = 0; l < L; l++) {
        SLAM_REQUIRE(h_quota[l] >= 0 && h_quota[l] <= SLAM_ORB_MAX_FEATURES, "%s: quota[%d]=%d out of range [0, %d]", who, l, h_quota[l],
                     SLAM_ORB_MAX_FEATURES);
        n_max += h_quota[l];
    }
    if (int rc = orb_make_plan(who, B, H, W, L, h_level_w, h_level_h, n_max, P, total)) return rc;
    for (int l = 0; l < L; l++) P.quota[l] = h_quota[l];
    return SLAM_OK;
}

extern "C" int slam_orb_extract_u8(slam_ctx* ctx, const uint8_t* d_images, int64_t B, int64_t H, int64_t W, const uint8_t* d_mask,
                                   int mask_batched, int L, const int32_t* h_level_w, const int32_t* h_level_h, const int32_t* h_quota,
                                   int fast_threshold, const int8_t* d_table, void* d_workspace, uint64_t workspace_bytes, int32_t* d_count,
                                   int32_t* d_kp, int64_t* d_resp, uint8_t* d_desc) {
    orb_plan P;
    uint64_t total = 0;
    if (int rc = orb_checks("slam_orb_extract_u8", ctx, B, H, W, L, h_level_w, h_level_h, h_quota, fast_threshold, P, total)) return rc;
    if (B == 0) return SLAM_OK;
    SLAM_REQUIRE(d_images && d_table && d_workspace && d_count && (P.n_max == 0 || (d_kp && d_resp && d_desc)),
                 "slam_orb_extract_u8: null device pointer");
    SLAM_REQUIRE(workspace_bytes >= total, "slam_orb_extract_u8: workspace of %llu bytes, %llu needed (slam_orb_workspace)",
                 (unsigned long long)workspace_bytes, (unsigned long long)total);
    SLAM_REQUIRE((((uintptr_t)d_workspace | (uintptr_t)d_table | (uintptr_t)d_desc | (uintptr_t)d_kp | (uintptr_t)d_resp) & 15) == 0,
                 "slam_orb_extract_u8: d_workspace, d_table, d_kp, d_resp and d_desc must be 16-byte aligned");
    SLAM_HIP(hipSetDevice(ctx->device));
    return orb_launch(ctx, P, B, d_images, d_mask, mask_batched, fast_threshold, d_table, d_workspace, d_count, d_kp, d_resp, d_desc);
}

// Appends, to every image block of a finished plan, what the quadtree selection needs per level: a node index per candidate, the
// node table (the roots and at most quota + 2 children) and the list of the nodes' best candidates.
static void orb_extend_plan(orb_plan& P, orb_dist& D, int64_t B, uint64_t& total) {
    memset(&D, 0, sizeof(D));
    uint64_t off = P.image_stride;
    for (int l = 0; l < P.L; l++) {
        const int w = P.w[l] - 2 * ORB_BORDER, h = P.h[l] - 2 * ORB_BORDER;
        if (P.cap[l] > 0) {
            const long long roots = (2ll * w + h) / (2ll * h);
            D.n_ini[l] = (int)(roots > 1 ? roots : 1);
            D.node_cap[l] = D.n_ini[l] + P.quota[l] + 2;
        }
        D.cn[l] = off; off += orb_up((uint64_t)P.cap[l] * 4, 16);
        D.node[l] = off; off += (uint64_t)D.node_cap[l] * sizeof(orb_node);
        D.fin[l] = off; off += (uint64_t)D.node_cap[l] * sizeof(orb_cand);
    }
    P.image_stride = orb_up(off, 256);
    total = P.image_base + (uint64_t)(B > 0 ? B : 1) * P.image_stride;
}

static int orb_dist_checks(const char* who, int fast_threshold, int fast_threshold_min, orb_plan& P, orb_dist& D, int64_t B, uint64_t& total) {
    SLAM_REQUIRE(fast_threshold_min >= 1 && fast_threshold_min <= fast_threshold, "%s: fast_threshold_min=%d out of range [1, fast_threshold=%d]",
                 who, fast_threshold_min, fast_threshold);
    orb_extend_plan(P, D, B, total);
    D.t_ini = fast_threshold;
    D.adaptive = fast_threshold_min < fast_threshold;
    return SLAM_OK;
}

extern "C" int slam_orb_dist_workspace(int64_t B, int64_t H, int64_t W, int L, const int32_t* h_level_w, const int32_t* h_level_h,
                                       const int32_t* h_quota, uint64_t* bytes, uint64_t* h_layout) {
    orb_plan P;
    orb_dist D;
    uint64_t total = 0;
    SLAM_REQUIRE(L >= 1 && L <= SLAM_ORB_MAX_LEVELS, "slam_orb_dist_workspace: L=%d out of range [1, %d]", L, SLAM_ORB_MAX_LEVELS);
    SLAM_REQUIRE(h_quota, "slam_orb_dist_workspace: null quota array");
    int64_t n_max = 0;
    for (int l = 0; l < L; l++) {
        SLAM_REQUIRE(h_quota[l] >= 0 && h_quota[l] <= SLAM_ORB_MAX_FEATURES, "slam_orb_dist_workspace: quota[%d]=%d out of range [0, %d]", l,
                     h_quota[l], SLAM_ORB_MAX_FEATURES);
        n_max += h_quota[l];
    }
    if (int rc = orb_make_plan("slam_orb_dist_workspace", B, H, W, L, h_level_w, h_level_h, n_max, P, total)) return rc;
    SLAM_REQUIRE(bytes, "slam_orb_dist_workspace: null bytes");
    for (int l = 0; l < L; l++) P.quota[l] = h_quota[l];
    orb_extend_plan(P, D, B, total);
    *bytes = total;
    if (h_layout) {
        h_layout[0] = P.image_base; h_layout[1] = P.image_stride; h_layout[2] = P.counts_off; h_layout[3] = P.sel_off;
        for (int l = 0; l < L; l++) {
            uint64_t* e = h_layout + 4 + 6 * l;
            e[0] = P.img[l]; e[1] = P.blur[l]; e[2] = P.score[l]; e[3] = P.cand[l]; e[4] = (uint64_t)P.pitch[l]; e[5] = (uint64_t)P.cap[l];
            uint64_t* f = h_layout + 4 + 6 * L + 4 * l;
            f[0] = D.cn[l]; f[1] = D.node[l]; f[2] = D.fin[l]; f[3] = (uint64_t)D.node_cap[l];
        }
    }
    return SLAM_OK;
}

extern "C" int slam_orb_extract_dist_u8(slam_ctx* ctx, const uint8_t* d_images, int64_t B, int64_t H, int64_t W, const uint8_t* d_mask,
                                        int mask_batched, int L, const int32_t* h_level_w, const int32_t* h_level_h, const int32_t* h_quota,
                                        int fast_threshold, int fast_threshold_min, const int8_t* d_table, void* d_workspace,
                                        uint64_t workspace_bytes, int32_t* d_count, int32_t* d_kp, int64_t* d_resp, uint8_t* d_desc) {
    orb_plan P;
    orb_dist D;
    uint64_t total = 0;
    if (int rc = orb_checks("slam_orb_extract_dist_u8", ctx, B, H, W, L, h_level_w, h_level_h, h_quota, fast_threshold, P, total)) return rc;
    if (int rc = orb_dist_checks("slam_orb_extract_dist_u8", fast_threshold, fast_threshold_min, P, D, B, total)) return rc;
    if (B == 0) return SLAM_OK;
    SLAM_REQUIRE(d_images && d_table && d_workspace && d_count && (P.n_max == 0 || (d_kp && d_resp && d_desc)),
                 "slam_orb_extract_dist_u8: null device pointer");
    SLAM_REQUIRE(workspace_bytes >= total, "slam_orb_extract_dist_u8: workspace of %llu bytes, %llu needed (slam_orb_dist_workspace)",
                 (unsigned long long)workspace_bytes, (unsigned long long)total);
    SLAM_REQUIRE((((uintptr_t)d_workspace | (uintptr_t)d_table | (uintptr_t)d_desc | (uintptr_t)d_kp | (uintptr_t)d_resp) & 15) == 0,
                 "slam_orb_extract_dist_u8: d_workspace, d_table, d_kp, d_resp and d_desc must be 16-byte aligned");
    SLAM_HIP(hipSetDevice(ctx->device));
    return orb_launch(ctx, P, B, d_images, d_mask, mask_batched, fast_threshold_min, d_table, d_workspace, d_count, d_kp, d_resp, d_desc, &D);
}

extern "C" int slam_orb_extract_u8_host(slam_ctx* ctx, const uint8_t* h_images, int64_t B, int64_t H, int64_t W, const uint8_t* h_mask,
                                        int mask_batched, int L, const int32_t* h_level_w, const int32_t* h_level_h, const int32_t* h_quota,
                                        int fast_threshold, const int8_t* h_table, int32_t* h_count, int32_t* h_kp, int64_t* h_resp,
                                        uint8_t* h_desc) {
    orb_plan P;
    uint64_t total = 0;
    if (int rc = orb_checks("slam_orb_extract_u8_host", ctx, B, H, W, L, h_level_w, h_level_h, h_quota, fast_threshold, P, total)) return rc;
    if (B == 0) return SLAM_OK;
    SLAM_REQUIRE(h_images && h_table && h_count && (P.n_max == 0 || (h_kp && h_resp && h_desc)), "slam_orb_extract_u8_host: null host pointer");
    std::lock_guard<std::mutex> lk(ctx->call_mu);                       // the workspace and the staging arena are the context's
    SLAM_HIP(hipSetDevice(ctx->device));
    const uint64_t n_img = (uint64_t)B * H * W, n_mask = h_mask ? (mask_batched ? n_img : (uint64_t)H * W) : 0, slots = (uint64_t)B * P.n_max;
    const uint64_t o_table = 0, o_img = orb_up(SLAM_ORB_TABLE_BYTES, 256), o_mask = o_img + orb_up(n_img, 256), o_count = o_mask + orb_up(n_mask, 256);
    const uint64_t o_kp = o_count + orb_up((uint64_t)B * 4, 256), o_resp = o_kp + orb_up(slots * 16, 256), o_desc = o_resp + orb_up(slots * 8, 256);
    const uint64_t io_total = o_desc + orb_up(slots * 32, 256);
    void *ws = nullptr, *dev = nullptr, *host = nullptr;
    if (int rc = slam_io_arena(ctx, io_total, io_total, &dev, &host)) return rc;
    if (int rc = slam_workspace(ctx, total, &ws)) return rc;
    uint8_t *hb = (uint8_t*)host, *db = (uint8_t*)dev;
    memcpy(hb + o_table, h_table, SLAM_ORB_TABLE_BYTES);
    memcpy(hb + o_img, h_images, n_img);
    if (n_mask) memcpy(hb + o_mask, h_mask, n_mask);
    ctx->io_h2d_bytes += o_count;
    ctx->io_d2h_bytes += io_total - o_count;
    SLAM_HIP(hipMemcpyAsync(db, hb, o_count, hipMemcpyHostToDevice, ctx->stream));
    if (int rc = orb_launch(ctx, P, B, db + o_img, n_mask ? db + o_mask : nullptr, mask_batched, fast_threshold, (const int8_t*)(db + o_table), ws,
                            (int32_t*)(db + o_count), (int32_t*)(db + o_kp), (int64_t*)(db + o_resp), db + o_desc))
        return rc;
    SLAM_HIP(hipMemcpyAsync(hb + o_count, db + o_count, io_total - o_count, hipMemcpyDeviceToHost, ctx->stream));
    SLAM_HIP(hipStreamSynchronize(ctx->stream));
    memcpy(h_count, hb + o_count, (size_t)B * 4);
    if (slots) {
        memcpy(h_kp, hb + o_kp, slots * 16);
        memcpy(h_resp, hb + o_resp, slots * 8);
        memcpy(h_desc, hb + o_desc, slots * 32);
    }
    return SLAM_OK;
}
