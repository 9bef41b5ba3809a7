// camera.hip — lens distortion on gfx950: what ORB-SLAM does in Frame::UndistortKeyPoints / ComputeImageBounds
// and OpenCV in initUndistortRectifyMap + remap, on device-resident rows.
//
//   slam_cam_undistort_f64   raw pixels -> pinhole pixels, normalised coordinates and a status per point (Newton, cam_model.h)
//   slam_cam_distort_f64     pinhole pixels -> raw pixels
//   slam_cam_rectify_map     the fixed-point map (1/32 pixel) of a destination camera K', R into the raw image
//   slam_cam_remap_u8        bilinear resampling of B images through one map, integers only, with a validity mask
//
// The arithmetic of the first three is cam_model.h, which tests/camera_twin.cpp builds for the host from the same text.  The
// camera records, the set table and the rotation travel in the kernel arguments: every lane of a workgroup works on one set,
// so the record and the model switch are uniform and live in scalar registers.  No entry point takes memory from the context.
#include "internal.h"
#include "cam_model.h"
#include <math.h>

#define CAM_LANES 256
#define CAM_SETS 32             // point sets per launch of cam_points_kernel (more sets: more launches)

struct cam_sets {
    int nsets;
    int blk[CAM_SETS + 1];      // first workgroup of each set; blk[nsets] = the grid
    int first[CAM_SETS];        // first point of each set
    int count[CAM_SETS];
    int cam[CAM_SETS];
};

struct cam_table {
    cam_rec c[SLAM_CAM_MAX];
};

struct cam_view {
    cam_rec c;
    double R[9];
    double nfx, nfy, ncx, ncy;
};

// one lane per point, workgroups by set.  dir 0: undistort, 1: distort.
__global__ __launch_bounds__(CAM_LANES) void cam_points_kernel(cam_sets S, cam_table T, int dir, int iterations, const double* __restrict__ px,
                                                               double* __restrict__ px_out, double* __restrict__ norm,
                                                               uint8_t* __restrict__ status) {
    const int blk = blockIdx.x;
    int s = 0;
    for (int k = 1; k < S.nsets; k++) s += blk >= S.blk[k] ? 1 : 0;
    s = __builtin_amdgcn_readfirstlane(s);
    const int i = (blk - S.blk[s]) * CAM_LANES + (int)threadIdx.x;
    if (i >= S.count[s]) return;
    const cam_rec c = T.c[S.cam[s]];
    const int model = (int)c.model;
    const size_t p = (size_t)S.first[s] + (size_t)i;
    const double u = px[2 * p], v = px[2 * p + 1];
    const cam_point o = dir == 0 ? cam_undistort_px(c, model, u, v, iterations) : cam_distort_px(c, model, u, v);
    px_out[2 * p] = o.u;
    px_out[2 * p + 1] = o.v;
    if (norm) {
        norm[2 * p] = o.x;
        norm[2 * p + 1] = o.y;
    }
    status[p] = (uint8_t)o.status;
}

// one lane per map entry, 64 x 4 entries a workgroup; an entry is one 8-byte store
__global__ __launch_bounds__(CAM_LANES) void cam_map_kernel(cam_view V, int Wd, int Hd, int32_t* __restrict__ map) {
    const int j = blockIdx.x * 64 + threadIdx.x, i = blockIdx.y * 4 + threadIdx.y;
    if (j >= Wd || i >= Hd) return;
    int32_t U, W;
    cam_map_entry(V.c, (int)V.c.model, V.R, V.nfx, V.nfy, V.ncx, V.ncy, j, i, &U, &W);
    reinterpret_cast<int2*>(map)[(size_t)i * Wd + j] = make_int2(U, W);
}

// one tap: nothing is loaded for a weight of 0; a tap outside the source reads the border and clears *ok
__device__ __forceinline__ int cam_tap(const uint8_t* __restrict__ img, int64_t pitch, int Ws, int Hs, int x, int y, int w, int border, bool* ok) {
    if (w == 0) return 0;
    if (x >= 0 && x < Ws && y >= 0 && y < Hs) return w * (int)img[(int64_t)y * pitch + x];
    *ok = false;
    return w * border;
}

// four destination pixels of one row per lane (one dword store each for the image and the mask where the rows allow it), 64 x 4
// lanes a workgroup; the lane keeps its four map entries and walks the images b = blockIdx.z, blockIdx.z + gridDim.z, ...
__global__ __launch_bounds__(CAM_LANES) void cam_remap_kernel(const uint8_t* __restrict__ src, int B, int Hs, int Ws, int64_t src_pitch,
                                                              int64_t src_stride, const int32_t* __restrict__ map, int Hd, int Wd, int border,
                                                              uint8_t* __restrict__ dst, int64_t dst_pitch, int64_t dst_stride,
                                                              uint8_t* __restrict__ mask, int words) {
    const int x4 = (blockIdx.x * 64 + threadIdx.x) * 4, y = blockIdx.y * 4 + threadIdx.y;
    if (x4 >= Wd || y >= Hd) return;
    const int nx = Wd - x4 < 4 ? Wd - x4 : 4;
    int2 e[4];
#pragma unroll
    for (int q = 0; q < 4; q++) e[q] = q < nx ? reinterpret_cast<const int2*>(map)[(size_t)y * Wd + x4 + q] : make_int2(CAM_MAP_SENTINEL, CAM_MAP_SENTINEL);
    for (int b = blockIdx.z; b < B; b += gridDim.z) {
        const uint8_t* img = src + (int64_t)b * src_stride;
        unsigned pix = 0, mk = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int U = e[q].x, V = e[q].y;
            int p = border;
            bool ok = false;
            if (U != CAM_MAP_SENTINEL && V != CAM_MAP_SENTINEL) {
                const int x0 = U >> 5, a = U & 31, y0 = V >> 5, c = V & 31;
                ok = true;
                int sum = cam_tap(img, src_pitch, Ws, Hs, x0, y0, (32 - a) * (32 - c), border, &ok);
                sum += cam_tap(img, src_pitch, Ws, Hs, x0 + 1, y0, a * (32 - c), border, &ok);
                sum += cam_tap(img, src_pitch, Ws, Hs, x0, y0 + 1, (32 - a) * c, border, &ok);
                sum += cam_tap(img, src_pitch, Ws, Hs, x0 + 1, y0 + 1, a * c, border, &ok);
                p = (sum + 512) >> 10;
            }
            pix |= (unsigned)p << (8 * q);
            mk |= (ok ? 255u : 0u) << (8 * q);
        }
        const int64_t o = (int64_t)b * dst_stride + (int64_t)y * dst_pitch + x4;
        if (words && nx == 4) {
            *reinterpret_cast<unsigned*>(dst + o) = pix;
            if (mask) *reinterpret_cast<unsigned*>(mask + o) = mk;
        } else {
            for (int q = 0; q < nx; q++) {
                dst[o + q] = (uint8_t)(pix >> (8 * q));
                if (mask) mask[o + q] = (uint8_t)(mk >> (8 * q));
            }
        }
    }
}

// ================================================================= entry points ==============================================
// [a, a + na) and [b, b + nb) share a byte (null pointers share nothing)
static bool cam_overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && x < y + nb && y < x + na;
}

static int cam_points(slam_ctx* ctx, const char* who, int dir, int64_t B, const int64_t* h_offsets, int64_t C, const double* h_cameras,
                      const int32_t* h_cam_index, int iterations, const double* d_px, double* d_px_out, double* d_norm, uint8_t* d_status) {
    SLAM_REQUIRE(ctx, "%s: null ctx", who);
    SLAM_REQUIRE(B >= 0 && B <= (1 << 20) && C >= 1 && C <= SLAM_CAM_MAX, "%s: bad sizes (B=%lld, C=%lld; C in [1, %d])", who, (long long)B,
                 (long long)C, SLAM_CAM_MAX);
    SLAM_REQUIRE(h_offsets && h_cameras, "%s: null host pointer", who);
    SLAM_REQUIRE(iterations >= 0 && iterations <= SLAM_CAM_ITERATIONS_MAX, "%s: iterations=%d must be in [0, %d]", who, iterations,
                 SLAM_CAM_ITERATIONS_MAX);
    for (int64_t k = 0; k < C; k++) {
        const int bad = cam_record_check(h_cameras + CAM_RECORD * k);
        SLAM_REQUIRE(bad == 0, "%s: camera %lld: %s", who, (long long)k,
                     bad == 1 ? "a value is not finite" : bad == 2 ? "fx and fy must be positive" : "the model must be 0, 1 or 2");
    }
    SLAM_REQUIRE(h_offsets[0] == 0, "%s: offsets must start at 0", who);
    for (int64_t b = 0; b < B; b++) {
        SLAM_REQUIRE(h_offsets[b + 1] >= h_offsets[b] && h_offsets[b + 1] <= (1 << 30), "%s: offsets must ascend and stay within 2^30", who);
        SLAM_REQUIRE(!h_cam_index || (h_cam_index[b] >= 0 && h_cam_index[b] < C), "%s: set %lld names camera %d of %lld", who, (long long)b,
                     h_cam_index ? h_cam_index[b] : 0, (long long)C);
    }
    const int64_t n = h_offsets[B];
    if (n == 0) return SLAM_OK;
    SLAM_REQUIRE(d_px && d_px_out && d_status, "%s: null device pointer", who);
    SLAM_REQUIRE(!cam_overlap(d_px, 16 * (uint64_t)n, d_px_out, 16 * (uint64_t)n) && !cam_overlap(d_px, 16 * (uint64_t)n, d_norm, 16 * (uint64_t)n) &&
                     !cam_overlap(d_px, 16 * (uint64_t)n, d_status, (uint64_t)n),
                 "%s: an output overlaps d_px (the call does not work in place)", who);
    SLAM_HIP(hipSetDevice(ctx->device));
    cam_table T;
    memset(&T, 0, sizeof(T));
    memcpy(T.c, h_cameras, sizeof(double) * CAM_RECORD * (size_t)C);
    int64_t b = 0;
    while (b < B) {
        cam_sets S;
        memset(&S, 0, sizeof(S));
        int blocks = 0;
        while (b < B && S.nsets < CAM_SETS) {
            const int64_t cnt = h_offsets[b + 1] - h_offsets[b];
            if (cnt > 0) {
                S.blk[S.nsets] = blocks;
                S.first[S.nsets] = (int)h_offsets[b];
                S.count[S.nsets] = (int)cnt;
                S.cam[S.nsets] = h_cam_index ? h_cam_index[b] : 0;
                blocks += (int)((cnt + CAM_LANES - 1) / CAM_LANES);
                S.nsets++;
            }
            b++;
        }
        if (S.nsets == 0) break;
        for (int k = S.nsets; k <= CAM_SETS; k++) S.blk[k] = blocks;
        cam_points_kernel<<<(unsigned)blocks, CAM_LANES, 0, ctx->stream>>>(S, T, dir, iterations, d_px, d_px_out, d_norm, d_status);
        SLAM_HIP(hipGetLastError());
    }
    return SLAM_OK;
}

extern "C" int slam_cam_undistort_f64(slam_ctx* ctx, int64_t B, const int64_t* h_offsets, int64_t C, const double* h_cameras,
                                      const int32_t* h_cam_index, int iterations, const double* d_px, double* d_px_out, double* d_norm,
                                      uint8_t* d_status) {
    return cam_points(ctx, "slam_cam_undistort_f64", 0, B, h_offsets, C, h_cameras, h_cam_index, iterations, d_px, d_px_out, d_norm, d_status);
}

extern "C" int slam_cam_distort_f64(slam_ctx* ctx, int64_t B, const int64_t* h_offsets, int64_t C, const double* h_cameras,
                                    const int32_t* h_cam_index, const double* d_px, double* d_px_out, double* d_norm, uint8_t* d_status) {
    return cam_points(ctx, "slam_cam_distort_f64", 1, B, h_offsets, C, h_cameras, h_cam_index, 0, d_px, d_px_out, d_norm, d_status);
}

extern "C" int slam_cam_rectify_map(slam_ctx* ctx, const double* h_camera, const double* h_R, const double* h_new_K, int64_t Wd, int64_t Hd,
                                    int32_t* d_map) {
    SLAM_REQUIRE(ctx, "slam_cam_rectify_map: null ctx");
    SLAM_REQUIRE(h_camera && h_new_K, "slam_cam_rectify_map: null host pointer");
    SLAM_REQUIRE(Wd >= 1 && Hd >= 1 && Wd <= SLAM_CAM_SIDE_MAX && Hd <= SLAM_CAM_SIDE_MAX, "slam_cam_rectify_map: the destination %lld x %lld must be in [1, %d]",
                 (long long)Wd, (long long)Hd, SLAM_CAM_SIDE_MAX);
    const int bad = cam_record_check(h_camera);
    SLAM_REQUIRE(bad == 0, "slam_cam_rectify_map: camera: %s",
                 bad == 1 ? "a value is not finite" : bad == 2 ? "fx and fy must be positive" : "the model must be 0, 1 or 2");
    SLAM_REQUIRE(h_new_K[0] > 0.0 && h_new_K[1] > 0.0 && h_new_K[0] <= CAM_DBL_MAX && h_new_K[1] <= CAM_DBL_MAX && fabs(h_new_K[2]) <= CAM_DBL_MAX &&
                     fabs(h_new_K[3]) <= CAM_DBL_MAX,
                 "slam_cam_rectify_map: the new focal lengths must be positive and the new intrinsics finite");
    cam_view V;
    memset(&V, 0, sizeof(V));
    memcpy(&V.c, h_camera, sizeof(double) * CAM_RECORD);
    for (int k = 0; k < 9; k++) {
        V.R[k] = h_R ? h_R[k] : (k % 4 == 0 ? 1.0 : 0.0);
        SLAM_REQUIRE(fabs(V.R[k]) <= CAM_DBL_MAX, "slam_cam_rectify_map: R is not finite");
    }
    V.nfx = h_new_K[0]; V.nfy = h_new_K[1]; V.ncx = h_new_K[2]; V.ncy = h_new_K[3];
    SLAM_REQUIRE(d_map && ((uintptr_t)d_map & 7) == 0, "slam_cam_rectify_map: d_map must be a device pointer aligned to 8 bytes");
    SLAM_HIP(hipSetDevice(ctx->device));
    const dim3 grid((unsigned)((Wd + 63) / 64), (unsigned)((Hd + 3) / 4));
    cam_map_kernel<<<grid, dim3(64, 4), 0, ctx->stream>>>(V, (int)Wd, (int)Hd, d_map);
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

extern "C" int slam_cam_remap_u8(slam_ctx* ctx, const uint8_t* d_src, int64_t B, int64_t Hs, int64_t Ws, int64_t src_pitch, int64_t src_stride,
                                 const int32_t* d_map, int64_t Hd, int64_t Wd, int border, uint8_t* d_dst, int64_t dst_pitch, int64_t dst_stride,
                                 uint8_t* d_mask) {
    SLAM_REQUIRE(ctx, "slam_cam_remap_u8: null ctx");
    SLAM_REQUIRE(B >= 0 && B <= (1 << 20), "slam_cam_remap_u8: B=%lld must be in [0, 2^20]", (long long)B);
    SLAM_REQUIRE(Hs >= 1 && Ws >= 1 && Hd >= 1 && Wd >= 1 && Hs <= SLAM_CAM_SIDE_MAX && Ws <= SLAM_CAM_SIDE_MAX && Hd <= SLAM_CAM_SIDE_MAX &&
                     Wd <= SLAM_CAM_SIDE_MAX,
                 "slam_cam_remap_u8: image sides must be in [1, %d] (source %lld x %lld, destination %lld x %lld)", SLAM_CAM_SIDE_MAX, (long long)Ws,
                 (long long)Hs, (long long)Wd, (long long)Hd);
    SLAM_REQUIRE(src_pitch >= Ws && dst_pitch >= Wd && src_pitch <= (1 << 20) && dst_pitch <= (1 << 20), "slam_cam_remap_u8: a pitch is below its width (or above 2^20)");
    SLAM_REQUIRE(src_stride >= src_pitch * (Hs - 1) + Ws && dst_stride >= dst_pitch * (Hd - 1) + Wd && src_stride <= ((int64_t)1 << 36) &&
                     dst_stride <= ((int64_t)1 << 36),
                 "slam_cam_remap_u8: an image stride is below its image (or above 2^36)");
    SLAM_REQUIRE(border >= 0 && border <= 255, "slam_cam_remap_u8: border=%d must be in [0, 255]", border);
    if (B == 0) return SLAM_OK;
    SLAM_REQUIRE(d_src && d_map && d_dst, "slam_cam_remap_u8: null device pointer");
    SLAM_REQUIRE(((uintptr_t)d_map & 7) == 0, "slam_cam_remap_u8: d_map must be aligned to 8 bytes");
    const uint64_t src_bytes = (uint64_t)((B - 1) * src_stride + (Hs - 1) * src_pitch + Ws), dst_bytes = (uint64_t)((B - 1) * dst_stride + (Hd - 1) * dst_pitch + Wd);
    SLAM_REQUIRE(!cam_overlap(d_src, src_bytes, d_dst, dst_bytes) && !cam_overlap(d_src, src_bytes, d_mask, dst_bytes) &&
                     !cam_overlap(d_dst, dst_bytes, d_mask, dst_bytes),
                 "slam_cam_remap_u8: source, destination and mask must not overlap");
    SLAM_HIP(hipSetDevice(ctx->device));
    const int words = ((((uintptr_t)d_dst | (uintptr_t)d_mask) & 3) == 0 && dst_pitch % 4 == 0 && dst_stride % 4 == 0) ? 1 : 0;
    const int64_t lanes_x = (Wd + 3) / 4;
    const int64_t groups = ((lanes_x + 63) / 64) * ((Hd + 3) / 4);
    // about 4096 workgroups, as far as the images allow: a lane reads its map entries once and walks B / z images with them.
    // 64 frames of 752 x 480 (profiles/camera_remap_ab.log): 94 us at 1024, 80 us at 4096 and 8192, 88 us at one image per lane.
    const int64_t target = 4096;
    int64_t z = groups >= target ? 1 : (target + groups - 1) / groups;
    if (z > B) z = B;
    if (z > 65535) z = 65535;
    const dim3 grid((unsigned)((lanes_x + 63) / 64), (unsigned)((Hd + 3) / 4), (unsigned)z);
    cam_remap_kernel<<<grid, dim3(64, 4), 0, ctx->stream>>>(d_src, (int)B, (int)Hs, (int)Ws, src_pitch, src_stride, d_map, (int)Hd, (int)Wd, border,
                                                           d_dst, dst_pitch, dst_stride, d_mask, words);
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}
