// pnp_twin.cpp — the host twin of csrc/pnp.hip (test infrastructure).
//
// Includes the kernel file itself with PNP_HOST_ONLY defined: every pnp_* routine below IS the device routine's source,
// compiled for the host with contraction off and no FMA instructions available (x86-64 baseline), so a result here is what
// the device must give bit for bit.  On top of the routines: a restatement of the RANSAC loop (argmax by the kernel's own key,
// geo_key3 of geometry_common.h, hypotheses one after the other) and one C entry per device call.
//
// Built twice by tests/pnp_twin.py: a shared library (loaded through ctypes) and, with PNP_TWIN_MAIN and
// -fsanitize=address,undefined, a stand-alone program that reads a job file and writes a result file.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define PNP_HOST_ONLY
#define __host__
#define __device__
#define __forceinline__ inline
#include "../slam-experiments_amd/csrc/pnp.hip"

extern "C" {

// X [S,3,3], x [S,3,2]; pose [S,4,12] (unused slots zero), nsol [S]
int pnpt_p3p(int64_t S, const double* X, const double* x, double* pose, int32_t* nsol) {
    for (int64_t s = 0; s < S; s++) nsol[s] = pnp_p3p(X + 9 * s, x + 6 * s, pose + 48 * s);
    return 0;
}

void pnpt_draw_sample(uint64_t seed, int h, int n, int32_t* idx) {
    int v[3] = {0, 0, 0};
    pnp_draw_sample(seed, h, n, v);
    for (int k = 0; k < 3; k++) idx[k] = v[k];
}

void pnpt_inlier(const double* T, int64_t n, const double* X, const double* px, double fx, double fy, double cx, double cy,
                 double threshold_px, uint8_t* out) {
    const pnp_cam cam = {fx, fy, cx, cy};
    const double thr2 = threshold_px * threshold_px;
    for (int64_t i = 0; i < n; i++) out[i] = pnp_inlier(T, X[3 * i], X[3 * i + 1], X[3 * i + 2], px[2 * i], px[2 * i + 1], cam, thr2) ? 1 : 0;
}

// slam_pnp_ransac_f64 for one candidate of n correspondences, every hypothesis 0 .. H-1 solved and scored in turn;
// counts (or null) int32 [H,4]: the exact inlier count of every (hypothesis, solution), -1 where there is no solution
int pnpt_ransac(int64_t n64, const double* X, const double* px, double fx, double fy, double cx, double cy, int H, double threshold_px,
                uint64_t seed, double* pose, uint8_t* inlier, int32_t* stats, int32_t* counts) {
    if (H < 1 || H > GEO_H_MAX || n64 < 0 || n64 > (1 << 28)) return -1;
    const int n = (int)n64;
    for (int k = 0; k < 12; k++) pose[k] = (k % 5 == 0) ? 1.0 : 0.0;
    for (int i = 0; i < n; i++) inlier[i] = 0;
    stats[0] = 0; stats[1] = -1; stats[2] = -1; stats[3] = 0;
    if (counts) for (int64_t i = 0; i < 4 * (int64_t)H; i++) counts[i] = -1;
    if (n < 3) return 0;
    const pnp_cam cam = {fx, fy, cx, cy};
    const double thr2 = threshold_px * threshold_px;
    unsigned long long best = 0ull;
    long long models = 0;
    for (int h = 0; h < H; h++) {
        double T[48];
        const int ns = pnp_solve_hypothesis(X, px, n, cam, seed, h, T);
        models += ns;
        for (int r = 0; r < ns; r++) {
            int count = 0;
            for (int i = 0; i < n; i++) count += pnp_inlier(T + 12 * r, X[3 * i], X[3 * i + 1], X[3 * i + 2], px[2 * i], px[2 * i + 1], cam, thr2) ? 1 : 0;
            if (counts) counts[4 * h + r] = count;
            const unsigned long long k = geo_key3(count, h, r);
            if (k > best) best = k;
        }
    }
    if (!best) return 0;
    const int count = geo_key_count(best), h = geo_key3_h(best), sol = geo_key3_sub(best);
    double T[48];
    pnp_solve_hypothesis(X, px, n, cam, seed, h, T);
    for (int k = 0; k < 12; k++) pose[k] = T[12 * sol + k];
    for (int i = 0; i < n; i++) inlier[i] = pnp_inlier(pose, X[3 * i], X[3 * i + 1], X[3 * i + 2], px[2 * i], px[2 * i + 1], cam, thr2) ? 1 : 0;
    stats[0] = count; stats[1] = h; stats[2] = sol; stats[3] = (int32_t)models;
    return 0;
}

}  // extern "C"

#ifdef PNP_TWIN_MAIN
// pnp_twin_san <job file> <result file>.  Job: int64 kind, then
//   kind 0 (solver):    int64 S, X [S,9], x [S,6] -> nsol int32 [S], pose [S,48]
//   kind 1 (candidate): int64 n, int64 H, uint64 seed, double fx fy cx cy threshold, X [n,3], px [n,2]
//                       -> pose [12], stats int32 [4], mask [n]
// all native-endian, doubles unless said otherwise.  Exit 0 on success; a sanitizer report ends the run non-zero.
static bool rd(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }
int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s job result\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    int64_t kind = -1;
    bool ok = rd(in, &kind, 8);
    std::vector<char> out;
    auto put = [&](const void* p, size_t bytes) { out.insert(out.end(), (const char*)p, (const char*)p + bytes); };
    if (ok && kind == 0) {
        int64_t S = 0;
        ok = rd(in, &S, 8) && S >= 0 && S <= (1 << 24);
        std::vector<double> X(ok ? 9 * (size_t)S : 0), x(ok ? 6 * (size_t)S : 0), pose(ok ? 48 * (size_t)S : 0);
        std::vector<int32_t> ns(ok ? (size_t)S : 0);
        ok = ok && rd(in, X.data(), 8 * X.size()) && rd(in, x.data(), 8 * x.size());
        if (ok) {
            pnpt_p3p(S, X.data(), x.data(), pose.data(), ns.data());
            put(ns.data(), 4 * ns.size());
            put(pose.data(), 8 * pose.size());
        }
    } else if (ok && kind == 1) {
        int64_t n = 0, H = 0;
        uint64_t seed = 0;
        double p[5];
        ok = rd(in, &n, 8) && rd(in, &H, 8) && rd(in, &seed, 8) && rd(in, p, 40) && n >= 0 && n <= (1 << 24);
        std::vector<double> X(ok ? 3 * (size_t)n : 0), px(ok ? 2 * (size_t)n : 0);
        ok = ok && rd(in, X.data(), 8 * X.size()) && rd(in, px.data(), 8 * px.size());
        if (ok) {
            double pose[12];
            int32_t st[4];
            std::vector<uint8_t> mask((size_t)n);
            ok = pnpt_ransac(n, X.data(), px.data(), p[0], p[1], p[2], p[3], (int)H, p[4], seed, pose, mask.data(), st, nullptr) == 0;
            put(pose, 96); put(st, 16); put(mask.data(), mask.size());
        }
    } else {
        ok = false;
    }
    fclose(in);
    if (!ok) { fprintf(stderr, "bad job file\n"); return 2; }
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    const bool wrote = out.empty() || fwrite(out.data(), 1, out.size(), o) == out.size();
    return (fclose(o) == 0 && wrote) ? 0 : 2;
}
#endif
