// hg_twin.cpp — the host twin of csrc/homography.hip (test infrastructure).
//
// Includes the kernel file itself with HG_HOST_ONLY defined: every hg_* routine below IS the device routine's source,
// compiled for the host with contraction off and no FMA instructions available (x86-64 baseline), so a result here is what
// the device must give bit for bit.  On top of the routines: a restatement of the RANSAC loop (argmax by the same key,
// hypotheses one after the other), of the two votes of the decomposition and of the score sums, one C entry per device call.
//
// Built twice by tests/hg_twin.py: a shared library (loaded through ctypes) and, with HG_TWIN_MAIN and
// -fsanitize=address,undefined, a stand-alone program that reads a job file and writes a result file.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define HG_HOST_ONLY
#define __host__
#define __device__
#define __forceinline__ inline
#include "../slam-experiments_amd/csrc/homography.hip"

extern "C" {

// p1, p2 [S,4,2]; H [S,9], ok [S]
int hgt_fourpoint(int64_t S, const double* p1, const double* p2, double* H, int32_t* ok) {
    for (int64_t s = 0; s < S; s++) ok[s] = hg_fourpoint(p1 + 8 * s, p2 + 8 * s, H + 9 * s) ? 1 : 0;
    return 0;
}

void hgt_draw_sample(uint64_t seed, int h, int n, int32_t* idx) {
    int v[4] = {0, 0, 0, 0};
    hg_draw_sample(seed, h, n, v);
    for (int k = 0; k < 4; k++) idx[k] = v[k];
}

void hgt_inlier(const double* H, int64_t n, const double* px1, const double* px2, double threshold_px, uint8_t* out) {
    const double thr2 = threshold_px * threshold_px;
    for (int64_t i = 0; i < n; i++) out[i] = hg_inlier(H, px1[2 * i], px1[2 * i + 1], px2[2 * i], px2[2 * i + 1], thr2) ? 1 : 0;
}

// slam_hg_ransac_f64 for one pair of n matches, every hypothesis 0 .. H-1 solved and scored in turn; counts (or null)
// int32 [H]: the exact inlier count of every hypothesis, -1 where it has no model
int hgt_ransac(int64_t n64, const double* px1, const double* px2, int H, double threshold_px, uint64_t seed, double* Hout, uint8_t* inlier,
               int32_t* stats, int32_t* counts) {
    if (H < 1 || H > HG_H_MAX || n64 < 0 || n64 > (1 << 28)) return -1;
    const int n = (int)n64;
    for (int k = 0; k < 9; k++) Hout[k] = 0.0;
    for (int i = 0; i < n; i++) inlier[i] = 0;
    stats[0] = 0; stats[1] = -1; stats[2] = -1; stats[3] = 0;
    if (counts) for (int h = 0; h < H; h++) counts[h] = -1;
    if (n < 4) return 0;
    const double thr2 = threshold_px * threshold_px;
    unsigned long long best = 0ull;
    int models = 0;
    for (int h = 0; h < H; h++) {
        double T[9];
        if (!hg_solve_hypothesis(px1, px2, n, seed, h, T)) continue;
        models++;
        int count = 0;
        for (int i = 0; i < n; i++) count += hg_inlier(T, px1[2 * i], px1[2 * i + 1], px2[2 * i], px2[2 * i + 1], thr2) ? 1 : 0;
        if (counts) counts[h] = count;
        const unsigned long long k = hg_key(count, h);
        if (k > best) best = k;
    }
    stats[3] = models;
    if (!best) return 0;
    const int count = (int)(best >> 32), h = HG_H_MAX - (int)(best & 0xFFFFFFFFull);
    hg_solve_hypothesis(px1, px2, n, seed, h, Hout);
    for (int i = 0; i < n; i++) inlier[i] = hg_inlier(Hout, px1[2 * i], px1[2 * i + 1], px2[2 * i], px2[2 * i + 1], thr2) ? 1 : 0;
    stats[0] = count; stats[1] = h; stats[2] = 0;
    return 0;
}

// slam_hg_decompose_f64 for one pair: pose_all [48], normal_all [12], count [4], pose [12], sv [3], inlier_out [n], stats [4]
int hgt_decompose(int64_t n64, const double* px1, const double* px2, double fx, double fy, double cx, double cy, const double* H,
                  const uint8_t* inlier_in, double dist, double* pose_all, double* normal_all, int32_t* count, double* pose, double* sv,
                  uint8_t* inlier_out, int32_t* stats) {
    if (n64 < 0 || n64 > (1 << 28)) return -1;
    const int n = (int)n64;
    const hg_cam cam = {fx, fy, cx, cy};
    for (int i = 0; i < 48; i++) pose_all[i] = 0.0;
    for (int i = 0; i < 12; i++) { normal_all[i] = 0.0; pose[i] = (i % 5 == 0) ? 1.0 : 0.0; }
    for (int k = 0; k < 4; k++) count[k] = 0;
    for (int i = 0; i < n; i++) inlier_out[i] = 0;
    double Hn[9], v1[3], v3[3];
    if (!hg_singular(H, cam, Hn, sv, v1, v3)) {
        stats[0] = 0; stats[1] = -1; stats[2] = 0; stats[3] = 0;
        return 0;
    }
    double Hs[9];
    for (int t = 0; t < 9; t++) Hs[t] = Hn[t] / sv[1];
    std::vector<double> xn(4 * (size_t)n);
    for (int i = 0; i < n; i++) {
        xn[4 * i] = (px1[2 * i] - cam.cx) / cam.fx; xn[4 * i + 1] = (px1[2 * i + 1] - cam.cy) / cam.fy;
        xn[4 * i + 2] = (px2[2 * i] - cam.cx) / cam.fx; xn[4 * i + 3] = (px2[2 * i + 1] - cam.cy) / cam.fy;
    }
    int pos = 0, neg = 0;
    for (int i = 0; i < n; i++) {
        if (inlier_in && !inlier_in[i]) continue;
        const double r = hg_bilinear(Hs, xn[4 * i], xn[4 * i + 1], xn[4 * i + 2], xn[4 * i + 3]);
        pos += r > 0.0 ? 1 : 0;
        neg += r < 0.0 ? 1 : 0;
    }
    if (neg > pos) for (int t = 0; t < 9; t++) Hs[t] = -Hs[t];
    if ((sv[0] - sv[2]) / sv[1] < HG_ROTATION_ONLY) {
        double R[9];
        hg_nearest_rotation(Hs, v1, v3, R);
        for (int i = 0; i < 12; i++) pose[i] = pose_all[i] = (i & 3) == 3 ? 0.0 : R[3 * (i >> 2) + (i & 3)];
        stats[0] = 0; stats[1] = -2; stats[2] = 0; stats[3] = 1;
        return 0;
    }
    hg_candidates(Hs, sv[0] / sv[1], sv[2] / sv[1], v1, v3, pose_all, normal_all);
    for (int i = 0; i < n; i++) {
        if (inlier_in && !inlier_in[i]) continue;
        for (int k = 0; k < 4; k++) count[k] += hg_cheirality(pose_all + 12 * k, xn[4 * i], xn[4 * i + 1], xn[4 * i + 2], xn[4 * i + 3], dist) ? 1 : 0;
    }
    int win = 0, second = 0;
    for (int k = 1; k < 4; k++)
        if (count[k] > count[win]) win = k;
    for (int k = 0; k < 4; k++)
        if (k != win && count[k] > second) second = count[k];
    for (int i = 0; i < 12; i++) pose[i] = pose_all[12 * win + i];
    for (int i = 0; i < n; i++) {
        if (inlier_in && !inlier_in[i]) continue;
        inlier_out[i] = hg_cheirality(pose, xn[4 * i], xn[4 * i + 1], xn[4 * i + 2], xn[4 * i + 3], dist) ? 1 : 0;
    }
    stats[0] = count[win]; stats[1] = win; stats[2] = second; stats[3] = 4;
    return 0;
}

// slam_hg_model_score_f64 for one pair: score int64 [2], ratio [1]
int hgt_model_score(int64_t n, const double* px1, const double* px2, double fx, double fy, double cx, double cy, const double* H,
                    const double* E, double sigma, int64_t* score, double* ratio) {
    const hg_cam cam = {fx, fy, cx, cy};
    double Hi[9], F[9];
    hg_adjugate(H, Hi);
    hg_fundamental(E, cam, F);
    long long sh = 0, se = 0;
    for (int64_t i = 0; i < n; i++) hg_score_match(H, Hi, F, px1[2 * i], px1[2 * i + 1], px2[2 * i], px2[2 * i + 1], sigma * sigma, &sh, &se);
    score[0] = sh; score[1] = se;
    *ratio = hg_ratio(sh, se);
    return 0;
}

}  // extern "C"

#ifdef HG_TWIN_MAIN
// hg_twin_san <job file> <result file>.  Job: int64 kind, then
//   kind 0 (solver): int64 S, p1 [S,8], p2 [S,8] -> ok int32 [S], H [S,9]
//   kind 1 (pair):   int64 n, int64 H, uint64 seed, double fx fy cx cy threshold_h distance sigma, E [9], px1 [n,2], px2 [n,2]
//                    -> the RANSAC (H [9], stats int32 [4], mask [n]), then the decomposition of that H on its inliers
//                       (pose_all [48], normal_all [12], pose [12], sv [3], count int32 [4], stats int32 [4], good [n]), then the
//                       scores of that H against E (score int64 [2], ratio)
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
        std::vector<double> p1(ok ? 8 * (size_t)S : 0), p2(ok ? 8 * (size_t)S : 0), H(ok ? 9 * (size_t)S : 0);
        std::vector<int32_t> good(ok ? (size_t)S : 0);
        ok = ok && rd(in, p1.data(), 8 * p1.size()) && rd(in, p2.data(), 8 * p2.size());
        if (ok) {
            hgt_fourpoint(S, p1.data(), p2.data(), H.data(), good.data());
            put(good.data(), 4 * good.size());
            put(H.data(), 8 * H.size());
        }
    } else if (ok && kind == 1) {
        int64_t n = 0, H = 0;
        uint64_t seed = 0;
        double p[7], E[9];
        ok = rd(in, &n, 8) && rd(in, &H, 8) && rd(in, &seed, 8) && rd(in, p, 56) && rd(in, E, 72) && n >= 0 && n <= (1 << 24);
        std::vector<double> px1(ok ? 2 * (size_t)n : 0), px2(ok ? 2 * (size_t)n : 0);
        ok = ok && rd(in, px1.data(), 8 * px1.size()) && rd(in, px2.data(), 8 * px2.size());
        if (ok) {
            double Hm[9], pose_all[48], normal_all[12], pose[12], sv[3], ratio;
            int32_t st[4], cnt[4], st2[4];
            int64_t score[2];
            std::vector<uint8_t> mask((size_t)n), good((size_t)n);
            ok = hgt_ransac(n, px1.data(), px2.data(), (int)H, p[4], seed, Hm, mask.data(), st, nullptr) == 0 &&
                 hgt_decompose(n, px1.data(), px2.data(), p[0], p[1], p[2], p[3], Hm, mask.data(), p[5], pose_all, normal_all, cnt, pose, sv,
                               good.data(), st2) == 0 &&
                 hgt_model_score(n, px1.data(), px2.data(), p[0], p[1], p[2], p[3], Hm, E, p[6], score, &ratio) == 0;
            put(Hm, 72); put(st, 16); put(mask.data(), mask.size());
            put(pose_all, 384); put(normal_all, 96); put(pose, 96); put(sv, 24); put(cnt, 16); put(st2, 16); put(good.data(), good.size());
            put(score, 16); put(&ratio, 8);
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
