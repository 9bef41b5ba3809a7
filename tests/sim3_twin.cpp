// sim3_twin.cpp — the host twin of csrc/sim3.hip (test infrastructure).
//
// Includes the kernel file itself with SIM3_HOST_ONLY defined: every s3_* routine below IS the device routine's source,
// compiled for the host with contraction off and no FMA instructions available (x86-64 baseline), so a result here is what
// the device must give bit for bit.  On top of the routines: a restatement of the RANSAC loop (argmax by the same key,
// hypotheses one after the other), a restatement of the refit's summation order (256 lanes, each over its positions in
// ascending order, then the tree) and one C entry per device call.
//
// Built twice by tests/sim3_twin.py: a shared library (loaded through ctypes) and, with SIM3_TWIN_MAIN and
// -fsanitize=address,undefined, a stand-alone program that reads a job file and writes a result file.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define SIM3_HOST_ONLY
#define __host__
#define __device__
#define __forceinline__ inline
#include "../slam-experiments_amd/csrc/sim3.hip"

namespace {
const int LANES = 256;               // S3_REFIT_THREADS, restated

// the tree of the header: for stride = 128, 64, ..., 1: lane l < stride adds lane l + stride to its own
void tree(std::vector<double>& s, int K) {
    for (int stride = LANES / 2; stride >= 1; stride >>= 1)
        for (int l = 0; l < stride; l++)
            for (int k = 0; k < K; k++) s[(size_t)l * K + k] += s[(size_t)(l + stride) * K + k];
}
void stage(const double* X1, const double* X2, const double* sigma2, int64_t i, const s3_cam& cam, double chi2, double* c) {
    s3_stage(X1 + 3 * i, X2 + 3 * i, sigma2 ? sigma2[2 * i] : 1.0, sigma2 ? sigma2[2 * i + 1] : 1.0, cam, chi2, c);
}
}  // namespace

extern "C" {

// X1, X2 [S,3,3]; model [S,13], ok [S]
int s3t_threepoint(int64_t S, const double* X1, const double* X2, int fix_scale, double* model, int32_t* ok) {
    for (int64_t s = 0; s < S; s++) ok[s] = s3_threepoint(X1 + 9 * s, X2 + 9 * s, fix_scale != 0, model + 13 * s) ? 1 : 0;
    return 0;
}

void s3t_draw_sample(uint64_t seed, int h, int n, int32_t* idx) {
    int v[3] = {0, 0, 0};
    s3_draw_sample(seed, h, n, v);
    for (int k = 0; k < 3; k++) idx[k] = v[k];
}

void s3t_inlier(const double* model, int64_t n, const double* X1, const double* X2, const double* sigma2, double fx, double fy, double cx,
                double cy, double chi2, uint8_t* out) {
    const s3_cam cam = {fx, fy, cx, cy};
    double m[21], c[12];
    s3_scoring_form(model, true, m);
    for (int64_t i = 0; i < n; i++) {
        stage(X1, X2, sigma2, i, cam, chi2, c);
        out[i] = s3_inlier(m, c, cam) ? 1 : 0;
    }
}

// slam_sim3_ransac_f64 for one candidate of n correspondences, every hypothesis 0 .. H-1 solved and scored in turn;
// counts (or null) int32 [H]: the exact inlier count of every hypothesis, -1 where it has no model
int s3t_ransac(int64_t n64, const double* X1, const double* X2, const double* sigma2, double fx, double fy, double cx, double cy, int H,
               double chi2, int fix_scale, uint64_t seed, double* model, uint8_t* inlier, int32_t* stats, int32_t* counts) {
    if (H < 1 || H > GEO_H_MAX || n64 < 0 || n64 > (1 << 28)) return -1;
    const int n = (int)n64;
    s3_identity(model);
    for (int i = 0; i < n; i++) inlier[i] = 0;
    stats[0] = 0; stats[1] = -1; stats[2] = -1; stats[3] = 0;
    if (counts) for (int h = 0; h < H; h++) counts[h] = -1;
    if (n < 3) return 0;
    const s3_cam cam = {fx, fy, cx, cy};
    std::vector<double> c((size_t)n * 12);
    for (int i = 0; i < n; i++) stage(X1, X2, sigma2, i, cam, chi2, c.data() + 12 * (size_t)i);
    unsigned long long best = 0ull;
    int models = 0;
    double m[21], cand[13];
    for (int h = 0; h < H; h++) {
        if (!s3_solve_hypothesis(X1, X2, n, fix_scale != 0, seed, h, cand)) continue;
        models++;
        s3_scoring_form(cand, true, m);
        int count = 0;
        for (int i = 0; i < n; i++) count += s3_inlier(m, c.data() + 12 * (size_t)i, cam) ? 1 : 0;
        if (counts) counts[h] = count;
        const unsigned long long k = geo_key2(count, h);
        if (k > best) best = k;
    }
    if (!best) return 0;
    const int count = geo_key_count(best), h = geo_key2_h(best);
    s3_solve_hypothesis(X1, X2, n, fix_scale != 0, seed, h, model);
    s3_scoring_form(model, true, m);
    for (int i = 0; i < n; i++) inlier[i] = s3_inlier(m, c.data() + 12 * (size_t)i, cam) ? 1 : 0;
    stats[0] = count; stats[1] = h; stats[2] = 0; stats[3] = models;
    return 0;
}

// slam_sim3_refit_f64 for one candidate: mask uint8 [n] or null; model [13], stats [2] = {points used, ok}
int s3t_refit(int64_t n, const double* X1, const double* X2, const uint8_t* mask, int fix_scale, double* model, int32_t* stats) {
    if (n < 0 || n > (1 << 28)) return -1;
    std::vector<double> a((size_t)LANES * 6, 0.0), b((size_t)LANES * 11, 0.0);
    int used = 0;
    for (int l = 0; l < LANES; l++)
        for (int64_t i = l; i < n; i += LANES) {
            if (mask && !mask[i]) continue;
            s3_acc_points(a.data() + 6 * (size_t)l, X1 + 3 * i, X2 + 3 * i);
            used++;
        }
    tree(a, 6);
    double c[6];
    for (int k = 0; k < 6; k++) c[k] = a[k] / (double)used;
    for (int l = 0; l < LANES; l++)
        for (int64_t i = l; i < n; i += LANES) {
            if (mask && !mask[i]) continue;
            s3_acc_centred(b.data() + 11 * (size_t)l, X1 + 3 * i, X2 + 3 * i, c);
        }
    tree(b, 11);
    stats[0] = used;
    stats[1] = s3_refit_model(used, c, b.data(), fix_scale != 0, model) ? 1 : 0;
    return 0;
}

}  // extern "C"

#ifdef SIM3_TWIN_MAIN
// sim3_twin_san <job file> <result file>.  Job: int64 kind, then
//   kind 0 (solver):    int64 S, int64 fix_scale, X1 [S,9], X2 [S,9] -> ok int32 [S], model [S,13]
//   kind 1 (candidate): int64 n, int64 H, uint64 seed, int64 fix_scale, int64 has_sigma, double fx fy cx cy chi2, X1 [n,3],
//                       X2 [n,3], sigma2 [n,2] if has_sigma -> model [13], stats int32 [4], mask [n]
//   kind 2 (refit):     int64 n, int64 fix_scale, int64 has_mask, X1 [n,3], X2 [n,3], mask uint8 [n] if has_mask
//                       -> model [13], stats int32 [2]
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
        int64_t S = 0, fix = 0;
        ok = rd(in, &S, 8) && rd(in, &fix, 8) && S >= 0 && S <= (1 << 24);
        std::vector<double> X1(ok ? 9 * (size_t)S : 0), X2(ok ? 9 * (size_t)S : 0), model(ok ? 13 * (size_t)S : 0);
        std::vector<int32_t> good(ok ? (size_t)S : 0);
        ok = ok && rd(in, X1.data(), 8 * X1.size()) && rd(in, X2.data(), 8 * X2.size());
        if (ok) {
            s3t_threepoint(S, X1.data(), X2.data(), (int)fix, model.data(), good.data());
            put(good.data(), 4 * good.size());
            put(model.data(), 8 * model.size());
        }
    } else if (ok && kind == 1) {
        int64_t n = 0, H = 0, fix = 0, has = 0;
        uint64_t seed = 0;
        double p[5];
        ok = rd(in, &n, 8) && rd(in, &H, 8) && rd(in, &seed, 8) && rd(in, &fix, 8) && rd(in, &has, 8) && rd(in, p, 40) && n >= 0 && n <= (1 << 24);
        std::vector<double> X1(ok ? 3 * (size_t)n : 0), X2(ok ? 3 * (size_t)n : 0), sg(ok && has ? 2 * (size_t)n : 0);
        ok = ok && rd(in, X1.data(), 8 * X1.size()) && rd(in, X2.data(), 8 * X2.size()) && rd(in, sg.data(), 8 * sg.size());
        if (ok) {
            double model[13];
            int32_t st[4];
            std::vector<uint8_t> mask((size_t)n);
            ok = s3t_ransac(n, X1.data(), X2.data(), has ? sg.data() : nullptr, p[0], p[1], p[2], p[3], (int)H, p[4], (int)fix, seed, model,
                            mask.data(), st, nullptr) == 0;
            put(model, 104); put(st, 16); put(mask.data(), mask.size());
        }
    } else if (ok && kind == 2) {
        int64_t n = 0, fix = 0, has = 0;
        ok = rd(in, &n, 8) && rd(in, &fix, 8) && rd(in, &has, 8) && n >= 0 && n <= (1 << 24);
        std::vector<double> X1(ok ? 3 * (size_t)n : 0), X2(ok ? 3 * (size_t)n : 0);
        std::vector<uint8_t> mask(ok && has ? (size_t)n : 0);
        ok = ok && rd(in, X1.data(), 8 * X1.size()) && rd(in, X2.data(), 8 * X2.size()) && rd(in, mask.data(), mask.size());
        if (ok) {
            double model[13];
            int32_t st[2];
            ok = s3t_refit(n, X1.data(), X2.data(), has ? mask.data() : nullptr, (int)fix, model, st) == 0;
            put(model, 104); put(st, 8);
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
