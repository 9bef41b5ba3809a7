// two_view_twin.cpp — the host twin of csrc/two_view.hip (test infrastructure).
//
// Includes the kernel file itself with TV_HOST_ONLY defined: every tv_* routine below IS the device routine's source,
// compiled for the host with contraction off and no FMA instructions available (x86-64 baseline), so a result here is
// what the device must give bit for bit if "a pure function of its inputs whatever it is inlined into" holds.  The
// "LDS" is a host array with the kernel's own lane stride (TV_LANES); lane 0 is used.  On top of the routines: a
// restatement of the RANSAC (argmax by the kernel's own key, geo_key3 of geometry_common.h, hypotheses in any order) and
// of the recoverPose vote.
//
// Built twice by oracle/Makefile: libtvtwin.so (bound in oracle.py) and tv_twin_san, a stand-alone program with
// -fsanitize=undefined,address that reads a job file and writes a result file (TV_TWIN_MAIN).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <vector>

#define TV_HOST_ONLY
#define __host__
#define __device__
#define __forceinline__ inline
#include "../slam-experiments_amd/csrc/two_view.hip"

namespace {
struct Lds {
    std::vector<double> mem;
    explicit Lds(double fill) : mem((size_t)TV_LDS_PER_LANE * TV_LANES, fill) {}
    double* lane0() { return mem.data(); }
};
double g_fill = 0.0;          // what the "LDS" holds before a solve (the device's is whatever the last block left)

double now_s() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}
int solve_hypothesis(double* lds, const double* xn, int n, uint64_t seed, int h) {
    int idx[5];
    tv_draw_sample(seed, h, n, idx);
    double p1[10], p2[10];
    for (int k = 0; k < 5; k++) {
        const double* v = xn + 4 * (size_t)idx[k];
        p1[2 * k] = v[0]; p1[2 * k + 1] = v[1]; p2[2 * k] = v[2]; p2[2 * k + 1] = v[3];
    }
    return tv_solve(lds, p1, p2);
}
}  // namespace

extern "C" {

void tvt_set_fill(double v) { g_fill = v; }

// x1, x2 [S,5,2]; E [S,10,9] (unused slots zero), nroots [S]; seconds [S] or null: wall time of each solve
int tvt_solve(int64_t S, const double* x1, const double* x2, double* E, int32_t* nroots, double* seconds) {
    for (int64_t s = 0; s < S; s++) {
        Lds l(g_fill);
        double* lds = l.lane0();
        const double t0 = seconds ? now_s() : 0.0;
        const int n = tv_solve(lds, x1 + 10 * s, x2 + 10 * s);
        if (seconds) seconds[s] = now_s() - t0;
        nroots[s] = n;
        for (int i = 0; i < 90; i++) E[90 * s + i] = i < 9 * n ? TVL(TV_EOUT + i) : 0.0;
    }
    return 0;
}

// the lane's TV_LDS_PER_LANE doubles after each of the five routines before tv_assemble (dump [5,236]), the number of
// polynomial roots (*nz) and the result as tvt_solve gives it: to find the first routine whose output differs
int tvt_solve_stages(const double* x1, const double* x2, double* dump, int32_t* nz, double* E, int32_t* nroots) {
    Lds l(g_fill);
    double* lds = l.lane0();
    auto snap = [&](int k) { for (int i = 0; i < TV_LDS_PER_LANE; i++) dump[k * TV_LDS_PER_LANE + i] = TVL(i); };
    tv_null_space(lds, x1, x2, false); snap(0);
    tv_constraints(lds); snap(1);
    if (tv_eliminate(lds) < TV_PIVOT_MIN) {              // as tv_solve: the dumps are then those of the second basis
        tv_null_space(lds, x1, x2, true); snap(0);
        tv_constraints(lds); snap(1);
        tv_eliminate(lds);
    }
    snap(2);
    tv_bpoly(lds); snap(3);
    *nz = tv_real_roots(lds); snap(4);
    const int n = tv_assemble(lds, *nz);
    *nroots = n;
    for (int i = 0; i < 90; i++) E[i] = i < 9 * n ? TVL(TV_EOUT + i) : 0.0;
    return 0;
}

void tvt_sampson_sq(const double* E, int64_t n, const double* x1, const double* x2, double* out) {
    for (int64_t i = 0; i < n; i++) out[i] = tv_sampson_sq(E, x1[2 * i], x1[2 * i + 1], x2[2 * i], x2[2 * i + 1]);
}

void tvt_draw_sample(uint64_t seed, int h, int n, int32_t* idx) {
    int v[5];
    tv_draw_sample(seed, h, n, v);
    for (int k = 0; k < 5; k++) idx[k] = v[k];
}

void tvt_decompose(const double* E, double* R1, double* R2, double* t) { tv_decompose(E, R1, R2, t); }

void tvt_cheirality(const double* R, const double* t, int64_t n, const double* x1, const double* x2, double dist, uint8_t* good) {
    for (int64_t i = 0; i < n; i++) good[i] = tv_cheirality(R, t, x1[2 * i], x1[2 * i + 1], x2[2 * i], x2[2 * i + 1], dist) ? 1 : 0;
}

void tvt_triangulate(int64_t N, const double* P1, const double* P2, const double* x1, const double* x2, double* X, double* w) {
    for (int64_t i = 0; i < N; i++) {
        double v[4];
        tv_triangulate_point(P1, P2, x1[2 * i], x1[2 * i + 1], x2[2 * i], x2[2 * i + 1], v);
        X[3 * i] = v[0] / v[3]; X[3 * i + 1] = v[1] / v[3]; X[3 * i + 2] = v[2] / v[3];
        w[i] = v[3];
    }
}

// slam_tv_essential_ransac_f64 for one pair of n matches (pixels), every hypothesis 0 .. H-1 solved and scored in turn
int tvt_ransac(int64_t n64, const double* px1, const double* px2, double fx, double fy, double cx, double cy, int H,
               double threshold_px, uint64_t seed, double* E_out, uint8_t* inlier, int32_t* stats) {
    if (H < 1 || H > GEO_H_MAX || n64 < 0 || n64 > (1 << 28)) return -1;
    const int n = (int)n64;
    for (int t = 0; t < 9; t++) E_out[t] = 0.0;
    for (int i = 0; i < n; i++) inlier[i] = 0;
    stats[0] = 0; stats[1] = -1; stats[2] = -1; stats[3] = 0;
    if (n < 5) return 0;
    std::vector<double> xn(4 * (size_t)n);
    for (int i = 0; i < n; i++) {
        xn[4 * i] = (px1[2 * i] - cx) / fx; xn[4 * i + 1] = (px1[2 * i + 1] - cy) / fy;
        xn[4 * i + 2] = (px2[2 * i] - cx) / fx; xn[4 * i + 3] = (px2[2 * i + 1] - cy) / fy;
    }
    const double thr = threshold_px / ((fx + fy) / 2.0), thr2 = thr * thr;
    unsigned long long best = 0ull;
    long long models = 0;
#pragma omp parallel
    {
        Lds l(g_fill);
        double* lds = l.lane0();
        unsigned long long mine = 0ull;
        long long mymodels = 0;
#pragma omp for schedule(dynamic, 64) nowait
        for (int h = 0; h < H; h++) {
            const int nr = solve_hypothesis(lds, xn.data(), n, seed, h);
            mymodels += nr;
            for (int r = 0; r < nr; r++) {
                double E[9];
                for (int t = 0; t < 9; t++) E[t] = TVL(TV_EOUT + 9 * r + t);
                int count = 0;
                for (int i = 0; i < n; i++) count += tv_sampson_sq(E, xn[4 * i], xn[4 * i + 1], xn[4 * i + 2], xn[4 * i + 3]) < thr2 ? 1 : 0;
                const unsigned long long k = geo_key3(count, h, r);
                if (k > mine) mine = k;
            }
        }
#pragma omp critical
        {
            if (mine > best) best = mine;
            models += mymodels;
        }
    }
    stats[3] = (int32_t)models;
    if (!best) return 0;
    const int count = geo_key_count(best), h = geo_key3_h(best), root = geo_key3_sub(best);
    Lds l(g_fill);
    double* lds = l.lane0();
    solve_hypothesis(lds, xn.data(), n, seed, h);
    for (int t = 0; t < 9; t++) E_out[t] = TVL(TV_EOUT + 9 * root + t);
    for (int i = 0; i < n; i++) inlier[i] = tv_sampson_sq(E_out, xn[4 * i], xn[4 * i + 1], xn[4 * i + 2], xn[4 * i + 3]) < thr2 ? 1 : 0;
    stats[0] = count; stats[1] = h; stats[2] = root;
    return 0;
}

// slam_tv_recover_pose_f64 for one pair: pose [12], inlier_out [n], stats [2]; counts [4] (or null) the four votes
int tvt_recover_pose(int64_t n64, const double* px1, const double* px2, double fx, double fy, double cx, double cy, const double* E,
                     const uint8_t* inlier_in, double dist, double* pose, uint8_t* inlier_out, int32_t* stats, int32_t* counts) {
    const int n = (int)n64;
    double nrm = 0.0;
    for (int t = 0; t < 9; t++) nrm += E[t] * E[t];
    if (counts) for (int k = 0; k < 4; k++) counts[k] = 0;
    if (!(nrm > 0.0) || !isfinite(nrm)) {
        for (int k = 0; k < 12; k++) pose[k] = (k % 5 == 0) ? 1.0 : 0.0;
        for (int i = 0; i < n; i++) inlier_out[i] = 0;
        stats[0] = 0; stats[1] = -1;
        return 0;
    }
    double R1[9], R2[9], t[3], tn[3];
    tv_decompose(E, R1, R2, t);
    for (int i = 0; i < 3; i++) tn[i] = -t[i];
    int cnt[4] = {0, 0, 0, 0};
    for (int i = 0; i < n; i++) {
        if (inlier_in && !inlier_in[i]) continue;
        const double a = (px1[2 * i] - cx) / fx, b = (px1[2 * i + 1] - cy) / fy, c = (px2[2 * i] - cx) / fx, d = (px2[2 * i + 1] - cy) / fy;
        cnt[0] += tv_cheirality(R1, t, a, b, c, d, dist) ? 1 : 0;
        cnt[1] += tv_cheirality(R2, t, a, b, c, d, dist) ? 1 : 0;
        cnt[2] += tv_cheirality(R1, tn, a, b, c, d, dist) ? 1 : 0;
        cnt[3] += tv_cheirality(R2, tn, a, b, c, d, dist) ? 1 : 0;
    }
    int win = 0;
    for (int k = 1; k < 4; k++)
        if (cnt[k] > cnt[win]) win = k;
    const double* R = (win & 1) ? R2 : R1;
    const double* tt = (win & 2) ? tn : t;
    for (int i = 0; i < n; i++) {
        uint8_t good = 0;
        if (!inlier_in || inlier_in[i])
            good = tv_cheirality(R, tt, (px1[2 * i] - cx) / fx, (px1[2 * i + 1] - cy) / fy, (px2[2 * i] - cx) / fx, (px2[2 * i + 1] - cy) / fy, dist) ? 1 : 0;
        inlier_out[i] = good;
    }
    for (int k = 0; k < 12; k++) pose[k] = (k & 3) == 3 ? tt[k >> 2] : R[3 * (k >> 2) + (k & 3)];
    stats[0] = cnt[win]; stats[1] = win;
    if (counts) for (int k = 0; k < 4; k++) counts[k] = cnt[k];
    return 0;
}

}  // extern "C"

#ifdef TV_TWIN_MAIN
// tv_twin_san <job file> <result file>.  Job: int64 kind, then
//   kind 0 (solver): int64 S, x1 [S,10], x2 [S,10] -> nroots int32 [S], E [S,90]
//   kind 1 (pair):   int64 n, int64 H, uint64 seed, double fx fy cx cy threshold distance, px1 [n,2], px2 [n,2]
//                    -> E [9], stats int32 [4], mask [n], pose [12], pose stats int32 [2], good [n]
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
        std::vector<double> x1(ok ? 10 * (size_t)S : 0), x2(x1.size()), E(ok ? 90 * (size_t)S : 0);
        std::vector<int32_t> nr(ok ? (size_t)S : 0);
        ok = ok && rd(in, x1.data(), 8 * x1.size()) && rd(in, x2.data(), 8 * x2.size());
        if (ok) {
            tvt_solve(S, x1.data(), x2.data(), E.data(), nr.data(), nullptr);
            put(nr.data(), 4 * nr.size());
            put(E.data(), 8 * E.size());
        }
    } else if (ok && kind == 1) {
        int64_t n = 0, H = 0;
        uint64_t seed = 0;
        double p[6];
        ok = rd(in, &n, 8) && rd(in, &H, 8) && rd(in, &seed, 8) && rd(in, p, 48) && n >= 0 && n <= (1 << 24);
        std::vector<double> px1(ok ? 2 * (size_t)n : 0), px2(px1.size());
        ok = ok && rd(in, px1.data(), 8 * px1.size()) && rd(in, px2.data(), 8 * px2.size());
        if (ok) {
            double E[9], pose[12];
            int32_t st[4], ps[2];
            std::vector<uint8_t> mask((size_t)n), good((size_t)n);
            ok = tvt_ransac(n, px1.data(), px2.data(), p[0], p[1], p[2], p[3], (int)H, p[4], seed, E, mask.data(), st) == 0;
            tvt_recover_pose(n, px1.data(), px2.data(), p[0], p[1], p[2], p[3], E, nullptr, p[5], pose, good.data(), ps, nullptr);
            put(E, 72); put(st, 16); put(mask.data(), mask.size()); put(pose, 96); put(ps, 8); put(good.data(), good.size());
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
