// sim3_opt_twin.cpp — the host twin of csrc/sim3_opt.hip (test infrastructure).
//
// Includes the kernel file itself with SIM3_OPT_HOST_ONLY defined: every so_* routine below IS the device routine's source,
// compiled for the host with contraction off and no FMA instructions available (x86-64 baseline), so a result here is what
// the device must give bit for bit.  On top of the routines: a restatement of the summation order of the header (256 lanes,
// each over its positions in ascending order, the tree inside each group of 64 lanes, the four groups as (g0 + g1) + (g2 + g3)),
// the Levenberg-Marquardt loop and the schedule written sequentially from the header, and one C entry per thing a test asks.
//
// Built twice by tests/sim3_opt_twin.py: a shared library (loaded through ctypes) and, with SIM3_OPT_TWIN_MAIN and
// -fsanitize=address,undefined, a stand-alone program that reads a job file and writes a result file.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define SIM3_OPT_HOST_ONLY
#define __host__
#define __device__
#define __forceinline__ inline
#include "../slam-experiments_amd/csrc/sim3_opt.hip"

namespace {
const int LANES = 256, GROUP = 64;

struct problem {
    int n;
    std::vector<double> pairs;       // [n,12]
    std::vector<uint8_t> active;
    geo_cam cam;
    int fix_scale;
    long trials, evaluations;
};

// sums of K terms per active pair in the header's order; term(i, a) adds pair i's contribution to a [K]
template <int K, class F>
void ordered_sums(const problem& P, F term, double* out) {
    std::vector<double> lane((size_t)LANES * K, 0.0);
    for (int l = 0; l < LANES; l++)
        for (int i = l; i < P.n; i += LANES)
            if (P.active[i]) term(i, lane.data() + (size_t)l * K);
    for (int g = 0; g < LANES; g += GROUP)
        for (int stride = GROUP / 2; stride >= 1; stride >>= 1)
            for (int l = 0; l < stride; l++)
                for (int k = 0; k < K; k++) lane[(size_t)(g + l) * K + k] += lane[(size_t)(g + l + stride) * K + k];
    for (int k = 0; k < K; k++)
        out[k] = (lane[k] + lane[(size_t)GROUP * K + k]) + (lane[(size_t)2 * GROUP * K + k] + lane[(size_t)3 * GROUP * K + k]);
}
void linearize(problem& P, const double* model, double delta, double* sums) {
    double m[21];
    so_form(model, m);
    P.evaluations++;
    ordered_sums<SO_TERMS>(P, [&](int i, double* a) { so_acc_pair(a, m, P.pairs.data() + 12 * (size_t)i, P.cam, delta, P.fix_scale); }, sums);
}
double cost(problem& P, const double* model, double delta, bool* bad) {
    double m[21], out[1];
    so_form(model, m);
    *bad = false;
    ordered_sums<1>(P, [&](int i, double* a) { a[0] += so_cost_pair(m, P.pairs.data() + 12 * (size_t)i, P.cam, delta, bad); }, out);
    return out[0];
}
// one stage, the header's statement; true when it ended on ten failures
bool stage(problem& P, double* model, double delta, int iters, int* accepted) {
    double sums[SO_TERMS], lambda = 0.0, ni = 2.0;
    for (int it = 0; it < iters; it++) {
        linearize(P, model, delta, sums);
        if (it == 0) lambda = so_lambda0(sums);
        bool took = false;
        for (int trial = 0; trial < SO_TRIALS && !took; trial++) {
            P.trials++;
            double x[7], cand[13], rho = -1.0;
            bool ok = so_solve(sums, lambda, P.fix_scale, x);
            if (ok) {
                so_retract(model, x, cand);
                ok = so_model_ok(cand);
            }
            if (ok) {
                bool bad;
                const double c = cost(P, cand, delta, &bad);
                ok = so_finite(c) && !bad;
                rho = (sums[35] - c) / so_gain_scale(sums, lambda, x);
            }
            if (ok && rho > 0.0) {
                memcpy(model, cand, sizeof cand);
                lambda *= so_accept_factor(rho);
                ni = 2.0;
                (*accepted)++;
                took = true;
            } else {
                lambda *= ni;
                ni *= 2.0;
            }
        }
        if (!took) return true;
    }
    return false;
}
void classify(problem& P, const double* model, double th2, int* counts) {
    double m[21];
    so_form(model, m);
    counts[0] = counts[1] = 0;
    for (int i = 0; i < P.n; i++) {
        if (!P.active[i]) continue;
        so_res r;
        so_residual(m, P.pairs.data() + 12 * (size_t)i, P.cam, r);
        const bool keep = so_keep(r, th2);
        P.active[i] = keep ? 1 : 0;
        counts[keep ? 0 : 1]++;
    }
}
void gather(int64_t n, const double* X1, const double* X2, const double* px1, const double* px2, const double* sigma2, std::vector<double>& pairs) {
    pairs.resize(12 * (size_t)n);
    for (int64_t i = 0; i < n; i++) {
        double* p = pairs.data() + 12 * (size_t)i;
        for (int k = 0; k < 3; k++) { p[k] = X1[3 * i + k]; p[3 + k] = X2[3 * i + k]; }
        p[6] = px1[2 * i]; p[7] = px1[2 * i + 1]; p[8] = px2[2 * i]; p[9] = px2[2 * i + 1];
        p[10] = sigma2 ? sigma2[2 * i] : 1.0; p[11] = sigma2 ? sigma2[2 * i + 1] : 1.0;
    }
}
}  // namespace

extern "C" {

// one pair p [12] at a model: e [4] = (e2, e1), c [2] = (c1, c2), depth [2] = (z, wz), J [4,7] = (J2; J1)
void s3o_pair(const double* model, const double* p, double fx, double fy, double cx, double cy, int fix_scale, double* e, double* c, double* depth,
              double* J) {
    const geo_cam cam = {fx, fy, cx, cy};
    double m[21], J2[2][7], J1[2][7];
    so_form(model, m);
    so_res r;
    so_residual(m, p, cam, r);
    so_jacobians(m, p, r, cam, fix_scale, J2, J1);
    e[0] = r.e2[0]; e[1] = r.e2[1]; e[2] = r.e1[0]; e[3] = r.e1[1];
    c[0] = r.c1; c[1] = r.c2;
    depth[0] = r.Y[2]; depth[1] = r.W[2];
    for (int k = 0; k < 7; k++) { J[k] = J2[0][k]; J[7 + k] = J2[1][k]; J[14 + k] = J1[0][k]; J[21 + k] = J1[1][k]; }
}

void s3o_retract(const double* model, const double* x, double* out) { so_retract(model, x, out); }

// the 36 sums of a linearisation over the pairs with active != 0 (null: all), Huber width delta
int s3o_linearize(int64_t n, const double* X1, const double* X2, const double* px1, const double* px2, const double* sigma2, const uint8_t* active,
                  const double* model, double fx, double fy, double cx, double cy, double delta, int fix_scale, double* sums) {
    if (n < 0 || n > (1 << 24)) return -1;
    problem P = {(int)n, {}, std::vector<uint8_t>((size_t)n, 1), {fx, fy, cx, cy}, fix_scale != 0, 0, 0};
    gather(n, X1, X2, px1, px2, sigma2, P.pairs);
    if (active) P.active.assign(active, active + n);
    linearize(P, model, delta, sums);
    return 0;
}

// slam_sim3_optimize_f64 for one candidate of n correspondences; work (or null) int64 [2] = {trials, linearisations}
int s3o_optimize(int64_t n, const double* X1, const double* X2, const double* px1, const double* px2, const double* sigma2, const double* model_in,
                 double fx, double fy, double cx, double cy, double th2, int it0, int it_bad, int it_clean, int min_pairs, int fix_scale,
                 double* model_out, uint8_t* inlier, double* chi2, int32_t* stats, int64_t* work) {
    if (n < 0 || n > (1 << 24)) return -1;
    problem P = {(int)n, {}, std::vector<uint8_t>((size_t)n, 0), {fx, fy, cx, cy}, fix_scale != 0, 0, 0};
    gather(n, X1, X2, px1, px2, sigma2, P.pairs);
    double in[13], model[13];
    memcpy(in, model_in, sizeof in);
    memcpy(model, model_in, sizeof in);
    int status = 0, accepted = 0, counts[2] = {0, 0}, nbad = 0;
    std::vector<uint8_t> live((size_t)n, 0);
    if (!so_model_ok(in)) {
        status = SO_REJECTED | SO_BAD_MODEL;
        so_identity(in);
    } else {
        double m[21];
        so_form(in, m);
        for (int i = 0; i < P.n; i++) {
            const double* p = P.pairs.data() + 12 * (size_t)i;
            bool a = so_pair_ok(p);
            if (a) {
                so_res r;
                so_residual(m, p, P.cam, r);
                a = so_front(r);
            }
            P.active[i] = live[i] = a ? 1 : 0;
        }
        for (int st = 0; st < 2; st++) {
            const double delta = st == 0 ? sqrt(th2) : 0.0;
            const int iters = st == 0 ? it0 : (nbad > 0 ? it_bad : it_clean);
            if (stage(P, model, delta, iters, &accepted)) status |= SO_STALLED;
            classify(P, model, th2, counts);
            if (st == 0) {
                nbad = counts[1];
                if (counts[0] < min_pairs) { status |= SO_REJECTED; break; }
            }
        }
    }
    const bool rejected = (status & SO_REJECTED) != 0;
    double m[21];
    so_form(model, m);
    for (int i = 0; i < P.n; i++) {
        double c1 = NAN, c2 = NAN;
        if (live[i] && !rejected) {
            so_res r;
            so_residual(m, P.pairs.data() + 12 * (size_t)i, P.cam, r);
            c1 = r.c1; c2 = r.c2;
        }
        chi2[2 * (size_t)i] = c1; chi2[2 * (size_t)i + 1] = c2;
        inlier[i] = (!rejected && P.active[i]) ? 1 : 0;
    }
    memcpy(model_out, rejected ? in : model, sizeof in);
    stats[0] = rejected ? 0 : counts[0]; stats[1] = accepted; stats[2] = nbad; stats[3] = status;
    if (work) { work[0] = P.trials; work[1] = P.evaluations; }
    return 0;
}

}  // extern "C"

#ifdef SIM3_OPT_TWIN_MAIN
// sim3_opt_twin_san <job file> <result file>.  Job: int64 n, has_sigma, it0, it_bad, it_clean, min_pairs, fix_scale; double fx fy
// cx cy th2; model [13]; X1 [n,3], X2 [n,3], px1 [n,2], px2 [n,2], sigma2 [n,2] if has_sigma -> model [13], stats int32 [4],
// chi2 [n,2], mask uint8 [n].  All native-endian.  Exit 0 on success; a sanitizer report ends the run non-zero.
static bool rd(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }
int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s job result\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    int64_t h[7];
    double p[5], model[13];
    bool ok = rd(in, h, sizeof h) && rd(in, p, sizeof p) && rd(in, model, sizeof model) && h[0] >= 0 && h[0] <= (1 << 24);
    const size_t n = ok ? (size_t)h[0] : 0;
    std::vector<double> X1(3 * n), X2(3 * n), px1(2 * n), px2(2 * n), sg(ok && h[1] ? 2 * n : 0), chi2(2 * n);
    ok = ok && rd(in, X1.data(), 8 * X1.size()) && rd(in, X2.data(), 8 * X2.size()) && rd(in, px1.data(), 8 * px1.size()) &&
         rd(in, px2.data(), 8 * px2.size()) && rd(in, sg.data(), 8 * sg.size());
    fclose(in);
    if (!ok) { fprintf(stderr, "bad job file\n"); return 2; }
    std::vector<uint8_t> mask(n);
    double out[13];
    int32_t st[4];
    if (s3o_optimize((int64_t)n, X1.data(), X2.data(), px1.data(), px2.data(), h[1] ? sg.data() : nullptr, model, p[0], p[1], p[2], p[3], p[4],
                     (int)h[2], (int)h[3], (int)h[4], (int)h[5], (int)h[6], out, mask.data(), chi2.data(), st, nullptr) != 0) return 2;
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    bool wrote = fwrite(out, 1, sizeof out, o) == sizeof out && fwrite(st, 1, sizeof st, o) == sizeof st;
    wrote = wrote && (n == 0 || (fwrite(chi2.data(), 8, 2 * n, o) == 2 * n && fwrite(mask.data(), 1, n, o) == n));
    return (fclose(o) == 0 && wrote) ? 0 : 2;
}
#endif
