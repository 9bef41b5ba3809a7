// sim3_graph_twin.cpp — the host twin of csrc/sim3_graph.hip (test infrastructure).
//
// Includes the kernel file itself with S3G_HOST_ONLY defined: the per-edge routines below (chart, J_j, Ad, the J^T Omega J
// blocks, retraction, 7x7 inverse) ARE the device routines' source, compiled for the host by g++ with contraction off and no
// FMA instructions available (x86-64 baseline).  sin, cos, atan2, log and exp come from different libraries on host and
// device, so this twin is compared with the device BY TOLERANCE, NOT BIT FOR BIT (unlike sim3_twin.cpp, whose routines use
// + - * / sqrt only).
//
// Built twice by tests/sim3_graph_twin.py: a shared library (loaded through ctypes) and, with S3G_TWIN_MAIN and
// -fsanitize=address,undefined, a stand-alone program that reads a job file and writes a result file.
#include <cmath>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
using std::isfinite;

#define S3G_HOST_ONLY
#include "../slam-experiments_amd/csrc/sim3_graph.hip"

extern "C" {

// n edges: Si, Sj, Z [n,13], Om [n,49] -> rho [n], why int32 [n]; full != 0 also W [n,49], Di, Dj [n,35]
int s3gt_edges(int64_t n, const double* Si, const double* Sj, const double* Z, const double* Om, double huber, int fix_scale, int full,
               double* rho, int32_t* why, double* W, double* Di, double* Dj) {
    for (int64_t e = 0; e < n; e++) {
        if (full) {
            double Wt[49];
            why[e] = s3g_edge<true>(Si + 13 * e, Sj + 13 * e, Z + 13 * e, Om + 49 * e, huber, fix_scale != 0, rho + e, W + 49 * e, Wt, nullptr,
                                    Di + 35 * e, Dj + 35 * e);
            for (int a = 0; a < 7; a++)
                for (int b = 0; b < 7; b++)
                    if (Wt[b * 7 + a] != W[49 * e + a * 7 + b] && !(Wt[b * 7 + a] != Wt[b * 7 + a])) return -1;      // the transposed copy
        } else {
            why[e] = s3g_edge<false>(Si + 13 * e, Sj + 13 * e, Z + 13 * e, Om + 49 * e, huber, fix_scale != 0, rho + e, nullptr, nullptr, nullptr,
                                     nullptr, nullptr);
        }
    }
    return 0;
}

// out [n,13] = Phi(dx [n,7]) o S [n,13]
int s3gt_update(int64_t n, const double* dx, const double* S, double* out) {
    for (int64_t k = 0; k < n; k++) s3g_apply_update(dx + 7 * k, S + 13 * k, out + 13 * k);
    return 0;
}

// Inv [n,49] = A [n,49]^-1 by LDL^T, ok [n] = SPD
int s3gt_inverse7(int64_t n, const double* A, double* Inv, int32_t* ok) {
    for (int64_t k = 0; k < n; k++) ok[k] = s3g_inverse7(A + 49 * k, Inv + 49 * k) ? 1 : 0;
    return 0;
}
}  // extern "C"

#ifdef S3G_TWIN_MAIN
// job file: int64 op, n, fix_scale, full; double huber; then the operands.  op 0: edges, 1: update, 2: inverse7.
static std::vector<double> take(FILE* f, size_t n) {
    std::vector<double> v(n ? n : 1);
    if (n && fread(v.data(), 8, n, f) != n) { fprintf(stderr, "short job file\n"); exit(2); }
    return v;
}
int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s job result\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t h[4];
    double huber;
    if (fread(h, 8, 4, f) != 4 || fread(&huber, 8, 1, f) != 1) return 2;
    const int64_t op = h[0], n = h[1];
    if (n < 0 || n > (1 << 20)) return 2;
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    const size_t N = (size_t)n;
    if (op == 0) {
        auto Si = take(f, 13 * N), Sj = take(f, 13 * N), Z = take(f, 13 * N), Om = take(f, 49 * N);
        std::vector<double> rho(N + 1), W(49 * N + 1), Di(35 * N + 1), Dj(35 * N + 1);
        std::vector<int32_t> why(N + 1);
        if (s3gt_edges(n, Si.data(), Sj.data(), Z.data(), Om.data(), huber, (int)h[2], (int)h[3], rho.data(), why.data(), W.data(), Di.data(), Dj.data()))
            return 3;
        fwrite(rho.data(), 8, N, o); fwrite(why.data(), 4, N, o);
        if (h[3]) { fwrite(W.data(), 8, 49 * N, o); fwrite(Di.data(), 8, 35 * N, o); fwrite(Dj.data(), 8, 35 * N, o); }
    } else if (op == 1) {
        auto dx = take(f, 7 * N), S = take(f, 13 * N);
        std::vector<double> out(13 * N + 1);
        s3gt_update(n, dx.data(), S.data(), out.data());
        fwrite(out.data(), 8, 13 * N, o);
    } else if (op == 2) {
        auto A = take(f, 49 * N);
        std::vector<double> Inv(49 * N + 1);
        std::vector<int32_t> ok(N + 1);
        s3gt_inverse7(n, A.data(), Inv.data(), ok.data());
        fwrite(Inv.data(), 8, 49 * N, o); fwrite(ok.data(), 4, N, o);
    } else {
        return 2;
    }
    fclose(o);
    fclose(f);
    return 0;
}
#endif
