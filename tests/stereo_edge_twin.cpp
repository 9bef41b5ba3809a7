// The host twin of the stereo / weighted edge model: csrc/stereo_edge.h - the text the kernels of ba_stereo.hip and
// pose_stereo.hip run - compiled with a plain C++ compiler (-ffp-contract=off) behind the surface of
// slam_reproj_rj_stereo_f64 plus the robust cost and the classification.  Built as a shared library for ctypes, and with
// -DSTEREO_EDGE_TWIN_MAIN as a stand-alone program (job file in, result file out) that runs under
// -fsanitize=address,undefined.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "../slam-experiments_amd/csrc/stereo_edge.h"

static double tw_nan() {
    const uint64_t b = 0x7ff8000000000000ull;
    double d;
    memcpy(&d, &b, 8);
    return d;
}

// every edge of an observation table: e [O,3], Jpose [O,18], Jpoint [O,9], chi2, w, rho [O], inlier u8 [O]; an index outside
// its range is never dereferenced (NaN outputs, no inlier, one count), an information that is none counts once.
// par [9] = fx, fy, cx, cy, bf, delta_mono, delta_stereo, chi2_mono, chi2_stereo.  Returns the count.
extern "C" int64_t se_tw_edges(int64_t K, int64_t L, int64_t O, const double* poses, const double* points, const int32_t* op, const int32_t* ol,
                               const double* meas3, const double* info, const double* par, double* e, double* jp, double* jq, double* chi2,
                               double* w, double* rho, uint8_t* inlier) {
    const se_cam cam = {par[0], par[1], par[2], par[3], par[4]};
    const se_huber hub = {par[5], par[6]};
    const se_gate gate = {par[7], par[8]};
    int64_t count = 0;
    for (int64_t o = 0; o < O; o++) {
        const int64_t k = op[o], l = ol[o];
        if (k < 0 || k >= K || l < 0 || l >= L) {
            count++;
            for (int i = 0; i < 3; i++) e[o * 3 + i] = tw_nan();
            for (int i = 0; i < 18; i++) jp[o * 18 + i] = tw_nan();
            for (int i = 0; i < 9; i++) jq[o * 9 + i] = tw_nan();
            chi2[o] = w[o] = rho[o] = tw_nan();
            inlier[o] = 0;
            continue;
        }
        if (!se_info_ok(info[o])) count++;
        se_res r;
        se_residual(poses + k * 12, points + l * 3, meas3[o * 3], meas3[o * 3 + 1], meas3[o * 3 + 2], info[o], cam, hub, r);
        se_jac j;
        se_jacobians(poses + k * 12, r, cam, j);
        for (int i = 0; i < 3; i++) e[o * 3 + i] = r.e[i];
        for (int i = 0; i < 3; i++)
            for (int a = 0; a < 6; a++) jp[o * 18 + i * 6 + a] = j.jp[i][a];
        for (int i = 0; i < 3; i++)
            for (int c = 0; c < 3; c++) jq[o * 9 + i * 3 + c] = j.jq[i][c];
        chi2[o] = r.chi2;
        w[o] = r.w;
        rho[o] = r.rho;
        // the gate is on the weighted chi2 itself, which the kernel does not change
        inlier[o] = se_inlier(r, gate) ? 1 : 0;
    }
    return count;
}

#ifdef STEREO_EDGE_TWIN_MAIN
// job: int64 K, L, O; double par[9]; poses [K,12], points [L,3], op int32 [O], ol int32 [O], meas3 [O,3], info [O]
// result: e, jp, jq, chi2, w, rho (f64), inlier (u8), count (int64)
template <typename T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}
template <typename T>
static bool wr(FILE* f, const std::vector<T>& v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    int64_t h[3];
    double par[9];
    if (fread(h, 8, 3, f) != 3 || fread(par, 8, 9, f) != 9 || h[0] < 0 || h[1] < 0 || h[2] < 0) return 4;
    const size_t K = (size_t)h[0], L = (size_t)h[1], O = (size_t)h[2];
    std::vector<double> poses, points, meas3, info;
    std::vector<int32_t> op, ol;
    if (!rd(f, poses, K * 12) || !rd(f, points, L * 3) || !rd(f, op, O) || !rd(f, ol, O) || !rd(f, meas3, O * 3) || !rd(f, info, O)) return 5;
    fclose(f);
    std::vector<double> e(O * 3), jp(O * 18), jq(O * 9), chi2(O), w(O), rho(O);
    std::vector<uint8_t> inl(O);
    const int64_t count = se_tw_edges(h[0], h[1], h[2], poses.data(), points.data(), op.data(), ol.data(), meas3.data(), info.data(), par, e.data(),
                                      jp.data(), jq.data(), chi2.data(), w.data(), rho.data(), inl.data());
    FILE* g = fopen(argv[2], "wb");
    if (!g) return 6;
    if (!wr(g, e) || !wr(g, jp) || !wr(g, jq) || !wr(g, chi2) || !wr(g, w) || !wr(g, rho) || !wr(g, inl) || fwrite(&count, 8, 1, g) != 1) return 7;
    fclose(g);
    return 0;
}
#endif
