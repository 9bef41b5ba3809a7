// tri_match_twin.cpp - the per-candidate gates and the per-match geometry of the epipolar search (csrc/tri_point.h, DESIGN.md
// 4m) as a stand-alone host program: the header the device kernels include, built by a plain C++ compiler with
// -ffp-contract=off (and, in the CPU suite, with AddressSanitizer and UndefinedBehaviorSanitizer).  Usage: tri_match_twin JOB
// JOB (binary, native endianness) starts with int64 mode, n_levels and f64 scale[16], sigma2[16].
//   mode 0 (gates): f64 chi2, epipole_r2, F[9], ex, ey; int64 n1, n2; f32 xy1[2 n1], xy2[2 n2]; int32 level2[n2].
//       Prints n1 lines of n2 digits: bit 0 = off the epipole, bit 1 = on the epipolar line.
//   mode 1 (geometry): f64 fx fy cx cy cos_max chi2_px ratio_factor, T1[12], T2[12], O1[3], O2[3]; int64 n; f32 xy1[2n],
//       xy2[2n]; int32 l1[n], l2[n].  Prints per match: status and the bits of X[3], normal[3], range[2] as hex.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#define __host__
#define __device__
#define __forceinline__ inline
#include "tri_point.h"

template <typename T>
static bool take(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t head[2];
    tp_params c;
    memset(&c, 0, sizeof(c));
    if (fread(head, sizeof(head), 1, f) != 1 || fread(c.scale, sizeof(c.scale), 1, f) != 1 || fread(c.sigma2, sizeof(c.sigma2), 1, f) != 1) return 3;
    if (head[1] < 1 || head[1] > TP_LEVELS_MAX) return 3;
    c.n_levels = (int)head[1];
    std::vector<float> xy1, xy2;
    std::vector<int32_t> la, lb;
    if (head[0] == 0) {
        double num[13];
        int64_t n[2];
        if (fread(num, sizeof(num), 1, f) != 1 || fread(n, sizeof(n), 1, f) != 1) return 3;
        if (n[0] < 0 || n[1] < 0 || n[0] > (1 << 16) || n[1] > (1 << 16)) return 3;
        if (!take(f, xy1, 2 * (size_t)n[0]) || !take(f, xy2, 2 * (size_t)n[1]) || !take(f, lb, (size_t)n[1])) return 3;
        for (int l = 0; l < c.n_levels; l++) {          // as the library's host side makes them
            c.line_lim[l] = num[0] * c.sigma2[l];
            c.epi_lim[l] = num[1] * c.scale[l];
        }
        std::vector<char> line((size_t)n[1] + 1);
        for (int64_t i = 0; i < n[0]; i++) {
            const tp_line ln = tp_epiline(num + 2, (double)xy1[2 * i], (double)xy1[2 * i + 1]);
            for (int64_t j = 0; j < n[1]; j++) {
                const int l = tp_level(lb[j], c.n_levels);
                const double x2 = (double)xy2[2 * j], y2 = (double)xy2[2 * j + 1];
                line[j] = (char)('0' + (tp_off_epipole(num[11], num[12], x2, y2, c.epi_lim[l]) ? 1 : 0) + (tp_on_line(ln, x2, y2, c.line_lim[l]) ? 2 : 0));
            }
            line[n[1]] = 0;
            puts(line.data());
        }
    } else if (head[0] == 1) {
        double num[7 + 30];
        int64_t n;
        if (fread(num, sizeof(num), 1, f) != 1 || fread(&n, sizeof(n), 1, f) != 1) return 3;
        if (n < 0 || n > (1 << 20)) return 3;
        if (!take(f, xy1, 2 * (size_t)n) || !take(f, xy2, 2 * (size_t)n) || !take(f, la, (size_t)n) || !take(f, lb, (size_t)n)) return 3;
        c.fx = num[0], c.fy = num[1], c.cx = num[2], c.cy = num[3];
        c.cos_max = num[4], c.chi2_px = num[5], c.ratio_factor = num[6];
        for (int64_t i = 0; i < n; i++) {
            const tp_point o = tp_triangulate(c, num + 7, num + 19, num + 31, num + 34, (double)xy1[2 * i], (double)xy1[2 * i + 1],
                                              (double)xy2[2 * i], (double)xy2[2 * i + 1], la[i], lb[i]);
            const double out[8] = {o.X[0], o.X[1], o.X[2], o.normal[0], o.normal[1], o.normal[2], o.range[0], o.range[1]};
            printf("%d", o.status);
            for (int k = 0; k < 8; k++) {
                uint64_t bits;
                memcpy(&bits, &out[k], 8);
                printf(" %016llx", (unsigned long long)bits);
            }
            printf("\n");
        }
    } else {
        return 3;
    }
    fclose(f);
    return 0;
}
