// fuse_twin.cpp - the per-point and per-candidate arithmetic of the fusion search and of the map-point refresh (csrc/fuse_point.h,
// DESIGN.md 4n) as a stand-alone host program: the header the device kernels include, built by a plain C++ compiler with
// -ffp-contract=off (and, in the CPU suite, with AddressSanitizer and UndefinedBehaviorSanitizer).  Usage: fuse_twin JOB
// JOB (binary, native endianness) starts with int64 mode.
//   mode 0 (gates): int64 n, flags (1 range, 2 normal, 4 level), n_levels; f64 camera[4], bounds[4], cos2_limit, th, m_lo2, m_hi2,
//       A[12], Ow[3], scale[16], scale2[16]; f64 xyz[3n]; then as flagged f64 range[2n], f64 normal[3n], int32 level[n].
//       Prints per point: status, the bits of u and v as hex, lp.
//   mode 1 (candidates): int64 n; f64 u, v; f32 xy[2n]; f64 lim[n].  Prints n digits: 1 = a candidate.
//   mode 2 (medians): int64 n; int32 D[n n].  Prints per row its median, then the chosen row.
//   mode 3 (normal and range): int64 n, ref, level, n_levels; f64 X[3], scale[16], O[3n].  Prints the bits of normal[3], range[2].
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#define __host__
#define __device__
#define __forceinline__ inline
#include "fuse_point.h"

template <typename T>
static bool take(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

static void hex(double x, const char* end) {
    uint64_t bits;
    memcpy(&bits, &x, 8);
    printf("%016llx%s", (unsigned long long)bits, end);
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t mode;
    if (fread(&mode, 8, 1, f) != 1) return 3;
    if (mode == 0) {
        int64_t head[3];
        double num[12 + 15 + 32];
        if (fread(head, sizeof(head), 1, f) != 1 || fread(num, sizeof(num), 1, f) != 1) return 3;
        const int64_t n = head[0], flags = head[1];
        if (n < 0 || n > (1 << 20) || head[2] < 1 || head[2] > FP_LEVELS_MAX) return 3;
        pp_camera c;
        memset(&c, 0, sizeof(c));
        c.fx = num[0], c.fy = num[1], c.cx = num[2], c.cy = num[3];
        c.min_x = num[4], c.max_x = num[5], c.min_y = num[6], c.max_y = num[7];
        c.cos2_limit = num[8];
        c.n_levels = (int)head[2];
        memcpy(c.scale, num + 27, sizeof(c.scale));
        memcpy(c.scale2, num + 43, sizeof(c.scale2));
        std::vector<double> xyz, rng, nrm;
        std::vector<int32_t> lvl;
        if (!take(f, xyz, 3 * (size_t)n) || !take(f, rng, flags & 1 ? 2 * (size_t)n : 0) || !take(f, nrm, flags & 2 ? 3 * (size_t)n : 0) ||
            !take(f, lvl, flags & 4 ? (size_t)n : 0))
            return 3;
        for (int64_t i = 0; i < n; i++) {
            const pp_result o = fp_gates(c, num + 12, num + 24, num[9], &xyz[3 * i], flags & 1 ? &rng[2 * i] : nullptr,
                                         flags & 2 ? &nrm[3 * i] : nullptr, flags & 4 ? &lvl[i] : nullptr, num[10], num[11]);
            printf("%d ", o.status);
            hex(o.u, " ");
            hex(o.v, " ");
            printf("%d\n", o.lp);
        }
    } else if (mode == 1) {
        int64_t n;
        double uv[2];
        if (fread(&n, 8, 1, f) != 1 || fread(uv, sizeof(uv), 1, f) != 1 || n < 0 || n > (1 << 20)) return 3;
        std::vector<float> xy;
        std::vector<double> lim;
        if (!take(f, xy, 2 * (size_t)n) || !take(f, lim, (size_t)n)) return 3;
        std::vector<char> line((size_t)n + 1, 0);
        for (int64_t j = 0; j < n; j++) line[j] = fp_candidate(uv[0], uv[1], xy[2 * j], xy[2 * j + 1], lim[j]) ? '1' : '0';
        puts(line.data());
    } else if (mode == 2) {
        int64_t n;
        if (fread(&n, 8, 1, f) != 1 || n < 0 || n > FP_OBS_MAX) return 3;
        std::vector<int32_t> D;
        if (!take(f, D, (size_t)(n * n))) return 3;
        uint32_t best = 0xFFFFFFFFu;
        for (int64_t i = 0; i < n; i++) {
            const int32_t* row = &D[(size_t)(i * n)];
            const int med = fp_median((int)n, [&](int k) { return (int)row[k]; });
            printf("%d\n", med);
            const uint32_t key = fp_choice_key(med, (int)i);
            if (key < best) best = key;
        }
        printf("%d\n", n > 0 ? (int)(best & 255u) : -1);
    } else if (mode == 3) {
        int64_t head[4];
        double X[3], scale[16];
        if (fread(head, sizeof(head), 1, f) != 1 || fread(X, sizeof(X), 1, f) != 1 || fread(scale, sizeof(scale), 1, f) != 1) return 3;
        const int64_t n = head[0];
        if (n < 1 || n > FP_OBS_MAX || head[1] < 0 || head[1] >= n || head[3] < 1 || head[3] > FP_LEVELS_MAX) return 3;
        std::vector<double> O;
        if (!take(f, O, 3 * (size_t)n)) return 3;
        double s[3] = {0, 0, 0}, dist = 0, t[4];
        for (int64_t k = 0; k < n; k++) {
            fp_view(X, &O[3 * (size_t)k], t);
            if (k == 0) s[0] = t[0], s[1] = t[1], s[2] = t[2];
            else s[0] += t[0], s[1] += t[1], s[2] += t[2];
            if (k == head[1]) dist = t[3];
        }
        double nr[3], rg[2];
        fp_normal_range(s, dist, (int)head[2], scale, (int)head[3], nr, rg);
        hex(nr[0], " ");
        hex(nr[1], " ");
        hex(nr[2], " ");
        hex(rg[0], " ");
        hex(rg[1], "\n");
    } else {
        return 3;
    }
    fclose(f);
    return 0;
}
