// proj_match_twin.cpp - the per-point gates of the projection search (csrc/proj_point.h) as a stand-alone host
// program: the header the device kernel includes, built by a plain C++ compiler with -ffp-contract=off (and, in the test, with
// AddressSanitizer and UndefinedBehaviorSanitizer).  Usage: proj_match_twin JOB
// JOB (binary, native endianness): int64 n, flags (1 = ranges, 2 = normals, 4 = levels), n_levels; f64 fx fy cx cy, min_x max_x
// min_y max_y, cos2_limit, th, A[12], Ow[3], scale[16], scale2[16]; f64 xyz[3n]; f64 range[2n], normal[3n], int32 level[n] as
// flagged.  Prints one line per point: status, the bits of u and of v as hex, lp.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "proj_point.h"

template <typename T>
static bool take(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t head[3];
    double num[10 + 12 + 3 + 2 * PP_LEVELS_MAX];
    if (fread(head, sizeof(head), 1, f) != 1 || fread(num, sizeof(num), 1, f) != 1) return 3;
    const int64_t n = head[0], flags = head[1];
    if (n < 0 || n > (1 << 20) || head[2] < 1 || head[2] > PP_LEVELS_MAX) return 3;
    pp_camera c;
    memset(&c, 0, sizeof(c));
    c.fx = num[0], c.fy = num[1], c.cx = num[2], c.cy = num[3];
    c.min_x = num[4], c.max_x = num[5], c.min_y = num[6], c.max_y = num[7];
    c.cos2_limit = num[8];
    const double th = num[9];
    const double* A = num + 10;
    const double* Ow = num + 22;
    memcpy(c.scale, num + 25, sizeof(c.scale));
    memcpy(c.scale2, num + 25 + PP_LEVELS_MAX, sizeof(c.scale2));
    c.n_levels = (int)head[2];
    std::vector<double> xyz, range, normal;
    std::vector<int32_t> level;
    if (!take(f, xyz, 3 * (size_t)n) || !take(f, range, (flags & 1) ? 2 * (size_t)n : 0) || !take(f, normal, (flags & 2) ? 3 * (size_t)n : 0) ||
        !take(f, level, (flags & 4) ? (size_t)n : 0))
        return 3;
    fclose(f);
    for (int64_t i = 0; i < n; i++) {
        const pp_result o = pp_gates(c, A, Ow, th, &xyz[3 * i], (flags & 1) ? &range[2 * i] : nullptr, (flags & 2) ? &normal[3 * i] : nullptr,
                                     (flags & 4) ? &level[i] : nullptr);
        uint64_t ub, vb;
        memcpy(&ub, &o.u, 8);
        memcpy(&vb, &o.v, 8);
        printf("%d %016llx %016llx %d\n", o.status, (unsigned long long)ub, (unsigned long long)vb, o.lp);
    }
    return 0;
}
