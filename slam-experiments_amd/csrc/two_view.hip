// two_view.hip — batched two-view geometry on gfx950: what the reference gets from cv2.findEssentialMat,
// cv2.recoverPose and cv2.triangulatePoints (utils.py:10-28, utils.py:32-55), for MANY frame pairs in one call.
//
//   slam_tv_fivepoint_f64          the minimal solver on its own: all real essential matrices through five correspondences
//   slam_tv_essential_ransac_f64   H hypotheses per pair, every root scored on all matches of the pair (Sampson distance)
//   slam_tv_recover_pose_f64       SVD of E, the four (R, t) candidates, cheirality vote
//   slam_tv_triangulate_f64        the 4x4 DLT per point
//
// All arithmetic is f64 and the file is compiled with floating-point contraction OFF (the pragma below): no multiply-add is
// fused unless the source says fma(), so every function here is a pure function of its inputs whatever it is inlined into.
// The RANSAC depends on it twice: the winning hypothesis is solved again by the kernel that writes the result (instead of
// keeping ten matrices per hypothesis in memory) and must come out bit for bit as it was scored, and the scoring is stated in
// the header operation by operation so that a caller can recompute a mask exactly.
//
// The solver (Nister's five-point algorithm with the constraints built by polynomial arithmetic, not hand-expanded):
//   1. null space of the 5x9 epipolar system: Householder QR of its transpose, basis = Q e5..e8 mixed by a fixed orthogonal
//      matrix (orthonormal, in general position to the sample's structure), E = xX + yY + zZ + W;
//   2. det E = 0 and 2 E E^T E - tr(E E^T) E = 0 as ten cubics in (x, y, z): products of 4- and 10-coefficient polynomials
//      through constexpr index tables, one 20-coefficient row at a time in registers, rows stored to LDS;
//   3. Gauss-Jordan with row pivoting on the 10x20 system in LDS (columns: the ten monomials that contain x or y to a power
//      above one or together, then xz^2 xz x yz^2 yz y z^3 z^2 z 1); a pivot below TV_PIVOT_MIN: steps 1-3 again in a second basis;
//   4. rows (x^2 z) - z (x^2), (y^2 z) - z (y^2), (xyz) - z (xy) give B(z) [x y 1]^T = 0 with B 3x3 of degree 3, 3, 4:
//      det B(z) is the degree-10 polynomial;
//   5. its real roots: the roots of each derivative bracket the roots of the one below it (degree 1 up to 10), every bracket
//      closed by a safeguarded Newton iteration - bounded loops, no recursion, ascending order for free;
//   6. per root, (x, y) from the best-conditioned pair of rows of B(z), then a few Gauss-Newton steps on the ten constraints
//      themselves in (x, y, z) (the expanded degree-10 coefficients lose digits the constraints still have), E normalised.
// One hypothesis per lane.  A 10x20 f64 system is 400 VGPRs: it lives in LDS instead, lane-interleaved (entry i of lane l at
// double i * 64 + l: conflict-free whatever row a lane's pivot search is in), 236 doubles per lane = 118 KiB per 64-lane block
// (one block per CU).  Everything indexed at run time (pivot rows, derivative coefficients, root lists) is in LDS; register
// arrays are only indexed by unrolled constants, so nothing goes to scratch.
#ifndef TV_HOST_ONLY                 // a host build of the routines alone (the test suite's twin) defines it
#include "internal.h"
#endif
#include <math.h>
#include "geometry_common.h"         // sampler, Jacobi, triangulation, cheirality, range clamp, intrinsics, model key

#pragma clang fp contract(off)

#define TV_LANES 64
#define TV_LDS_PER_LANE 236          // doubles: 10x20 system (reused by the root finder and the result) + 4x9 null space
#define TV_HD __host__ __device__ __forceinline__
// the shared routines under this file's names, as its host twin calls them (the sample size is this file's: five matches)
#define tv_draw_sample geo_draw_sample<5>
#define tv_triangulate_point geo_triangulate_point
#define TVL(i) lds[(i) * TV_LANES]
// LDS layout per lane after the elimination (the system is dead by then)
#define TV_DER 0                     // 66: coefficients of p and its ten derivatives (11 + 10 + ... + 1)
#define TV_ROOTS_A 130               // 10 + 10: root lists of two consecutive derivatives
#define TV_ROOTS_B 140
#define TV_BPOLY 150                 // 39: B(z), per row x-part (4), y-part (4), constant part (5)
#define TV_BASIS 200                 // 36: X, Y, Z, W
#define TV_EOUT 0                    // 90: up to ten matrices (written after the roots are final)

// ---- polynomial index tables ---------------------------------------------------------------------------------------------
struct tv_exp { int x, y, z; };
struct tv_tables { int m2[4][4]; int m3[10][4]; };
constexpr tv_exp TV_MONO1[4] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {0, 0, 0}};
constexpr tv_exp TV_MONO2[10] = {{2, 0, 0}, {0, 2, 0}, {0, 0, 2}, {1, 1, 0}, {1, 0, 1}, {0, 1, 1}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {0, 0, 0}};
constexpr tv_exp TV_MONO3[20] = {{3, 0, 0}, {0, 3, 0}, {2, 1, 0}, {1, 2, 0}, {2, 0, 1}, {2, 0, 0}, {0, 2, 1}, {0, 2, 0}, {1, 1, 1}, {1, 1, 0},
                                 {1, 0, 2}, {1, 0, 1}, {1, 0, 0}, {0, 1, 2}, {0, 1, 1}, {0, 1, 0}, {0, 0, 3}, {0, 0, 2}, {0, 0, 1}, {0, 0, 0}};
constexpr tv_tables tv_make_tables() {
    tv_tables t = {};
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++)
            for (int k = 0; k < 10; k++)
                if (TV_MONO2[k].x == TV_MONO1[i].x + TV_MONO1[j].x && TV_MONO2[k].y == TV_MONO1[i].y + TV_MONO1[j].y &&
                    TV_MONO2[k].z == TV_MONO1[i].z + TV_MONO1[j].z) t.m2[i][j] = k;
    for (int i = 0; i < 10; i++)
        for (int j = 0; j < 4; j++)
            for (int k = 0; k < 20; k++)
                if (TV_MONO3[k].x == TV_MONO2[i].x + TV_MONO1[j].x && TV_MONO3[k].y == TV_MONO2[i].y + TV_MONO1[j].y &&
                    TV_MONO3[k].z == TV_MONO2[i].z + TV_MONO1[j].z) t.m3[i][j] = k;
    return t;
}
constexpr tv_tables TV_T = tv_make_tables();

// r (10) += s * a (4) * b (4)
TV_HD void tv_mul11(double* r, const double* a, const double* b, double s) {
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) r[TV_T.m2[i][j]] += s * (a[i] * b[j]);
}
// r (20) += a (10) * b (4)
TV_HD void tv_mul21(double* r, const double* a, const double* b) {
#pragma unroll
    for (int i = 0; i < 10; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) r[TV_T.m3[i][j]] += a[i] * b[j];
}
// entry (a, b) of E as a polynomial (coefficients of x, y, z, 1) from the null-space basis in LDS
TV_HD void tv_entry(const double* lds, int ab, double* e) {
#pragma unroll
    for (int c = 0; c < 4; c++) e[c] = TVL(TV_BASIS + 9 * c + ab);
}

// ---- 1. null space ---------------------------------------------------------------------------------------------------------
TV_HD void tv_null_space(double* lds, const double* x1, const double* x2, bool second) {
    double A[9][5];
#pragma unroll
    for (int c = 0; c < 5; c++) {
        const double h1[3] = {x1[2 * c], x1[2 * c + 1], 1.0}, h2[3] = {x2[2 * c], x2[2 * c + 1], 1.0};
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) A[3 * i + j][c] = h2[i] * h1[j];
    }
    double beta[5];
#pragma unroll
    for (int k = 0; k < 5; k++) {
        double s = 0.0;
#pragma unroll
        for (int r = k; r < 9; r++) s += A[r][k] * A[r][k];
        const double nrm = sqrt(s), akk = A[k][k];
        const double vk = akk > 0.0 ? akk + nrm : akk - nrm;
        const double v2 = s - akk * akk + vk * vk;
        A[k][k] = vk;
        beta[k] = v2 > 0.0 ? 2.0 / v2 : 0.0;
#pragma unroll
        for (int c = k + 1; c < 5; c++) {
            double d = 0.0;
#pragma unroll
            for (int r = k; r < 9; r++) d += A[r][k] * A[r][c];
            d *= beta[k];
#pragma unroll
            for (int r = k; r < 9; r++) A[r][c] -= d * A[r][k];
        }
    }
    // The basis is Q e5..e8 mixed by a fixed orthogonal 4x4 matrix in general position (det -1: a reflection, which is all the same to a basis).  Q e5..e8 itself inherits the
    // structure of the sample: for R = I and t along x the true matrix has NO component along Q e8, and the solver, which
    // fixes that component to 1, sees it as a root at infinity (the degree-10 polynomial loses its leading coefficient).
    // A fixed orthogonal mix keeps the span and the orthonormality and makes such an alignment a coincidence, not a geometry.
    // The second basis (the transposed matrix) is for the sample whose elimination met a vanishing pivot under the first.
    // A sample that is ill-conditioned in every basis is not helped by it: five points of which four or more lie beyond 100
    // baselines are a pure rotation to seven digits, the ten leading monomials are nearly dependent whatever the basis, and
    // roots are lost (3 % of such samples where the action-matrix route of the tests' numpy solver still finds the truth).
    const double MIX[4][4] = {{-0.8601663278085514, -0.2042084343276712, -0.09535298528857732, -0.4575156959606404},
                              {-0.04551667097915731, -0.4630968403770512, 0.8783752666759934, 0.10920824139068044},
                              {0.21812373239709487, -0.8622554346005882, -0.4518672426796806, 0.0689463404393164},
                              {-0.4587637284403457, 0.018862589535480343, -0.12320995934378486, 0.8797723285612201}};
#pragma unroll
    for (int j = 0; j < 4; j++) {
        double q[9];
#pragma unroll
        for (int r = 0; r < 9; r++) q[r] = (r >= 5) ? (second ? MIX[r - 5][j] : MIX[j][r - 5]) : 0.0;
#pragma unroll
        for (int k = 4; k >= 0; k--) {
            double d = 0.0;
#pragma unroll
            for (int r = k; r < 9; r++) d += A[r][k] * q[r];
            d *= beta[k];
#pragma unroll
            for (int r = k; r < 9; r++) q[r] -= d * A[r][k];
        }
#pragma unroll
        for (int r = 0; r < 9; r++) TVL(TV_BASIS + 9 * j + r) = q[r];
    }
}

// ---- 2. the ten cubic constraints ---------------------------------------------------------------------------------------------
TV_HD void tv_constraints(double* lds) {
    {   // det E, by the first row's cofactors
        double row[20];
#pragma unroll
        for (int i = 0; i < 20; i++) row[i] = 0.0;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;
            double a[4], b[4], m[10];
#pragma unroll
            for (int i = 0; i < 10; i++) m[i] = 0.0;
            tv_entry(lds, 3 + c1, a); tv_entry(lds, 6 + c2, b); tv_mul11(m, a, b, 1.0);
            tv_entry(lds, 3 + c2, a); tv_entry(lds, 6 + c1, b); tv_mul11(m, a, b, -1.0);
            tv_entry(lds, c, a);
            tv_mul21(row, m, a);
        }
#pragma unroll
        for (int i = 0; i < 20; i++) TVL(i) = row[i];
    }
    // L = E E^T - tr(E E^T) / 2 (symmetric: 6 polynomials of degree 2), then the nine entries of L E
    double L[6][10];
    const int li[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = i; j < 3; j++) {
            double* m = L[li[i][j]];
#pragma unroll
            for (int t = 0; t < 10; t++) m[t] = 0.0;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                double a[4], b[4];
                tv_entry(lds, 3 * i + k, a); tv_entry(lds, 3 * j + k, b);
                tv_mul11(m, a, b, 1.0);
            }
        }
#pragma unroll
    for (int t = 0; t < 10; t++) {
        const double h = 0.5 * ((L[0][t] + L[3][t]) + L[5][t]);
        L[0][t] -= h; L[3][t] -= h; L[5][t] -= h;
    }
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double row[20];
#pragma unroll
            for (int t = 0; t < 20; t++) row[t] = 0.0;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                double e[4];
                tv_entry(lds, 3 * k + j, e);
                tv_mul21(row, L[li[i][k]], e);
            }
#pragma unroll
            for (int t = 0; t < 20; t++) TVL(20 * (1 + 3 * i + j) + t) = row[t];
        }
}

// ---- 3. Gauss-Jordan with row pivoting on the left 10x10 block -----------------------------------------------------------------
// A sample whose smallest pivot is below this is eliminated again in the second basis.  The rows are O(1) (the basis is
// orthonormal) and the smallest pivot of a sample has a continuous tail: median 1e-2 .. 8e-2 over the scene families of the
// tests, below 1e-3 on 2 - 7 % of the samples of a family (their roots are still good to 1e-11), below 1e-4 on a few in a
// thousand; the fronto-parallel sample that lost its true root had 5e-7.  The roots lose about eps / pivot, the polish
// recovers a root that is off by 1e-8 but not one off by 1e-2: 1e-4 keeps the retry rare and two decades of margin.  It costs
// a retrying lane's wave steps 1-3 a second time (measured: the 64-pair batch of the tests went from 1.94 to 1.97 ms).
#define TV_PIVOT_MIN 1e-4
// returns the smallest pivot it divided by
TV_HD double tv_eliminate(double* lds) {
    double low = 1.0;
    for (int c = 0; c < 10; c++) {
        int best = c;
        double bv = fabs(TVL(20 * c + c));
        for (int r = c + 1; r < 10; r++) {
            const double v = fabs(TVL(20 * r + c));
            if (v > bv) { bv = v; best = r; }
        }
        if (best != c)
            for (int j = c; j < 20; j++) {
                const double t = TVL(20 * c + j);
                TVL(20 * c + j) = TVL(20 * best + j);
                TVL(20 * best + j) = t;
            }
        low = bv < low ? bv : low;
        const double inv = 1.0 / TVL(20 * c + c);
        for (int j = c + 1; j < 20; j++) TVL(20 * c + j) *= inv;
        for (int r = 0; r < 10; r++) {
            if (r == c) continue;
            const double f = TVL(20 * r + c);
            for (int j = c + 1; j < 20; j++) TVL(20 * r + j) -= f * TVL(20 * c + j);
        }
    }
    return low;
}

// ---- 4. B(z) and its determinant ---------------------------------------------------------------------------------------------
template <int NA, int NB>
TV_HD void tv_pmul(double* r, const double* a, const double* b, double s) {   // r += s a b, ascending coefficients
#pragma unroll
    for (int i = 0; i < NA; i++)
#pragma unroll
        for (int j = 0; j < NB; j++) r[i + j] += s * (a[i] * b[j]);
}
TV_HD void tv_bpoly(double* lds) {
    double Bx[3][4], By[3][4], Bc[3][5];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int ra = 20 * (4 + 2 * i), rb = ra + 20;   // rows (.. z) and (..) of the pair: k = a - z b
        Bx[i][0] = TVL(ra + 12);
        Bx[i][1] = TVL(ra + 11) - TVL(rb + 12);
        Bx[i][2] = TVL(ra + 10) - TVL(rb + 11);
        Bx[i][3] = -TVL(rb + 10);
        By[i][0] = TVL(ra + 15);
        By[i][1] = TVL(ra + 14) - TVL(rb + 15);
        By[i][2] = TVL(ra + 13) - TVL(rb + 14);
        By[i][3] = -TVL(rb + 13);
        Bc[i][0] = TVL(ra + 19);
        Bc[i][1] = TVL(ra + 18) - TVL(rb + 19);
        Bc[i][2] = TVL(ra + 17) - TVL(rb + 18);
        Bc[i][3] = TVL(ra + 16) - TVL(rb + 17);
        Bc[i][4] = -TVL(rb + 16);
    }
    double p[11];
#pragma unroll
    for (int i = 0; i < 11; i++) p[i] = 0.0;
#pragma unroll
    for (int c = 0; c < 3; c++) {       // cofactors along the constant column
        const int r1 = (c + 1) % 3, r2 = (c + 2) % 3;
        double m[7];
#pragma unroll
        for (int i = 0; i < 7; i++) m[i] = 0.0;
        tv_pmul<4, 4>(m, Bx[r1], By[r2], 1.0);
        tv_pmul<4, 4>(m, Bx[r2], By[r1], -1.0);
        tv_pmul<7, 5>(p, m, Bc[c], 1.0);
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int k = 0; k < 4; k++) { TVL(TV_BPOLY + 13 * i + k) = Bx[i][k]; TVL(TV_BPOLY + 13 * i + 4 + k) = By[i][k]; }
#pragma unroll
        for (int k = 0; k < 5; k++) TVL(TV_BPOLY + 13 * i + 8 + k) = Bc[i][k];
    }
#pragma unroll
    for (int i = 0; i < 11; i++) TVL(TV_DER + i) = p[i];
}

// ---- 5. real roots of the degree-10 polynomial ---------------------------------------------------------------------------------
// derivative d (0..9) has 11 - d coefficients at TV_DER + tv_der_off(d), ascending
TV_HD int tv_der_off(int d) { return d * 11 - d * (d - 1) / 2; }
TV_HD double tv_horner(const double* lds, int off, int n, double x) {      // n coefficients
    double r = TVL(off + n - 1);
    for (int i = n - 2; i >= 0; i--) r = r * x + TVL(off + i);
    return r;
}
TV_HD bool tv_neg(double v) { return v < 0.0; }
// the root of derivative d in (lo, hi), where the polynomial is negative at lo iff neg_lo and changes sign: Newton steps kept
// inside the bracket, bisection when one leaves it or gains too little
TV_HD double tv_close(const double* lds, int d, double lo, double hi, bool neg_lo) {
    const int off = tv_der_off(d), n = 11 - d, off1 = tv_der_off(d + 1);
    double x = 0.5 * (lo + hi), dxold = fabs(hi - lo), dx = dxold;
    double f = tv_horner(lds, off, n, x), df = tv_horner(lds, off1, n - 1, x);
    for (int it = 0; it < 200; it++) {
        const double lo_side = neg_lo ? lo : hi, hi_side = neg_lo ? hi : lo;      // f < 0 at lo_side, f >= 0 at hi_side
        const bool out = ((x - hi_side) * df - f) * ((x - lo_side) * df - f) > 0.0;
        double xn;
        if (out || !(fabs(2.0 * f) <= fabs(dxold * df))) {
            dxold = dx;
            dx = 0.5 * (hi - lo);
            xn = lo + dx;
            if (xn == lo || xn == hi) return x;
        } else {
            dxold = dx;
            dx = f / df;
            xn = x - dx;
            if (xn == x) return x;
            if (!(xn > lo && xn < hi)) { dx = 0.5 * (hi - lo); xn = lo + dx; if (xn == lo || xn == hi) return x; }
        }
        x = xn;
        f = tv_horner(lds, off, n, x);
        df = tv_horner(lds, off1, n - 1, x);
        if (f == 0.0) return x;
        if (tv_neg(f) == neg_lo) lo = x; else hi = x;
    }
    return x;
}
TV_HD int tv_real_roots(double* lds) {     // returns the count; the roots, ascending, are at TV_ROOTS_A
    int off = 0;
    for (int d = 0; d < 10; d++) {         // the ten derivatives (the tenth is the constant Newton divides by at the linear level)
        const int n = 11 - d, nxt = off + n;
        for (int i = 0; i + 1 < n; i++) TVL(nxt + i) = (double)(i + 1) * TVL(off + i + 1);
        off = nxt;
    }
    const double lead = TVL(TV_DER + 10);
    if (!(fabs(lead) > 0.0) || !isfinite(lead)) return 0;
    int m = 0;                              // roots of the derivative above (none for the linear one)
    int src = TV_ROOTS_A, dst = TV_ROOTS_B;
    for (int d = 9; d >= 0; d--) {
        const int offd = tv_der_off(d), n = 11 - d, deg = 10 - d;
        if (m == 0) { TVL(src) = 0.0; m = 1; }                       // no critical point: any break point will do
        const bool neg_pinf = tv_neg(lead), neg_ninf = (deg & 1) ? !neg_pinf : neg_pinf;
        int found = 0;
        double prev = 0.0;
        bool neg_prev = neg_ninf;
        for (int i = 0; i <= m; i++) {
            const bool last = i == m;
            const double t = last ? 0.0 : TVL(src + i);
            const bool neg_t = last ? neg_pinf : tv_neg(tv_horner(lds, offd, n, t));
            if (neg_t != neg_prev && found < deg) {
                double lo = prev, hi = t;
                bool ok = true;
                if (i == 0) {                                        // (-inf, t): walk left until the sign is the one at -inf
                    double step = 1.0 + fabs(t);
                    lo = t - step;
                    int guard = 0;
                    while (tv_neg(tv_horner(lds, offd, n, lo)) != neg_ninf && guard++ < 1100) { step *= 2.0; lo = t - step; }
                    ok = guard < 1100 && isfinite(lo);
                } else if (last) {                                   // (prev, +inf)
                    double step = 1.0 + fabs(prev);
                    hi = prev + step;
                    int guard = 0;
                    while (tv_neg(tv_horner(lds, offd, n, hi)) != neg_pinf && guard++ < 1100) { step *= 2.0; hi = prev + step; }
                    ok = guard < 1100 && isfinite(hi);
                }
                if (ok) { TVL(dst + found) = tv_close(lds, d, lo, hi, neg_prev); found++; }
            }
            prev = t;
            neg_prev = neg_t;
        }
        m = found;
        const int s = src; src = dst; dst = s;
    }
    if (src != TV_ROOTS_A)
        for (int i = 0; i < m; i++) TVL(TV_ROOTS_A + i) = TVL(src + i);
    return m;
}

// ---- 6. back-substitution and polish ---------------------------------------------------------------------------------------
TV_HD void tv_mm(const double* A, const double* B, double* C, bool ta, bool tb) {     // C = op(A) op(B), 3x3 row-major
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 3; k++) s += (ta ? A[3 * k + i] : A[3 * i + k]) * (tb ? B[3 * j + k] : B[3 * k + j]);
            C[3 * i + j] = s;
        }
}
TV_HD double tv_det3(const double* E) {
    return (E[0] * (E[4] * E[8] - E[5] * E[7]) - E[1] * (E[3] * E[8] - E[5] * E[6])) + E[2] * (E[3] * E[7] - E[4] * E[6]);
}
// r[0] = det E, r[1 + 3i + j] = (2 E E^T E - tr(E E^T) E)_ij; returns |r|^2
TV_HD double tv_residual(const double* E, double* r) {
    double G[9], M[9];
    tv_mm(E, E, G, false, true);
    tv_mm(G, E, M, false, false);
    const double tr = (G[0] + G[4]) + G[8];
    r[0] = tv_det3(E);
    double n2 = r[0] * r[0];
#pragma unroll
    for (int t = 0; t < 9; t++) { r[1 + t] = 2.0 * M[t] - tr * E[t]; n2 += r[1 + t] * r[1 + t]; }
    return n2;
}
TV_HD void tv_combine(const double* lds, double x, double y, double z, double* E) {
#pragma unroll
    for (int t = 0; t < 9; t++)
        E[t] = ((x * TVL(TV_BASIS + t) + y * TVL(TV_BASIS + 9 + t)) + z * TVL(TV_BASIS + 18 + t)) + TVL(TV_BASIS + 27 + t);
}
// Gauss-Newton on the ten constraints themselves in (x, y, z), from the root the polynomial gave: the expanded degree-10
// coefficients lose digits that the constraints, evaluated on E directly, still have.  A step is kept only if it lowers |r|.
#define TV_POLISH_STEPS 4
TV_HD void tv_polish(const double* lds, double* xyz) {
    double E[9], r[10];
    tv_combine(lds, xyz[0], xyz[1], xyz[2], E);
    double n2 = tv_residual(E, r);
    for (int it = 0; it < TV_POLISH_STEPS; it++) {
        double G[9], F[9], J[3][10];
        tv_mm(E, E, G, false, true);                     // E E^T
        tv_mm(E, E, F, true, false);                     // E^T E
        const double tr = (G[0] + G[4]) + G[8];
        const double cof[9] = {E[4] * E[8] - E[5] * E[7], E[5] * E[6] - E[3] * E[8], E[3] * E[7] - E[4] * E[6],
                               E[2] * E[7] - E[1] * E[8], E[0] * E[8] - E[2] * E[6], E[1] * E[6] - E[0] * E[7],
                               E[1] * E[5] - E[2] * E[4], E[2] * E[3] - E[0] * E[5], E[0] * E[4] - E[1] * E[3]};
#pragma unroll
        for (int c = 0; c < 3; c++) {
            double D[9], A1[9], T[9], A2[9], A3[9];
#pragma unroll
            for (int t = 0; t < 9; t++) D[t] = TVL(TV_BASIS + 9 * c + t);
            tv_mm(D, F, A1, false, false);               // D E^T E
            tv_mm(D, E, T, true, false);                 // D^T E
            tv_mm(E, T, A2, false, false);               // E D^T E
            tv_mm(G, D, A3, false, false);               // E E^T D
            double j0 = 0.0, ted = 0.0;
#pragma unroll
            for (int t = 0; t < 9; t++) { j0 += cof[t] * D[t]; ted += E[t] * D[t]; }
            J[c][0] = j0;
#pragma unroll
            for (int t = 0; t < 9; t++) J[c][1 + t] = (2.0 * ((A1[t] + A2[t]) + A3[t]) - 2.0 * ted * E[t]) - tr * D[t];
        }
        double N[3][3], g[3];
#pragma unroll
        for (int a = 0; a < 3; a++) {
#pragma unroll
            for (int b = a; b < 3; b++) {
                double sum = 0.0;
#pragma unroll
                for (int t = 0; t < 10; t++) sum += J[a][t] * J[b][t];
                N[a][b] = N[b][a] = sum;
            }
            double sum = 0.0;
#pragma unroll
            for (int t = 0; t < 10; t++) sum += J[a][t] * r[t];
            g[a] = sum;
        }
        const double c00 = N[1][1] * N[2][2] - N[1][2] * N[2][1], c01 = N[1][2] * N[2][0] - N[1][0] * N[2][2],
                     c02 = N[1][0] * N[2][1] - N[1][1] * N[2][0];
        const double det = (N[0][0] * c00 + N[0][1] * c01) + N[0][2] * c02;
        const double c11 = N[0][0] * N[2][2] - N[0][2] * N[2][0], c12 = N[0][1] * N[2][0] - N[0][0] * N[2][1],
                     c22 = N[0][0] * N[1][1] - N[0][1] * N[1][0];
        const double d0 = ((c00 * g[0] + c01 * g[1]) + c02 * g[2]) / det, d1 = ((c01 * g[0] + c11 * g[1]) + c12 * g[2]) / det,
                     d2 = ((c02 * g[0] + c12 * g[1]) + c22 * g[2]) / det;
        const double xn = xyz[0] - d0, yn = xyz[1] - d1, zn = xyz[2] - d2;
        double En[9], rn[10];
        tv_combine(lds, xn, yn, zn, En);
        const double m2 = tv_residual(En, rn);
        if (!(m2 < n2)) break;                           // (also a NaN step)
        xyz[0] = xn; xyz[1] = yn; xyz[2] = zn; n2 = m2;
#pragma unroll
        for (int t = 0; t < 9; t++) E[t] = En[t];
#pragma unroll
        for (int t = 0; t < 10; t++) r[t] = rn[t];
    }
}
TV_HD double tv_h4(const double* lds, int o, double z) { return ((TVL(o + 3) * z + TVL(o + 2)) * z + TVL(o + 1)) * z + TVL(o); }
TV_HD int tv_assemble(double* lds, int nz) {       // E per root at TV_EOUT + 9 k; returns how many were kept
    double zs[10];
    int kept = 0;
#pragma unroll
    for (int i = 0; i < 10; i++) zs[i] = i < nz ? TVL(TV_ROOTS_A + i) : 0.0;
#pragma unroll
    for (int i = 0; i < 10; i++) {
        if (i >= nz) continue;
        const double z = zs[i];
        double r[3][3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int o = TV_BPOLY + 13 * k;
            r[k][0] = tv_h4(lds, o, z);
            r[k][1] = tv_h4(lds, o + 4, z);
            r[k][2] = tv_h4(lds, o + 8, z) + ((TVL(o + 12) * z) * z) * (z * z);
        }
        double nb[3] = {0.0, 0.0, 0.0}, best = -1.0;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int a = k, b = (k + 1) % 3;
            const double n0 = r[a][1] * r[b][2] - r[a][2] * r[b][1], n1 = r[a][2] * r[b][0] - r[a][0] * r[b][2],
                         n2 = r[a][0] * r[b][1] - r[a][1] * r[b][0];
            const double nn = (n0 * n0 + n1 * n1) + n2 * n2;
            if (nn > best) { best = nn; nb[0] = n0; nb[1] = n1; nb[2] = n2; }
        }
        double xyz[3] = {nb[0] / nb[2], nb[1] / nb[2], z};
        if (!(isfinite(xyz[0]) && isfinite(xyz[1]))) continue;
        tv_polish(lds, xyz);
        double e[9], s = 0.0;
        tv_combine(lds, xyz[0], xyz[1], xyz[2], e);
#pragma unroll
        for (int t = 0; t < 9; t++) s += e[t] * e[t];
        const double inv = 1.0 / sqrt(s);
        if (!(inv > 0.0) || !isfinite(inv)) continue;
        for (int t = 0; t < 9; t++) TVL(TV_EOUT + 9 * kept + t) = e[t] * inv;
        kept++;
    }
    return kept;
}

// the whole solver for this lane's sample: x1, x2 = five normalised points each; result in LDS at TV_EOUT
TV_HD int tv_solve(double* lds, const double* x1, const double* x2) {
    tv_null_space(lds, x1, x2, false);
    tv_constraints(lds);
    if (tv_eliminate(lds) < TV_PIVOT_MIN) {             // the ten leading monomials are nearly dependent in this basis (a few
        tv_null_space(lds, x1, x2, true);               // samples in a thousand): the roots would lose most of their digits.
        tv_constraints(lds);                            // Another basis gives another system; a NaN pivot compares false and
        tv_eliminate(lds);                              // is not retried (non-finite input has no roots in any basis)
    }
    tv_bpoly(lds);
    return tv_assemble(lds, tv_real_roots(lds));
}

// ---- scoring and sampling (stated in the header) ---------------------------------------------------------------------------
TV_HD double tv_sampson_sq(const double* E, double a, double b, double c, double d) {
    const double l0 = E[0] * a + E[1] * b + E[2], l1 = E[3] * a + E[4] * b + E[5], l2 = E[6] * a + E[7] * b + E[8];
    const double m0 = E[0] * c + E[3] * d + E[6], m1 = E[1] * c + E[4] * d + E[7];
    const double r = c * l0 + d * l1 + l2;
    return r * r / (l0 * l0 + l1 * l1 + m0 * m0 + m1 * m1);
}

// cv2.decomposeEssentialMat: R1 = U W V^T, R2 = U W^T V^T (det U = det V = +1), t = the unit left null vector of E, its
// largest component (the first of equals) positive.  The SVD through the eigenvectors of E^T E (singular values 1, 1, 0
// up to scale: the squared condition does no harm here).
TV_HD void tv_decompose(const double* E, double* R1, double* R2, double* t) {
    double S[3][3], V[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = i; j < 3; j++) S[i][j] = S[j][i] = (E[i] * E[j] + E[3 + i] * E[3 + j]) + E[6 + i] * E[6 + j];
    geo_jacobi<3, 8>(S, V);
    int lo = 0;
    double lv = S[0][0];
    if (S[1][1] < lv) { lo = 1; lv = S[1][1]; }
    if (S[2][2] < lv) lo = 2;
    double v1[3], v2[3], v3[3], u1[3], u2[3], u3[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        v1[k] = lo == 0 ? V[k][1] : V[k][0];
        v2[k] = lo == 2 ? V[k][1] : V[k][2];
    }
    geo_cross(v1, v2, v3);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        u1[i] = (E[3 * i] * v1[0] + E[3 * i + 1] * v1[1]) + E[3 * i + 2] * v1[2];
        u2[i] = (E[3 * i] * v2[0] + E[3 * i + 1] * v2[1]) + E[3 * i + 2] * v2[2];
    }
    geo_unit(u1);
    const double dp = (u1[0] * u2[0] + u1[1] * u2[1]) + u1[2] * u2[2];
#pragma unroll
    for (int i = 0; i < 3; i++) u2[i] -= dp * u1[i];
    geo_unit(u2);
    geo_cross(u1, u2, u3);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double w = u1[i] * v2[j] - u2[i] * v1[j], k = u3[i] * v3[j];
            R1[3 * i + j] = w + k;
            R2[3 * i + j] = k - w;
        }
    double big = u3[0];
    if (fabs(u3[1]) > fabs(big)) big = u3[1];
    if (fabs(u3[2]) > fabs(big)) big = u3[2];
    const double sg = big < 0.0 ? -1.0 : 1.0;
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = sg * u3[i];
}
// good under [R | t]: geo_cheirality on the packed 3x4
TV_HD bool tv_cheirality(const double* R, const double* t, double a, double b, double c, double d, double dist) {
    const double P2[12] = {R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2]};
    return geo_cheirality(P2, a, b, c, d, dist);
}

#ifndef TV_HOST_ONLY
// =============================================================== kernels =====================================================

__global__ __launch_bounds__(TV_LANES) void tv_fivepoint_kernel(int S, const double* __restrict__ x1, const double* __restrict__ x2,
                                                                double* __restrict__ E, int* __restrict__ nroots) {
    __shared__ double s_lds[TV_LDS_PER_LANE * TV_LANES];
    const int lane = threadIdx.x, s = blockIdx.x * TV_LANES + lane;
    const int sc = min(s, S - 1);                       // the spare lanes of the last block solve its last sample again
    double* lds = s_lds + lane;
    double p1[10], p2[10];
#pragma unroll
    for (int i = 0; i < 10; i++) { p1[i] = x1[(size_t)sc * 10 + i]; p2[i] = x2[(size_t)sc * 10 + i]; }
    const int n = tv_solve(lds, p1, p2);
    if (s < S) {
        nroots[s] = n;
        for (int i = 0; i < 90; i++) E[(size_t)s * 90 + i] = i < 9 * n ? TVL(TV_EOUT + i) : 0.0;
    }
}

__global__ void tv_prepare_kernel(int M, int B, const double2* __restrict__ px1, const double2* __restrict__ px2, geo_cam cam,
                                  double4* __restrict__ xn, unsigned long long* __restrict__ keys, int* __restrict__ models) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < M) {
        const double2 p = px1[i], q = px2[i];
        xn[i] = make_double4((p.x - cam.cx) / cam.fx, (p.y - cam.cy) / cam.fy, (q.x - cam.cx) / cam.fx, (q.y - cam.cy) / cam.fy);
    }
    if (i < B) { keys[i] = 0ull; models[i] = 0; }
}

__device__ __forceinline__ int tv_solve_hypothesis(double* lds, const double4* xn, int n, uint64_t seed, int h) {
    int idx[5];
    geo_draw_sample<5>(seed, h, n, idx);
    double p1[10], p2[10];
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const double4 v = xn[idx[k]];
        p1[2 * k] = v.x; p1[2 * k + 1] = v.y; p2[2 * k] = v.z; p2[2 * k + 1] = v.w;
    }
    return tv_solve(lds, p1, p2);
}

// grid (ceil(H / 64), B): lane = one hypothesis of pair blockIdx.y
__global__ __launch_bounds__(TV_LANES) void tv_ransac_kernel(const int* __restrict__ offsets, int M, const double4* __restrict__ xn_all,
                                                             int H, double thr2, uint64_t seed, unsigned long long* __restrict__ keys,
                                                             int* __restrict__ models) {
    __shared__ double s_lds[TV_LDS_PER_LANE * TV_LANES];
    __shared__ unsigned long long s_key;
    __shared__ int s_models;
    const int b = blockIdx.y, lane = threadIdx.x, h = blockIdx.x * TV_LANES + lane;
    int first, last; bool bad;
    geo_range(offsets, b, M, &first, &last, &bad);
    const int n = last - first;
    if (n < 5) return;                                  // block-uniform
    if (lane == 0) { s_key = 0ull; s_models = 0; }
    __syncthreads();
    const double4* xn = xn_all + first;
    double* lds = s_lds + lane;
    const int nr = tv_solve_hypothesis(lds, xn, n, seed, min(h, H - 1));
    unsigned long long best = 0ull;
    for (int r = 0; r < nr; r++) {
        double E[9];
#pragma unroll
        for (int t = 0; t < 9; t++) E[t] = TVL(TV_EOUT + 9 * r + t);
        int count = 0;
        for (int i = 0; i < n; i++) {
            const double4 v = xn[i];
            count += tv_sampson_sq(E, v.x, v.y, v.z, v.w) < thr2 ? 1 : 0;
        }
        const unsigned long long k = geo_key3(count, h, r);
        best = k > best ? k : best;
    }
    if (h < H) {
        if (best) atomicMax(&s_key, best);
        if (nr) atomicAdd(&s_models, nr);
    }
    __syncthreads();
    if (lane == 0) {
        if (s_key) atomicMax(&keys[b], s_key);          // integer maxima and sums: the order of arrival does not matter
        if (s_models) atomicAdd(&models[b], s_models);
    }
}

// grid B: the winner of pair b solved again (every lane the same hypothesis), its matrix, mask and stats written
__global__ __launch_bounds__(TV_LANES) void tv_ransac_result_kernel(const int* __restrict__ offsets, int M, const double4* __restrict__ xn_all,
                                                                    double thr2, uint64_t seed, const unsigned long long* __restrict__ keys,
                                                                    const int* __restrict__ models, double* __restrict__ E_out,
                                                                    uint8_t* __restrict__ inlier, int* __restrict__ stats,
                                                                    unsigned int* __restrict__ index_errors) {
    __shared__ double s_lds[TV_LDS_PER_LANE * TV_LANES];
    const int b = blockIdx.x, lane = threadIdx.x;
    int first, last; bool bad;
    geo_range(offsets, b, M, &first, &last, &bad);
    if (bad && lane == 0) atomicAdd(index_errors, 1u);
    const int n = last - first;
    const unsigned long long key = n >= 5 ? keys[b] : 0ull;
    if (!key) {
        if (lane < 9) E_out[9 * b + lane] = 0.0;
        for (int i = lane; i < n; i += TV_LANES) inlier[first + i] = 0;
        if (lane == 0) { stats[4 * b] = 0; stats[4 * b + 1] = -1; stats[4 * b + 2] = -1; stats[4 * b + 3] = n >= 5 ? models[b] : 0; }
        return;
    }
    const int count = geo_key_count(key), h = geo_key3_h(key), root = geo_key3_sub(key);
    const double4* xn = xn_all + first;
    double* lds = s_lds + lane;
    tv_solve_hypothesis(lds, xn, n, seed, h);
    double E[9];
#pragma unroll
    for (int t = 0; t < 9; t++) E[t] = TVL(TV_EOUT + 9 * root + t);
    for (int i = lane; i < n; i += TV_LANES) {
        const double4 v = xn[i];
        inlier[first + i] = tv_sampson_sq(E, v.x, v.y, v.z, v.w) < thr2 ? 1 : 0;
    }
    if (lane == 0) {
#pragma unroll
        for (int t = 0; t < 9; t++) E_out[9 * b + t] = E[t];
        stats[4 * b] = count; stats[4 * b + 1] = h; stats[4 * b + 2] = root; stats[4 * b + 3] = models[b];
    }
}

#define TV_RP_THREADS 256
__global__ __launch_bounds__(TV_RP_THREADS) void tv_recover_pose_kernel(const int* __restrict__ offsets, int M, const double2* __restrict__ px1,
                                                                        const double2* __restrict__ px2, geo_cam cam,
                                                                        const double* __restrict__ E_all, const uint8_t* __restrict__ inlier_in,
                                                                        double dist, double* __restrict__ pose, uint8_t* __restrict__ inlier_out,
                                                                        int* __restrict__ stats, unsigned int* __restrict__ index_errors) {
    __shared__ int s_count[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    int first, last; bool bad;
    geo_range(offsets, b, M, &first, &last, &bad);
    if (bad && tid == 0) atomicAdd(index_errors, 1u);
    const int n = last - first;
    double E[9], nrm = 0.0;
#pragma unroll
    for (int t = 0; t < 9; t++) { E[t] = E_all[9 * b + t]; nrm += E[t] * E[t]; }
    if (!(nrm > 0.0) || !isfinite(nrm)) {               // no model (a pair of fewer than five matches): identity, no inliers
        if (tid < 12) pose[12 * b + tid] = (tid % 5 == 0) ? 1.0 : 0.0;
        for (int i = tid; i < n; i += TV_RP_THREADS) inlier_out[first + i] = 0;
        if (tid == 0) { stats[2 * b] = 0; stats[2 * b + 1] = -1; }
        return;
    }
    if (tid < 4) s_count[tid] = 0;
    __syncthreads();
    double R1[9], R2[9], t[3], tn[3];
    tv_decompose(E, R1, R2, t);
#pragma unroll
    for (int i = 0; i < 3; i++) tn[i] = -t[i];
    int mine[4] = {0, 0, 0, 0};
    for (int i = tid; i < n; i += TV_RP_THREADS) {
        if (inlier_in && !inlier_in[first + i]) continue;
        const double2 p = px1[first + i], q = px2[first + i];
        const double a = (p.x - cam.cx) / cam.fx, bb = (p.y - cam.cy) / cam.fy, c = (q.x - cam.cx) / cam.fx, d = (q.y - cam.cy) / cam.fy;
        mine[0] += tv_cheirality(R1, t, a, bb, c, d, dist) ? 1 : 0;
        mine[1] += tv_cheirality(R2, t, a, bb, c, d, dist) ? 1 : 0;
        mine[2] += tv_cheirality(R1, tn, a, bb, c, d, dist) ? 1 : 0;
        mine[3] += tv_cheirality(R2, tn, a, bb, c, d, dist) ? 1 : 0;
    }
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (mine[k]) atomicAdd(&s_count[k], mine[k]);
    __syncthreads();
    int win = 0;
#pragma unroll
    for (int k = 1; k < 4; k++)
        if (s_count[k] > s_count[win]) win = k;
    const double* R = (win & 1) ? R2 : R1;
    const double* tt = (win & 2) ? tn : t;
    for (int i = tid; i < n; i += TV_RP_THREADS) {
        uint8_t good = 0;
        if (!inlier_in || inlier_in[first + i]) {
            const double2 p = px1[first + i], q = px2[first + i];
            good = tv_cheirality(R, tt, (p.x - cam.cx) / cam.fx, (p.y - cam.cy) / cam.fy, (q.x - cam.cx) / cam.fx,
                                 (q.y - cam.cy) / cam.fy, dist) ? 1 : 0;
        }
        inlier_out[first + i] = good;
    }
    if (tid < 12) pose[12 * b + tid] = (tid & 3) == 3 ? tt[tid >> 2] : R[3 * (tid >> 2) + (tid & 3)];
    if (tid == 0) { stats[2 * b] = s_count[win]; stats[2 * b + 1] = win; }
}

__global__ void tv_triangulate_kernel(int N, const double* __restrict__ P1, const double* __restrict__ P2, const double2* __restrict__ x1,
                                      const double2* __restrict__ x2, double* __restrict__ X, double* __restrict__ w) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    double p1[12], p2[12], v[4];
#pragma unroll
    for (int k = 0; k < 12; k++) { p1[k] = P1[k]; p2[k] = P2[k]; }
    const double2 a = x1[i], c = x2[i];
    geo_triangulate_point(p1, p2, a.x, a.y, c.x, c.y, v);
    X[3 * (size_t)i] = v[0] / v[3];
    X[3 * (size_t)i + 1] = v[1] / v[3];
    X[3 * (size_t)i + 2] = v[2] / v[3];
    w[i] = v[3];
}

// =============================================================== entry points ================================================
#include "geometry_host.h"           // the checks, the vote block and the launch shapes the four estimators' entry points share

extern "C" int slam_tv_fivepoint_f64(slam_ctx* ctx, int64_t S, const double* d_x1, const double* d_x2, double* d_E, int32_t* d_nroots) {
    GEO_SAMPLE_SIZES(ctx, S);
    GEO_POINTERS(S, d_x1 && d_x2 && d_E && d_nroots);
    SLAM_HIP(hipSetDevice(ctx->device));
    tv_fivepoint_kernel<<<geo_blocks(S, TV_LANES), TV_LANES, 0, ctx->stream>>>((int)S, d_x1, d_x2, d_E, d_nroots);
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

extern "C" int slam_tv_essential_ransac_f64(slam_ctx* ctx, int64_t B, const int32_t* d_offsets, const double* d_px1, const double* d_px2,
                                            int64_t M, double fx, double fy, double cx, double cy, int H, double threshold_px, uint64_t seed,
                                            double* d_E, uint8_t* d_inlier, int32_t* d_stats) {
    GEO_RANSAC_SIZES(ctx, B, M, H);
    SLAM_REQUIRE(threshold_px > 0.0 && fx > 0.0 && fy > 0.0, "threshold and focal lengths must be positive");
    GEO_POINTERS(B, d_offsets && d_E && d_stats && (M == 0 || (d_px1 && d_px2 && d_inlier)));
    SLAM_REQUIRE((((uintptr_t)d_px1 | (uintptr_t)d_px2) & 15) == 0, "d_px1 / d_px2 must be 16-byte aligned");
    SLAM_HIP(hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> lk(ctx->call_mu);        // the workspace holds the normalised points, the keys and the model counts
    const uint64_t xn_bytes = (uint64_t)(M > 0 ? M : 1) * 32;
    void* ws = nullptr;
    if (int rc = slam_workspace(ctx, geo_vote_bytes(xn_bytes, B), &ws)) return rc;
    double4* xn = (double4*)ws;
    unsigned long long* keys; int* models;
    if (int rc = geo_vote_block(ctx, ws, xn_bytes, B, false, M, d_inlier, &keys, &models)) return rc;    // tv_prepare_kernel clears them
    const geo_cam cam = {fx, fy, cx, cy};
    const double thr = threshold_px / ((fx + fy) / 2.0), thr2 = thr * thr;
    tv_prepare_kernel<<<geo_blocks(M > B ? M : B, 256), 256, 0, ctx->stream>>>((int)M, (int)B, (const double2*)d_px1, (const double2*)d_px2, cam,
                                                                               xn, keys, models);
    SLAM_HIP(hipGetLastError());
    tv_ransac_kernel<<<geo_vote_grid(H, TV_LANES, B), TV_LANES, 0, ctx->stream>>>(d_offsets, (int)M, xn, H, thr2, seed, keys, models);
    SLAM_HIP(hipGetLastError());
    tv_ransac_result_kernel<<<(unsigned)B, TV_LANES, 0, ctx->stream>>>(d_offsets, (int)M, xn, thr2, seed, keys, models, d_E, d_inlier, d_stats,
                                                                      slam_index_error_counter(ctx));
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

extern "C" int slam_tv_recover_pose_f64(slam_ctx* ctx, int64_t B, const int32_t* d_offsets, const double* d_px1, const double* d_px2,
                                        int64_t M, double fx, double fy, double cx, double cy, const double* d_E,
                                        const uint8_t* d_inlier_in, double distance_thresh, double* d_pose, uint8_t* d_inlier_out,
                                        int32_t* d_stats) {
    GEO_CANDIDATE_SIZES(ctx, B, 1 << 20, M);
    SLAM_REQUIRE(fx > 0.0 && fy > 0.0 && distance_thresh > 0.0, "focal lengths and distance_thresh must be positive");
    GEO_POINTERS(B, d_offsets && d_E && d_pose && d_stats && (M == 0 || (d_px1 && d_px2 && d_inlier_out)));
    SLAM_REQUIRE((((uintptr_t)d_px1 | (uintptr_t)d_px2) & 15) == 0, "d_px1 / d_px2 must be 16-byte aligned");
    SLAM_HIP(hipSetDevice(ctx->device));
    const geo_cam cam = {fx, fy, cx, cy};
    if (M > 0) SLAM_HIP(hipMemsetAsync(d_inlier_out, 0, (size_t)M, ctx->stream));
    tv_recover_pose_kernel<<<(unsigned)B, TV_RP_THREADS, 0, ctx->stream>>>(d_offsets, (int)M, (const double2*)d_px1, (const double2*)d_px2, cam,
                                                                          d_E, d_inlier_in, distance_thresh, d_pose, d_inlier_out, d_stats,
                                                                          slam_index_error_counter(ctx));
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

extern "C" int slam_tv_triangulate_f64(slam_ctx* ctx, int64_t N, const double* d_P1, const double* d_P2, const double* d_x1,
                                       const double* d_x2, double* d_X, double* d_w) {
    SLAM_REQUIRE(ctx, "slam_tv_triangulate_f64: null ctx");
    SLAM_REQUIRE(N >= 0 && N <= (1 << 28), "N=%lld out of range [0, 2^28]", (long long)N);
    GEO_POINTERS(N, d_P1 && d_P2 && d_x1 && d_x2 && d_X && d_w);
    SLAM_REQUIRE((((uintptr_t)d_x1 | (uintptr_t)d_x2) & 15) == 0, "d_x1 / d_x2 must be 16-byte aligned");
    SLAM_HIP(hipSetDevice(ctx->device));
    tv_triangulate_kernel<<<geo_blocks(N, 256), 256, 0, ctx->stream>>>((int)N, d_P1, d_P2, (const double2*)d_x1, (const double2*)d_x2, d_X,
                                                                       d_w);
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}
#endif  // TV_HOST_ONLY
