// homography.hip — batched homography estimation on gfx950: cv2.findHomography (RANSAC), cv2.decomposeHomographyMat with the
// cheirality vote of cv2.recoverPose, and ORB-SLAM's H / E model scores, for MANY frame pairs in one call.  The reference
// leaves this branch of pose_estimation_2d2d unwritten (utils.py:27-29: raise NotImplementedError above a commented-out
// findHomography(source_pts, query_pts, method=RANSAC, ransacReprojThreshold=3)).
//
//   slam_hg_fourpoint_f64     the minimal solver on its own: the homography through four correspondences
//   slam_hg_ransac_f64        H hypotheses per pair, each scored on all matches by the one-way transfer error in pixels
//   slam_hg_decompose_f64     H -> up to four (R, t, n), the cheirality vote among them, the rotation-only case
//   slam_hg_model_score_f64   S_H, S_E of ORB-SLAM's initialiser as exact fixed-point integers, and R_H = S_H / (S_H + S_E)
//
// All arithmetic is f64 and the file is compiled with floating-point contraction OFF (the pragma below), as two_view.hip and
// pnp.hip: the winning hypothesis is solved again by the kernel that writes the result and must come out bit for bit as it
// was scored, and the host build of these routines (HG_HOST_ONLY, the test suite's twin) must give the device's bits.  For
// the same reason only + - * / sqrt are used.
//
// The solver.  Four points in general position are a projective basis, so the null vector of the 8x9 DLT system has a closed
// form in cofactors and needs neither an elimination order nor a pivot, and no entry of H is assumed non-zero:
//   1. both point sets Hartley-normalised (centroid to the origin, mean distance sqrt 2): p_i, q_i homogeneous, i = 0..3;
//   2. the correspondence whose opposite triangle is the largest changes places with the fourth (the only choice the solver
//      makes: the rounding errors of what follows are divided by the area of the base triangle [p0 p1 p2]);
//      l = adj([p0 p1 p2]) p3, i.e. l0 = det[p1 p2 p3], l1 = det[p2 p0 p3], l2 = det[p0 p1 p3] (twice the signed areas, from
//      coordinate differences); m the same of q.  A triangle of the four with sin^2 of any angle below 1e-20 in either
//      image, or with opposite orientation in the two images, ends the sample: no model;
//   3. Hn = sum_i c_i q_i (p_j x p_k)^T over the cyclic (i, j, k), c_i = m_i l_j l_k: Hn p_i ~ q_i for all four;
//   4. H = T2^-1 Hn T1, scaled to Frobenius norm 1, the sign that makes the sum of the four projective weights
//      h6 x + h7 y + h8 positive; then every one of the four must be positive (it is, up to rounding, when the
//      orientations agree), else no model.
// One sample per lane, straight-line code in registers: no run-time-indexed array, so nothing goes to scratch.
//
// The decomposition (Ma, Soatto, Kosecka, Sastry, "An Invitation to 3-D Vision", 5.3.3), through the eigenvectors of
// Hn^T Hn by cyclic Jacobi: see hg_candidates.  The Jacobi sweeps, the triangulation and the cheirality test are
// geometry_common.h's, the ones two_view.hip runs: the vote is defined as "triangulated as slam_tv_triangulate_f64".
#ifndef HG_HOST_ONLY                 // a host build of the routines alone (the test suite's twin) defines it
#include "internal.h"
#endif
#include <math.h>
#include <stdint.h>
#include "geometry_common.h"         // sampler, Jacobi, triangulation, cheirality, range clamp, intrinsics, model key, three-vectors

#pragma clang fp contract(off)

#define HG_HD __host__ __device__ __forceinline__
// the shared routines, key and intrinsics under this file's names, as its host twin calls them (four matches per sample)
#define hg_draw_sample geo_draw_sample<4>
#define hg_cheirality geo_cheirality
#define hg_key geo_key2
#define HG_H_MAX GEO_H_MAX
typedef geo_cam hg_cam;
#define HG_ROTATION_ONLY 1e-9        // (s1 - s3) / s2 below this: H is a rotation, no translation is reported.  The numpy
                                     // reference measures 2.4e-16 on pure_rotation/t0 (this file's Jacobi: 8.4e-16) and 1.25e-6
                                     // on pure_rotation/b1e-6 (profiles/homography_edges.log); the bound lies between the two
#define HG_CHI2_H 5.991              // chi-square, 2 degrees of freedom, 95 %
#define HG_CHI2_E 3.841              // chi-square, 1 degree of freedom, 95 %
#define HG_FIXED 1048576.0           // 2^20: a score term becomes (int64)(term * 2^20)

// ---- the minimal solver -------------------------------------------------------------------------------------------------------
HG_HD double hg_min(double a, double b) { return a < b ? a : b; }
// twice the signed area of the triangle (a, b, c); *flat: sin^2 of one of its angles is below GEO_FLAT (or a vertex repeats)
HG_HD double hg_area2(double ax, double ay, double bx, double by, double cx, double cy, bool* flat) {
    const double ux = bx - ax, uy = by - ay, vx = cx - ax, vy = cy - ay, wx = cx - bx, wy = cy - by;
    const double cr = ux * vy - uy * vx, c2 = cr * cr;
    const double lu = ux * ux + uy * uy, lv = vx * vx + vy * vy, lw = wx * wx + wy * wy;
    *flat = !(c2 > GEO_FLAT * (lu * lv)) || !(c2 > GEO_FLAT * (lu * lw)) || !(c2 > GEO_FLAT * (lv * lw));
    return cr;
}
// Hartley normalisation of four points p [8]: n [8] = s (p - c); returns false if the mean distance is not a positive finite double
HG_HD bool hg_hartley(const double* p, double* n, double* s, double* cx, double* cy) {
    *cx = (((p[0] + p[2]) + p[4]) + p[6]) * 0.25;
    *cy = (((p[1] + p[3]) + p[5]) + p[7]) * 0.25;
    double d = 0.0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const double dx = p[2 * k] - *cx, dy = p[2 * k + 1] - *cy;
        d += sqrt(dx * dx + dy * dy);
    }
    d *= 0.25;
    if (!(d > 0.0) || !isfinite(d)) return false;
    *s = 1.4142135623730951 / d;
#pragma unroll
    for (int k = 0; k < 4; k++) { n[2 * k] = *s * (p[2 * k] - *cx); n[2 * k + 1] = *s * (p[2 * k + 1] - *cy); }
    return true;
}
// p1, p2 [8]: four points (x, y) of image 1 and of image 2; H [9] row-major with p2 ~ H p1.  false: no model, H = 0.
HG_HD bool hg_fourpoint(const double* p1, const double* p2, double* H) {
#pragma unroll
    for (int i = 0; i < 9; i++) H[i] = 0.0;
    double big = 0.0;
#pragma unroll
    for (int i = 0; i < 8; i++) big += p1[i] * p1[i];
#pragma unroll
    for (int i = 0; i < 8; i++) big += p2[i] * p2[i];
    if (!(big < GEO_BIG)) return false;                           // NaN, inf, coordinates beyond 1e100
    double p[8], q[8], s1, c1x, c1y, s2, c2x, c2y;
    if (!hg_hartley(p1, p, &s1, &c1x, &c1y) || !hg_hartley(p2, q, &s2, &c2x, &c2y)) return false;
    bool f0, f1, f2, f3, g0, g1, g2, g3;
    {
        // The point left out of the base triangle [p0 p1 p2] is the one whose opposite triangle is the largest (the smaller of
        // its two images' areas; of equals the first in the order 3, 2, 1, 0): every rounding error below is divided by that
        // area.  It changes places with point 3; H does not depend on the order of the correspondences.
        const double t0 = hg_min(fabs(hg_area2(p[2], p[3], p[4], p[5], p[6], p[7], &f0)), fabs(hg_area2(q[2], q[3], q[4], q[5], q[6], q[7], &g0)));
        const double t1 = hg_min(fabs(hg_area2(p[4], p[5], p[0], p[1], p[6], p[7], &f1)), fabs(hg_area2(q[4], q[5], q[0], q[1], q[6], q[7], &g1)));
        const double t2 = hg_min(fabs(hg_area2(p[0], p[1], p[2], p[3], p[6], p[7], &f2)), fabs(hg_area2(q[0], q[1], q[2], q[3], q[6], q[7], &g2)));
        const double t3 = hg_min(fabs(hg_area2(p[0], p[1], p[2], p[3], p[4], p[5], &f3)), fabs(hg_area2(q[0], q[1], q[2], q[3], q[4], q[5], &g3)));
        int j = 3;
        double tb = t3;
        if (t2 > tb) { j = 2; tb = t2; }
        if (t1 > tb) { j = 1; tb = t1; }
        if (t0 > tb) { j = 0; tb = t0; }
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const bool sw = j == k;
#pragma unroll
            for (int c = 0; c < 2; c++) {
                const double a = p[2 * k + c], b = p[6 + c], e = q[2 * k + c], g = q[6 + c];
                p[2 * k + c] = sw ? b : a; p[6 + c] = sw ? a : b;
                q[2 * k + c] = sw ? g : e; q[6 + c] = sw ? e : g;
            }
        }
    }
    const double l0 = hg_area2(p[2], p[3], p[4], p[5], p[6], p[7], &f0);      // det[p1 p2 p3]
    const double l1 = hg_area2(p[4], p[5], p[0], p[1], p[6], p[7], &f1);      // det[p2 p0 p3]
    const double l2 = hg_area2(p[0], p[1], p[2], p[3], p[6], p[7], &f2);      // det[p0 p1 p3]
    const double l3 = hg_area2(p[0], p[1], p[2], p[3], p[4], p[5], &f3);      // det[p0 p1 p2]
    const double m0 = hg_area2(q[2], q[3], q[4], q[5], q[6], q[7], &g0);
    const double m1 = hg_area2(q[4], q[5], q[0], q[1], q[6], q[7], &g1);
    const double m2 = hg_area2(q[0], q[1], q[2], q[3], q[6], q[7], &g2);
    const double m3 = hg_area2(q[0], q[1], q[2], q[3], q[4], q[5], &g3);
    if (f0 || f1 || f2 || f3 || g0 || g1 || g2 || g3) return false;           // collinear or repeated points
    if (!(l0 * m0 > 0.0 && l1 * m1 > 0.0 && l2 * m2 > 0.0 && l3 * m3 > 0.0)) return false;      // a triangle turned over
    const double c0 = m0 * (l1 * l2), c1 = m1 * (l0 * l2), c2 = m2 * (l0 * l1);
    // rows of adj([p0 p1 p2]): p1 x p2, p2 x p0, p0 x p1 (third coordinates 1)
    const double a0[3] = {p[3] - p[5], p[4] - p[2], p[2] * p[5] - p[4] * p[3]};
    const double a1[3] = {p[5] - p[1], p[0] - p[4], p[4] * p[1] - p[0] * p[5]};
    const double a2[3] = {p[1] - p[3], p[2] - p[0], p[0] * p[3] - p[2] * p[1]};
    double N[9];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const double t0 = c0 * a0[j], t1 = c1 * a1[j], t2 = c2 * a2[j];
        N[j] = (q[0] * t0 + q[2] * t1) + q[4] * t2;
        N[3 + j] = (q[1] * t0 + q[3] * t1) + q[5] * t2;
        N[6 + j] = (t0 + t1) + t2;
    }
    // G = N T1, T1 = [s1 0 -s1 c1x; 0 s1 -s1 c1y; 0 0 1];  H = T2^-1 G, T2^-1 = [1/s2 0 c2x; 0 1/s2 c2y; 0 0 1]
    double G[9];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        G[3 * i] = s1 * N[3 * i];
        G[3 * i + 1] = s1 * N[3 * i + 1];
        G[3 * i + 2] = N[3 * i + 2] - (c1x * G[3 * i] + c1y * G[3 * i + 1]);
    }
    double T[9], nrm = 0.0;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        T[j] = G[j] / s2 + c2x * G[6 + j];
        T[3 + j] = G[3 + j] / s2 + c2y * G[6 + j];
        T[6 + j] = G[6 + j];
    }
#pragma unroll
    for (int i = 0; i < 9; i++) nrm += T[i] * T[i];
    nrm = sqrt(nrm);
    if (!(nrm > 0.0) || !isfinite(nrm)) return false;
#pragma unroll
    for (int i = 0; i < 9; i++) T[i] /= nrm;
    const double w0 = (T[6] * p1[0] + T[7] * p1[1]) + T[8], w1 = (T[6] * p1[2] + T[7] * p1[3]) + T[8];
    const double w2 = (T[6] * p1[4] + T[7] * p1[5]) + T[8], w3 = (T[6] * p1[6] + T[7] * p1[7]) + T[8];
    const double sg = ((w0 + w1) + (w2 + w3)) < 0.0 ? -1.0 : 1.0;
    if (!(sg * w0 > 0.0 && sg * w1 > 0.0 && sg * w2 > 0.0 && sg * w3 > 0.0)) return false;
    double chk = 0.0;
#pragma unroll
    for (int i = 0; i < 9; i++) { T[i] *= sg; chk += T[i]; }
    if (!isfinite(chk)) return false;
#pragma unroll
    for (int i = 0; i < 9; i++) H[i] = T[i];
    return true;
}

// ---- scoring and sampling (stated in the header) ---------------------------------------------------------------------------
HG_HD bool hg_inlier(const double* H, double x, double y, double u, double v, double thr2) {
    const double w = (H[6] * x + H[7] * y) + H[8];
    const double du = ((H[0] * x + H[1] * y) + H[2]) / w - u;
    const double dv = ((H[3] * x + H[4] * y) + H[5]) / w - v;
    return (w > 0.0) & ((du * du + dv * dv) < thr2);
}
// hypothesis h of a pair of n matches px1 / px2 [n,2]: its sample drawn and solved
HG_HD bool hg_solve_hypothesis(const double* px1, const double* px2, int n, uint64_t seed, int h, double* H) {
    int idx[4] = {0, 0, 0, 0};
    geo_draw_sample<4>(seed, h, n, idx);
    double a[8], b[8];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        a[2 * k] = px1[2 * (size_t)idx[k]]; a[2 * k + 1] = px1[2 * (size_t)idx[k] + 1];
        b[2 * k] = px2[2 * (size_t)idx[k]]; b[2 * k + 1] = px2[2 * (size_t)idx[k] + 1];
    }
    return hg_fourpoint(a, b, H);
}

// ---- the decomposition ---------------------------------------------------------------------------------------------------------
HG_HD void hg_mv(const double* M, const double* v, double* r) {
#pragma unroll
    for (int i = 0; i < 3; i++) r[i] = (M[3 * i] * v[0] + M[3 * i + 1] * v[1]) + M[3 * i + 2] * v[2];
}
// a takes the sign that makes its largest-magnitude component (the first of equals) positive; returns that sign
HG_HD double hg_fix_sign(double* a) {
    double big = a[0];
    if (fabs(a[1]) > fabs(big)) big = a[1];
    if (fabs(a[2]) > fabs(big)) big = a[2];
    const double sg = big < 0.0 ? -1.0 : 1.0;
    a[0] *= sg; a[1] *= sg; a[2] *= sg;
    return sg;
}
// Hn = K^-1 H K, operation by operation as the header states it
HG_HD void hg_to_normalised(const double* H, const geo_cam& cam, double* Hn) {
    double G[9];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        G[3 * i] = cam.fx * H[3 * i];
        G[3 * i + 1] = cam.fy * H[3 * i + 1];
        G[3 * i + 2] = (cam.cx * H[3 * i] + cam.cy * H[3 * i + 1]) + H[3 * i + 2];
    }
#pragma unroll
    for (int j = 0; j < 3; j++) {
        Hn[j] = (G[j] - cam.cx * G[6 + j]) / cam.fx;
        Hn[3 + j] = (G[3 + j] - cam.cy * G[6 + j]) / cam.fy;
        Hn[6 + j] = G[6 + j];
    }
}
// Singular values of Hn, descending, in sv [3] and its right singular vectors v1, v3 (of s1, s3) from the eigenvectors of
// Hn^T Hn; each of v1, v3 with its largest-magnitude component positive.  false: H or Hn has a sum of squares that is not a
// positive finite double, or s2 is not one (sv is then zero).
HG_HD bool hg_singular(const double* H, const geo_cam& cam, double* Hn, double* sv, double* v1, double* v3) {
    sv[0] = sv[1] = sv[2] = 0.0;
    double nrm = 0.0;
#pragma unroll
    for (int i = 0; i < 9; i++) nrm += H[i] * H[i];
    if (!(nrm > 0.0) || !isfinite(nrm)) return false;
    hg_to_normalised(H, cam, Hn);
    nrm = 0.0;
#pragma unroll
    for (int i = 0; i < 9; i++) nrm += Hn[i] * Hn[i];
    if (!(nrm > 0.0) || !isfinite(nrm)) return false;
    double S[3][3], V[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = i; j < 3; j++) S[i][j] = S[j][i] = (Hn[i] * Hn[j] + Hn[3 + i] * Hn[3 + j]) + Hn[6 + i] * Hn[6 + j];
    geo_jacobi<3, 8>(S, V);
    const double e0 = S[0][0], e1 = S[1][1], e2 = S[2][2];
    // hi: the largest (first of equals), lo: the smallest (last of equals), mid: the remaining one
    int hi = 0, lo = 2;
    if (e1 > e0) hi = 1;
    if (e2 > (hi == 0 ? e0 : e1)) hi = 2;
    if (hi == 2) lo = e1 < e0 ? 1 : 0;
    else { const double other = hi == 0 ? e1 : e0; lo = e2 <= other ? 2 : (hi == 0 ? 1 : 0); }
    const int mid = 3 - hi - lo;
    const double eh = hi == 0 ? e0 : hi == 1 ? e1 : e2, em = mid == 0 ? e0 : mid == 1 ? e1 : e2, el = lo == 0 ? e0 : lo == 1 ? e1 : e2;
    const double s1 = sqrt(eh > 0.0 ? eh : 0.0), s2 = sqrt(em > 0.0 ? em : 0.0), s3 = sqrt(el > 0.0 ? el : 0.0);
    if (!(s2 > 0.0) || !isfinite((s1 + s2) + s3)) return false;
    sv[0] = s1; sv[1] = s2; sv[2] = s3;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        v1[k] = hi == 0 ? V[k][0] : hi == 1 ? V[k][1] : V[k][2];
        v3[k] = lo == 0 ? V[k][0] : lo == 1 ? V[k][1] : V[k][2];
    }
    hg_fix_sign(v1);
    hg_fix_sign(v3);
    return true;
}
// The nearest rotation of Hs (= sg Hn / s2) when its singular values are equal to HG_ROTATION_ONLY: R = U V^T with
// v2 = v3 x v1, u1 = unit(Hs v1), u2 = unit(Hs v2 - (u1 . Hs v2) u1), u3 = u1 x u2: orthonormal with det +1 to rounding.
HG_HD void hg_nearest_rotation(const double* Hs, const double* v1, const double* v3, double* R) {
    double v2[3], u1[3], u2[3], u3[3], w3[3];
    geo_cross(v3, v1, v2);
    geo_unit(v2);
    geo_cross(v1, v2, w3);                                        // v3 again, exactly orthogonal to v1 and v2
    hg_mv(Hs, v1, u1);
    hg_mv(Hs, v2, u2);
    geo_unit(u1);
    const double dp = geo_dot(u1, u2);
#pragma unroll
    for (int i = 0; i < 3; i++) u2[i] -= dp * u1[i];
    geo_unit(u2);
    geo_cross(u1, u2, u3);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) R[3 * i + j] = (u1[i] * v1[j] + u2[i] * v2[j]) + u3[i] * w3[j];
}
// The four candidates of Hs (middle singular value 1, sign chosen), sg1 = s1 / s2, sg3 = s3 / s2, v1 / v3 from hg_singular:
//   v2 = v3 x v1;  a = sqrt(1 - sg3^2), b = sqrt(sg1^2 - 1) (a negative radicand, a rounding effect, counts as 0);
//   ua = unit(a v1 + b v3), ub = unit(a v1 - b v3): the two unit vectors orthogonal to v2 whose length Hs preserves;
//   per u:  n = v2 x u;  w1 = unit(Hs v2), w2 = unit(Hs u - (w1 . Hs u) w1), w3 = w1 x w2;  R = w1 v2^T + w2 u^T + w3 n^T;
//           t = (Hs - R) n, scaled to unit length (zero if its length is not a positive finite double);
//           (t, n) both change sign if the largest-magnitude component of n (the first of equals) is negative.
// pose [48]: (Ra, ta), (Ra, -ta), (Rb, tb), (Rb, -tb) as row-major 3x4; normal [12]: na, -na, nb, -nb.
HG_HD void hg_candidates(const double* Hs, double sg1, double sg3, const double* v1, const double* v3, double* pose, double* normal) {
    double v2[3], w1[3];
    geo_cross(v3, v1, v2);
    geo_unit(v2);
    hg_mv(Hs, v2, w1);
    geo_unit(w1);
    const double ra = 1.0 - sg3 * sg3, rb = sg1 * sg1 - 1.0;
    const double a = sqrt(ra > 0.0 ? ra : 0.0), b = sqrt(rb > 0.0 ? rb : 0.0);
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const double bs = c == 0 ? b : -b;
        double u[3], n[3], hu[3], w2[3], w3[3], R[9], Rn[3], Hsn[3], t[3];
#pragma unroll
        for (int i = 0; i < 3; i++) u[i] = a * v1[i] + bs * v3[i];
        geo_unit(u);
        geo_cross(v2, u, n);
        hg_mv(Hs, u, hu);
        const double dp = geo_dot(w1, hu);
#pragma unroll
        for (int i = 0; i < 3; i++) w2[i] = hu[i] - dp * w1[i];
        geo_unit(w2);
        geo_cross(w1, w2, w3);
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) R[3 * i + j] = (w1[i] * v2[j] + w2[i] * u[j]) + w3[i] * n[j];
        hg_mv(R, n, Rn);
        hg_mv(Hs, n, Hsn);
#pragma unroll
        for (int i = 0; i < 3; i++) t[i] = Hsn[i] - Rn[i];
        const double len = sqrt(geo_dot(t, t));
        const bool has = len > 0.0 && isfinite(len);
        const double sg = hg_fix_sign(n);
#pragma unroll
        for (int i = 0; i < 3; i++) t[i] = has ? sg * (t[i] / len) : 0.0;
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const double pm = k == 0 ? 1.0 : -1.0;
            double* P = pose + 12 * (2 * c + k);
#pragma unroll
            for (int i = 0; i < 3; i++) {
#pragma unroll
                for (int j = 0; j < 3; j++) P[4 * i + j] = R[3 * i + j];
                P[4 * i + 3] = pm * t[i];
                normal[3 * (2 * c + k) + i] = pm * n[i];
            }
        }
    }
}
// x2^T Hs x1 in normalised coordinates (the sign vote of the decomposition)
HG_HD double hg_bilinear(const double* Hs, double a, double b, double c, double d) {
    const double r0 = (Hs[0] * a + Hs[1] * b) + Hs[2], r1 = (Hs[3] * a + Hs[4] * b) + Hs[5], r2 = (Hs[6] * a + Hs[7] * b) + Hs[8];
    return (c * r0 + d * r1) + r2;
}

// ---- ORB-SLAM's model scores -------------------------------------------------------------------------------------------------
// adjugate of H, entry by entry as the header states it
HG_HD void hg_adjugate(const double* h, double* a) {
    a[0] = h[4] * h[8] - h[5] * h[7]; a[1] = h[2] * h[7] - h[1] * h[8]; a[2] = h[1] * h[5] - h[2] * h[4];
    a[3] = h[5] * h[6] - h[3] * h[8]; a[4] = h[0] * h[8] - h[2] * h[6]; a[5] = h[2] * h[3] - h[0] * h[5];
    a[6] = h[3] * h[7] - h[4] * h[6]; a[7] = h[1] * h[6] - h[0] * h[7]; a[8] = h[0] * h[4] - h[1] * h[3];
}
// F = K^-T E K^-1, operation by operation as the header states it
HG_HD void hg_fundamental(const double* E, const geo_cam& cam, double* F) {
    double A[9];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        A[3 * i] = E[3 * i] / cam.fx;
        A[3 * i + 1] = E[3 * i + 1] / cam.fy;
        A[3 * i + 2] = E[3 * i + 2] - (cam.cx * A[3 * i] + cam.cy * A[3 * i + 1]);
    }
#pragma unroll
    for (int j = 0; j < 3; j++) {
        F[j] = A[j] / cam.fx;
        F[3 + j] = A[3 + j] / cam.fy;
        F[6 + j] = A[6 + j] - (cam.cx * F[j] + cam.cy * F[3 + j]);
    }
}
HG_HD double hg_transfer_sq(const double* H, double x, double y, double u, double v) {
    const double w = (H[6] * x + H[7] * y) + H[8];
    const double du = ((H[0] * x + H[1] * y) + H[2]) / w - u;
    const double dv = ((H[3] * x + H[4] * y) + H[5]) / w - v;
    return du * du + dv * dv;
}
HG_HD long long hg_term(double chi, double gate) {               // NaN: chi < gate is false, nothing is added
    return chi < gate ? (long long)((HG_CHI2_H - chi) * HG_FIXED) : 0ll;
}
// the fixed-point terms of one match (x, y) -> (u, v): *sh += the two transfer terms, *se += the two epipolar terms
HG_HD void hg_score_match(const double* H, const double* Hi, const double* F, double x, double y, double u, double v, double sigma2,
                          long long* sh, long long* se) {
    *sh += hg_term(hg_transfer_sq(H, x, y, u, v) / sigma2, HG_CHI2_H);
    *sh += hg_term(hg_transfer_sq(Hi, u, v, x, y) / sigma2, HG_CHI2_H);
    const double l0 = (F[0] * x + F[1] * y) + F[2], l1 = (F[3] * x + F[4] * y) + F[5], l2 = (F[6] * x + F[7] * y) + F[8];
    const double m0 = (F[0] * u + F[3] * v) + F[6], m1 = (F[1] * u + F[4] * v) + F[7];
    const double r = (u * l0 + v * l1) + l2, r2 = r * r;
    *se += hg_term((r2 / (l0 * l0 + l1 * l1)) / sigma2, HG_CHI2_E);
    *se += hg_term((r2 / (m0 * m0 + m1 * m1)) / sigma2, HG_CHI2_E);
}
HG_HD double hg_ratio(long long sh, long long se) {
    return (sh + se) > 0 ? (double)sh / (double)(sh + se) : 0.0;
}

#ifndef HG_HOST_ONLY
// =============================================================== kernels =====================================================
#define HG_LANES 64
#define HG_THREADS 256               // hypotheses per block of the RANSAC kernel; threads per pair of the other two
#define HG_CHUNK 256                 // matches staged in LDS at a time (4 doubles each: 8 KiB)

__global__ __launch_bounds__(HG_LANES) void hg_fourpoint_kernel(int S, const double* __restrict__ p1, const double* __restrict__ p2,
                                                                double* __restrict__ H, int* __restrict__ ok) {
    const int s = blockIdx.x * HG_LANES + threadIdx.x;
    if (s >= S) return;
    double a[8], b[8], T[9];
#pragma unroll
    for (int i = 0; i < 8; i++) { a[i] = p1[(size_t)s * 8 + i]; b[i] = p2[(size_t)s * 8 + i]; }
    ok[s] = hg_fourpoint(a, b, T) ? 1 : 0;
#pragma unroll
    for (int i = 0; i < 9; i++) H[(size_t)s * 9 + i] = T[i];
}

// grid (ceil(H / 256), B): lane = one hypothesis of pair blockIdx.y; the pair's matches pass through LDS in chunks and are
// read as broadcasts (a wave's 64 hypotheses score the same match at the same time)
__global__ __launch_bounds__(HG_THREADS) void hg_ransac_kernel(const int* __restrict__ offsets, int M, const double* __restrict__ px1_all,
                                                               const double* __restrict__ px2_all, int H, double thr2, uint64_t seed,
                                                               unsigned long long* __restrict__ keys, int* __restrict__ models) {
    __shared__ double s_pt[HG_CHUNK * 4];
    __shared__ unsigned long long s_key;
    __shared__ int s_models;
    const int b = blockIdx.y, tid = threadIdx.x, h = blockIdx.x * HG_THREADS + tid;
    int first, last; bool bad;
    geo_range(offsets, b, M, &first, &last, &bad);
    const int n = last - first;
    if (n < 4) return;                                  // block-uniform
    if (tid == 0) { s_key = 0ull; s_models = 0; }
    const double* px1 = px1_all + 2 * (size_t)first;
    const double* px2 = px2_all + 2 * (size_t)first;
    double T[9];
    const bool has = hg_solve_hypothesis(px1, px2, n, seed, min(h, H - 1), T);      // the spare lanes solve the last hypothesis again
    const double h0 = T[0], h1 = T[1], h2 = T[2], h3 = T[3], h4 = T[4], h5 = T[5], h6 = T[6], h7 = T[7], h8 = T[8];
    int count = 0;
    for (int base = 0; base < n; base += HG_CHUNK) {
        const int m = min(HG_CHUNK, n - base);
        __syncthreads();                                // the chunk before is consumed (and the first time: s_key is set)
        for (int i = tid; i < m; i += HG_THREADS) {
            const double* p = px1 + 2 * (size_t)(base + i);
            const double* q = px2 + 2 * (size_t)(base + i);
            s_pt[4 * i] = p[0]; s_pt[4 * i + 1] = p[1]; s_pt[4 * i + 2] = q[0]; s_pt[4 * i + 3] = q[1];
        }
        __syncthreads();
        for (int i = 0; i < m; i++) {                   // no model: H = 0, w = 0, never an inlier
            const double x = s_pt[4 * i], y = s_pt[4 * i + 1], u = s_pt[4 * i + 2], v = s_pt[4 * i + 3];
            const double w = (h6 * x + h7 * y) + h8;
            const double du = ((h0 * x + h1 * y) + h2) / w - u;
            const double dv = ((h3 * x + h4 * y) + h5) / w - v;
            count += ((w > 0.0) & ((du * du + dv * dv) < thr2)) ? 1 : 0;
        }
    }
    if (h < H && has) {
        atomicMax(&s_key, geo_key2(count, h));
        atomicAdd(&s_models, 1);
    }
    __syncthreads();
    if (tid == 0) {
        if (s_key) atomicMax(&keys[b], s_key);          // integer maxima and sums: the order of arrival does not matter
        if (s_models) atomicAdd(&models[b], s_models);
    }
}

// grid B: the winner of pair b solved again (every lane the same hypothesis), its matrix, mask and stats written
__global__ __launch_bounds__(HG_LANES) void hg_ransac_result_kernel(const int* __restrict__ offsets, int M, const double* __restrict__ px1_all,
                                                                    const double* __restrict__ px2_all, double thr2, uint64_t seed,
                                                                    const unsigned long long* __restrict__ keys,
                                                                    const int* __restrict__ models, double* __restrict__ H_out,
                                                                    uint8_t* __restrict__ inlier, int* __restrict__ stats,
                                                                    unsigned int* __restrict__ index_errors) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int first, last; bool bad;
    geo_range(offsets, b, M, &first, &last, &bad);
    if (bad && lane == 0) atomicAdd(index_errors, 1u);
    const int n = last - first;
    const unsigned long long key = n >= 4 ? keys[b] : 0ull;
    if (!key) {
        if (lane < 9) H_out[9 * b + lane] = 0.0;
        for (int i = lane; i < n; i += HG_LANES) inlier[first + i] = 0;
        if (lane == 0) { stats[4 * b] = 0; stats[4 * b + 1] = -1; stats[4 * b + 2] = -1; stats[4 * b + 3] = n >= 4 ? models[b] : 0; }
        return;
    }
    const int count = geo_key_count(key), h = geo_key2_h(key);
    const double* px1 = px1_all + 2 * (size_t)first;
    const double* px2 = px2_all + 2 * (size_t)first;
    double T[9];
    hg_solve_hypothesis(px1, px2, n, seed, h, T);
    for (int i = lane; i < n; i += HG_LANES)
        inlier[first + i] = hg_inlier(T, px1[2 * (size_t)i], px1[2 * (size_t)i + 1], px2[2 * (size_t)i], px2[2 * (size_t)i + 1], thr2) ? 1 : 0;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 9; i++) H_out[9 * b + i] = T[i];
        stats[4 * b] = count; stats[4 * b + 1] = h; stats[4 * b + 2] = 0; stats[4 * b + 3] = models[b];
    }
}

// grid B, one block per pair: every thread decomposes the pair's H (the same arithmetic in every lane, so every branch on
// its outcome is block-uniform), the matches are shared out for the two votes
__global__ __launch_bounds__(HG_THREADS) void hg_decompose_kernel(const int* __restrict__ offsets, int M, const double* __restrict__ px1,
                                                                  const double* __restrict__ px2, geo_cam cam, const double* __restrict__ H_all,
                                                                  const uint8_t* __restrict__ inlier_in, double dist,
                                                                  double* __restrict__ pose_all, double* __restrict__ normal_all,
                                                                  int* __restrict__ count_all, double* __restrict__ pose,
                                                                  double* __restrict__ sv_out, uint8_t* __restrict__ inlier_out,
                                                                  int* __restrict__ stats, unsigned int* __restrict__ index_errors) {
    __shared__ int s_sign[2];
    __shared__ int s_count[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    int first, last; bool bad;
    geo_range(offsets, b, M, &first, &last, &bad);
    if (bad && tid == 0) atomicAdd(index_errors, 1u);
    const int n = last - first;
    double H[9], Hn[9], sv[3], v1[3], v3[3];
#pragma unroll
    for (int t = 0; t < 9; t++) H[t] = H_all[9 * b + t];
    const bool ok = hg_singular(H, cam, Hn, sv, v1, v3);
    if (tid < 3) sv_out[3 * b + tid] = sv[tid];
    for (int i = tid; i < 48; i += HG_THREADS) pose_all[48 * b + i] = 0.0;
    if (tid < 12) normal_all[12 * b + tid] = 0.0;
    if (tid < 4) count_all[4 * b + tid] = 0;
    for (int i = tid; i < n; i += HG_THREADS) inlier_out[first + i] = 0;
    if (!ok) {                                          // no model: identity, no candidates
        if (tid < 12) pose[12 * b + tid] = (tid % 5 == 0) ? 1.0 : 0.0;
        if (tid == 0) { stats[4 * b] = 0; stats[4 * b + 1] = -1; stats[4 * b + 2] = 0; stats[4 * b + 3] = 0; }
        return;
    }
    if (tid < 2) s_sign[tid] = 0;
    if (tid < 4) s_count[tid] = 0;
    __syncthreads();
    double Hs[9];
#pragma unroll
    for (int t = 0; t < 9; t++) Hs[t] = Hn[t] / sv[1];
    int pos = 0, neg = 0;
    for (int i = tid; i < n; i += HG_THREADS) {
        if (inlier_in && !inlier_in[first + i]) continue;
        const double a = (px1[2 * (size_t)(first + i)] - cam.cx) / cam.fx, bb = (px1[2 * (size_t)(first + i) + 1] - cam.cy) / cam.fy;
        const double c = (px2[2 * (size_t)(first + i)] - cam.cx) / cam.fx, d = (px2[2 * (size_t)(first + i) + 1] - cam.cy) / cam.fy;
        const double r = hg_bilinear(Hs, a, bb, c, d);
        pos += r > 0.0 ? 1 : 0;
        neg += r < 0.0 ? 1 : 0;
    }
    if (pos) atomicAdd(&s_sign[0], pos);
    if (neg) atomicAdd(&s_sign[1], neg);
    __syncthreads();
    if (s_sign[1] > s_sign[0]) {
#pragma unroll
        for (int t = 0; t < 9; t++) Hs[t] = -Hs[t];
    }
    if ((sv[0] - sv[2]) / sv[1] < HG_ROTATION_ONLY) {   // a rotation: one candidate, no translation, no vote
        double R[9];
        hg_nearest_rotation(Hs, v1, v3, R);
        if (tid < 12) {
            const double e = (tid & 3) == 3 ? 0.0 : R[3 * (tid >> 2) + (tid & 3)];
            pose[12 * b + tid] = e;
            pose_all[48 * b + tid] = e;
        }
        if (tid == 0) { stats[4 * b] = 0; stats[4 * b + 1] = -2; stats[4 * b + 2] = 0; stats[4 * b + 3] = 1; }
        return;
    }
    double P[48], Nn[12];
    hg_candidates(Hs, sv[0] / sv[1], sv[2] / sv[1], v1, v3, P, Nn);
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    for (int i = tid; i < n; i += HG_THREADS) {
        if (inlier_in && !inlier_in[first + i]) continue;
        const double a = (px1[2 * (size_t)(first + i)] - cam.cx) / cam.fx, bb = (px1[2 * (size_t)(first + i) + 1] - cam.cy) / cam.fy;
        const double c = (px2[2 * (size_t)(first + i)] - cam.cx) / cam.fx, d = (px2[2 * (size_t)(first + i) + 1] - cam.cy) / cam.fy;
        c0 += geo_cheirality(P, a, bb, c, d, dist) ? 1 : 0;
        c1 += geo_cheirality(P + 12, a, bb, c, d, dist) ? 1 : 0;
        c2 += geo_cheirality(P + 24, a, bb, c, d, dist) ? 1 : 0;
        c3 += geo_cheirality(P + 36, a, bb, c, d, dist) ? 1 : 0;
    }
    if (c0) atomicAdd(&s_count[0], c0);
    if (c1) atomicAdd(&s_count[1], c1);
    if (c2) atomicAdd(&s_count[2], c2);
    if (c3) atomicAdd(&s_count[3], c3);
    __syncthreads();
    int win = 0;
#pragma unroll
    for (int k = 1; k < 4; k++)
        if (s_count[k] > s_count[win]) win = k;
    int second = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (k != win && s_count[k] > second) second = s_count[k];
    double W[12];
#pragma unroll
    for (int i = 0; i < 12; i++) W[i] = win == 0 ? P[i] : win == 1 ? P[12 + i] : win == 2 ? P[24 + i] : P[36 + i];
    for (int i = tid; i < n; i += HG_THREADS) {
        if (inlier_in && !inlier_in[first + i]) continue;
        const double a = (px1[2 * (size_t)(first + i)] - cam.cx) / cam.fx, bb = (px1[2 * (size_t)(first + i) + 1] - cam.cy) / cam.fy;
        const double c = (px2[2 * (size_t)(first + i)] - cam.cx) / cam.fx, d = (px2[2 * (size_t)(first + i) + 1] - cam.cy) / cam.fy;
        inlier_out[first + i] = geo_cheirality(W, a, bb, c, d, dist) ? 1 : 0;
    }
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 48; i++) pose_all[48 * b + i] = P[i];
#pragma unroll
        for (int i = 0; i < 12; i++) { normal_all[12 * b + i] = Nn[i]; pose[12 * b + i] = W[i]; }
#pragma unroll
        for (int k = 0; k < 4; k++) count_all[4 * b + k] = s_count[k];
        stats[4 * b] = s_count[win]; stats[4 * b + 1] = win; stats[4 * b + 2] = second; stats[4 * b + 3] = 4;
    }
}

// grid B, one block per pair: the matches shared out, the terms summed as 64-bit integers (exact whatever the order)
__global__ __launch_bounds__(HG_THREADS) void hg_score_kernel(const int* __restrict__ offsets, int M, const double* __restrict__ px1,
                                                              const double* __restrict__ px2, geo_cam cam, const double* __restrict__ H_all,
                                                              const double* __restrict__ E_all, double sigma2, long long* __restrict__ score,
                                                              double* __restrict__ ratio, unsigned int* __restrict__ index_errors) {
    __shared__ unsigned long long s_sum[2];
    const int b = blockIdx.x, tid = threadIdx.x;
    int first, last; bool bad;
    geo_range(offsets, b, M, &first, &last, &bad);
    if (bad && tid == 0) atomicAdd(index_errors, 1u);
    const int n = last - first;
    if (tid < 2) s_sum[tid] = 0ull;
    __syncthreads();
    double H[9], Hi[9], E[9], F[9];
#pragma unroll
    for (int t = 0; t < 9; t++) { H[t] = H_all[9 * b + t]; E[t] = E_all[9 * b + t]; }
    hg_adjugate(H, Hi);
    hg_fundamental(E, cam, F);
    long long sh = 0, se = 0;
    for (int i = tid; i < n; i += HG_THREADS)
        hg_score_match(H, Hi, F, px1[2 * (size_t)(first + i)], px1[2 * (size_t)(first + i) + 1], px2[2 * (size_t)(first + i)],
                       px2[2 * (size_t)(first + i) + 1], sigma2, &sh, &se);
    if (sh) atomicAdd(&s_sum[0], (unsigned long long)sh);
    if (se) atomicAdd(&s_sum[1], (unsigned long long)se);
    __syncthreads();
    if (tid == 0) {
        const long long th = (long long)s_sum[0], te = (long long)s_sum[1];
        score[2 * b] = th; score[2 * b + 1] = te;
        ratio[b] = hg_ratio(th, te);
    }
}

// =============================================================== entry points ================================================
#include "geometry_host.h"           // the checks, the vote block and the launch shapes the four estimators' entry points share

extern "C" int slam_hg_fourpoint_f64(slam_ctx* ctx, int64_t S, const double* d_p1, const double* d_p2, double* d_H, int32_t* d_ok) {
    GEO_SAMPLE_SIZES(ctx, S);
    GEO_POINTERS(S, d_p1 && d_p2 && d_H && d_ok);
    SLAM_HIP(hipSetDevice(ctx->device));
    hg_fourpoint_kernel<<<geo_blocks(S, HG_LANES), HG_LANES, 0, ctx->stream>>>((int)S, d_p1, d_p2, d_H, d_ok);
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

extern "C" int slam_hg_ransac_f64(slam_ctx* ctx, int64_t B, const int32_t* d_offsets, const double* d_px1, const double* d_px2, int64_t M,
                                  int H, double threshold_px, uint64_t seed, double* d_H, uint8_t* d_inlier, int32_t* d_stats) {
    GEO_RANSAC_SIZES(ctx, B, M, H);
    SLAM_REQUIRE(threshold_px > 0.0, "threshold must be positive");
    GEO_POINTERS(B, d_offsets && d_H && d_stats && (M == 0 || (d_px1 && d_px2 && d_inlier)));
    SLAM_HIP(hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> lk(ctx->call_mu);        // the workspace holds the keys and the model counts
    void* ws = nullptr;
    if (int rc = slam_workspace(ctx, geo_vote_bytes(0, B), &ws)) return rc;
    unsigned long long* keys; int* models;
    if (int rc = geo_vote_block(ctx, ws, 0, B, true, M, d_inlier, &keys, &models)) return rc;
    const double thr2 = threshold_px * threshold_px;
    hg_ransac_kernel<<<geo_vote_grid(H, HG_THREADS, B), HG_THREADS, 0, ctx->stream>>>(d_offsets, (int)M, d_px1, d_px2, H, thr2, seed, keys, models);
    SLAM_HIP(hipGetLastError());
    hg_ransac_result_kernel<<<(unsigned)B, HG_LANES, 0, ctx->stream>>>(d_offsets, (int)M, d_px1, d_px2, thr2, seed, keys, models, d_H, d_inlier,
                                                                      d_stats, slam_index_error_counter(ctx));
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

extern "C" int slam_hg_decompose_f64(slam_ctx* ctx, int64_t B, const int32_t* d_offsets, const double* d_px1, const double* d_px2, int64_t M,
                                     double fx, double fy, double cx, double cy, const double* d_H, const uint8_t* d_inlier_in,
                                     double distance_thresh, double* d_pose_all, double* d_normal_all, int32_t* d_count, double* d_pose,
                                     double* d_sv, uint8_t* d_inlier_out, int32_t* d_stats) {
    GEO_CANDIDATE_SIZES(ctx, B, 1 << 20, M);
    SLAM_REQUIRE(fx > 0.0 && fy > 0.0 && distance_thresh > 0.0, "focal lengths and distance_thresh must be positive");
    GEO_POINTERS(B, d_offsets && d_H && d_pose_all && d_normal_all && d_count && d_pose && d_sv && d_stats &&
                        (M == 0 || (d_px1 && d_px2 && d_inlier_out)));
    SLAM_HIP(hipSetDevice(ctx->device));
    const geo_cam cam = {fx, fy, cx, cy};
    if (M > 0) SLAM_HIP(hipMemsetAsync(d_inlier_out, 0, (size_t)M, ctx->stream));
    hg_decompose_kernel<<<(unsigned)B, HG_THREADS, 0, ctx->stream>>>(d_offsets, (int)M, d_px1, d_px2, cam, d_H, d_inlier_in, distance_thresh,
                                                                    d_pose_all, d_normal_all, d_count, d_pose, d_sv, d_inlier_out, d_stats,
                                                                    slam_index_error_counter(ctx));
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

extern "C" int slam_hg_model_score_f64(slam_ctx* ctx, int64_t B, const int32_t* d_offsets, const double* d_px1, const double* d_px2, int64_t M,
                                       double fx, double fy, double cx, double cy, const double* d_H, const double* d_E, double sigma,
                                       int64_t* d_score, double* d_ratio) {
    GEO_CANDIDATE_SIZES(ctx, B, 1 << 20, M);
    SLAM_REQUIRE(fx > 0.0 && fy > 0.0 && sigma > 0.0 && sigma * sigma > 0.0 && sigma * sigma < GEO_BIG,
                 "focal lengths and sigma must be positive (sigma^2 a positive finite double)");
    GEO_POINTERS(B, d_offsets && d_H && d_E && d_score && d_ratio && (M == 0 || (d_px1 && d_px2)));
    SLAM_HIP(hipSetDevice(ctx->device));
    const geo_cam cam = {fx, fy, cx, cy};
    hg_score_kernel<<<(unsigned)B, HG_THREADS, 0, ctx->stream>>>(d_offsets, (int)M, d_px1, d_px2, cam, d_H, d_E, sigma * sigma,
                                                                (long long*)d_score, d_ratio, slam_index_error_counter(ctx));
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}
#endif  // HG_HOST_ONLY
