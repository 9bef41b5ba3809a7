// stereo_edge.h - the edge model of the stereo / level-weighted adjustments (ORB-SLAM's EdgeSE3ProjectXYZ,
// EdgeStereoSE3ProjectXYZ and their OnlyPose forms): one observation of a point under a pose as two (monocular) or three
// (stereo) residuals with a scalar information, the Huber kernel on the weighted chi2, the Jacobians, and the inlier rule.
// The same text runs in the kernels of ba_stereo.hip and pose_stereo.hip and on the host (tests/stereo_edge_twin.cpp builds it
// with a plain C++ compiler).  It carries NO contraction pragma of its own and uses only + - * / sqrt, no fma(): every file
// that includes it does so behind `#pragma clang fp contract(off)` (the host build: -ffp-contract=off), so both builds round
// every operation once, in the order written, and return the same bits.
//
// Rows 0 and 1 are ba_linearise of ba_common.h operation for operation: with mr NaN, s = 1 and delta_mono = huber_delta
// an edge here has the e, w, rho and Jacobian rows of that function, bit for bit (the parent rule of ba_stereo.hip).
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define SE_HD __host__ __device__ __forceinline__
#else
#define SE_HD inline
#endif

struct se_cam { double fx, fy, cx, cy, bf; };

struct se_gate { double chi2_mono, chi2_stereo; };      // inlier bounds on the weighted chi2, by kind
struct se_huber { double delta_mono, delta_stereo; };   // Huber widths on sqrt(weighted chi2), by kind; <= 0: no kernel

// the information of an edge as the sums take it: the inverse variance, or 0 for a value that is none (negative, NaN, inf)
SE_HD bool se_info_ok(double s) { return s >= 0.0 && s <= 1.7976931348623157e308; }
SE_HD double se_info(double s) { return se_info_ok(s) ? s : 0.0; }

// residuals, weighted chi2, Huber weight and cost of one edge; e[2] = 0 for a monocular edge (mr NaN)
struct se_res {
    double X, Y, Z, e[3], s, chi2, w, rho;
    int stereo;
};

SE_HD void se_residual(const double* P, const double* p, double mu, double mv, double mr, double info, const se_cam& cam,
                       const se_huber& hub, se_res& r) {
    r.X = P[0] * p[0] + P[1] * p[1] + P[2] * p[2] + P[3];
    r.Y = P[4] * p[0] + P[5] * p[1] + P[6] * p[2] + P[7];
    r.Z = P[8] * p[0] + P[9] * p[1] + P[10] * p[2] + P[11];
    const double u = (cam.fx * r.X + cam.cx * r.Z) / r.Z;
    const double v = (cam.fy * r.Y + cam.cy * r.Z) / r.Z;
    r.e[0] = mu - u;
    r.e[1] = mv - v;
    r.stereo = mr == mr ? 1 : 0;
    double c2 = r.e[0] * r.e[0] + r.e[1] * r.e[1];
    r.e[2] = 0.0;
    if (r.stereo) {
        r.e[2] = mr - (u - cam.bf / r.Z);
        c2 = c2 + r.e[2] * r.e[2];
    }
    r.s = se_info(info);
    r.chi2 = r.s * c2;
    const double delta = r.stereo ? hub.delta_stereo : hub.delta_mono;
    r.w = 1.0;
    r.rho = r.chi2;
    if (delta > 0.0) {
        const double en = sqrt(r.chi2);
        if (en > delta) {
            r.w = delta / en;
            r.rho = 2.0 * delta * en - delta * delta;
        }
    }
}

// the 3x6 pose Jacobian (rotation first, update T <- Exp([w, v]) T) and the 3x3 point Jacobian at the camera-frame point of r;
// row 2 is zero for a monocular edge
struct se_jac { double jp[3][6], jq[3][3]; };

SE_HD void se_jacobians(const double* P, const se_res& r, const se_cam& cam, se_jac& j) {
    const double X = r.X, Y = r.Y, Z = r.Z;
    const double Zinv = 1.0 / (Z + 1e-18), Zinv2 = Zinv * Zinv;
    j.jp[0][0] = cam.fx * X * Y * Zinv2; j.jp[0][1] = -cam.fx - cam.fx * X * X * Zinv2; j.jp[0][2] = cam.fx * Y * Zinv;
    j.jp[0][3] = -cam.fx * Zinv; j.jp[0][4] = 0.0; j.jp[0][5] = cam.fx * X * Zinv2;
    j.jp[1][0] = cam.fy + cam.fy * Y * Y * Zinv2; j.jp[1][1] = -cam.fy * X * Y * Zinv2; j.jp[1][2] = -cam.fy * X * Zinv;
    j.jp[1][3] = 0.0; j.jp[1][4] = -cam.fy * Zinv; j.jp[1][5] = cam.fy * Y * Zinv2;
    const double A[2][3] = {{cam.fx * Zinv, 0.0, -cam.fx * X * Zinv2}, {0.0, cam.fy * Zinv, -cam.fy * Y * Zinv2}};
    for (int c = 0; c < 3; c++) {
        j.jq[0][c] = -(A[0][0] * P[c] + A[0][2] * P[8 + c]);
        j.jq[1][c] = -(A[1][1] * P[4 + c] + A[1][2] * P[8 + c]);
    }
    if (r.stereo) {
        const double g = cam.bf * Zinv2;                 // d(bf / Z) = -g dZ, dZ = (Y, -X, 0, 0, 0, 1) . [w, v]
        j.jp[2][0] = j.jp[0][0] - g * Y; j.jp[2][1] = j.jp[0][1] + g * X; j.jp[2][2] = j.jp[0][2];
        j.jp[2][3] = j.jp[0][3]; j.jp[2][4] = j.jp[0][4]; j.jp[2][5] = j.jp[0][5] - g;
        for (int c = 0; c < 3; c++) j.jq[2][c] = j.jq[0][c] - g * P[8 + c];
    } else {
        for (int a = 0; a < 6; a++) j.jp[2][a] = 0.0;
        for (int c = 0; c < 3; c++) j.jq[2][c] = 0.0;
    }
}

// the one classification of both optimisers: information, positive depth (ORB-SLAM's isDepthPositive) and the gate of the kind
SE_HD bool se_inlier(const se_res& r, const se_gate& gate) {
    return r.s > 0.0 && r.Z > 0.0 && r.chi2 <= (r.stereo ? gate.chi2_stereo : gate.chi2_mono);
}
