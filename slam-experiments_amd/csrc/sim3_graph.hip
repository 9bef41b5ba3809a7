// sim3_graph.hip — Sim(3) pose-graph optimisation on gfx950: ORB-SLAM's OptimizeEssentialGraph (7-DoF loop closing) for this
// project's conventions, the consumer of slam_sim3_* models.  A new file beside pose_graph.hip (section 4c of DESIGN.md) with
// PRIVATE COPIES of what it needs from there: that file is specialised to 6x6 blocks throughout and stays as it is.
//
//   slam_s3g_linearize_f64   residual, Jacobians, robust weight per edge; diagonal blocks and gradient per vertex
//   slam_s3g_hmul_f64        y = (H + lambda I) x over the free vertices: the block-sparse 7x7 product (the hot path)
//   slam_s3g_pcg_f64         conjugate gradients on (H + lambda I) x = -b, preconditioner (H_vv + lambda I)^-1
//   slam_s3g_optimize_f64    the LM loop (g2o's schedule, as pose_graph.hip), slam_s3g_optimize_host_f64 on host buffers
//
// Conventions (include/slamhip.h has them in full).  A vertex is S = (s, R, t), X_cam = s R X_world + t, stored [13]: the
// row-major 3x4 [R|t], then s (the model layout of sim3.hip).  (s_a,R_a,t_a) o (s_b,R_b,t_b) = (s_a s_b, R_a R_b,
// s_a R_a t_b + t_a); inverse (1/s, R^T, -R^T t / s).  Tangent d = [w, v, sigma], rotation first, scale last.  Chart
// Phi(d) = Exp_SE3(w, v) o Scale(e^sigma) = (e^sigma, Exp(w), V(w) v); update S <- Phi(d) o S.  Edge (i, j) carries
// Z ~ S_j S_i^-1, D = S_j S_i^-1 Z^-1, r = Phi^-1(D) = [Log_SE3(R_D, t_D), log s_D], F = sum rho(r^T Omega r).
//   J_j = dr/dd_j = [[Jl^-1, Jl^-1 (0; t_D)], [0, 1]]      Jl^-1 the SE(3) inverse left Jacobian at r_1..6
//   J_i = dr/dd_i = -J_j Ad(A), A = S_j S_i^-1 = (s, R, t),  Ad(A) = [[R, 0, 0], [t^ R, s R, -t], [0, 0, 1]]
// fix_scale zeroes column 7 of both Jacobians: b_sigma = 0, H_sigma,sigma = lambda, every d_sigma = 0, every s bit for bit.
// This chart is the exact inverse of the retraction and reuses the SE(3) logarithm; it differs from g2o's Sim3::log at
// second order in sigma * v.  PARITY UNPINNED against g2o / ORB-SLAM (absent here).
//
// Guarantees, as pose_graph.hip: f64 with floating-point contraction OFF; no floating-point atomic; an edge writes into the
// SLOTS of its two ends (slot = position in the vertex -> edge list), a vertex adds its slots in list order; sums over the
// graph go through at most S3G_MAX_PART + S3G_HUB_BLOCKS per-block partials that every block of the next kernel adds again
// in the same order, so the CG scalars and the stop decision never leave the device (the done flag is read every
// S3G_CG_CHECK iterations).  A result is a pure function of the inputs.  Plain C++ and vector stores only.
//
// Storage per slot k of vertex v (adj[k] = 2 e + side):
//   S[k]   49 doubles   the block that multiplies x of the OTHER end: w J_i^T Omega J_j for side 0, its transpose for side 1
//   D[k]   35 doubles   this end's share of H_vv (28, upper triangle by rows) and of b_v (7)
//   nbr[k] int32        the other end's vertex, or -1 when that vertex is fixed
// Lane mapping of the product and of the CG vector kernels: SEVEN lanes per vertex, lane (v, row) owns row `row` of every
// block of v; a wave holds 9 vertices (63 of 64 lanes), a block 36.  Vertices above S3G_HUB_DEG slots take a wave each: nine
// slot groups, the nine partial rows added in group order through LDS; hub h goes to wave h mod 64 of 16 hub blocks.
// A 7x7 row is 56 bytes, so alternate rows are not 16-byte aligned: rows are read with 8-byte loads from PACKED 49-double
// slots.  The padded alternative (7x8 slots, 64-byte rows read as four 16-byte loads, 14 % more bytes) was built behind a
// compile-time switch, measured 6 % slower per CG iteration on the 10^5-vertex scene and deleted.
//
// The edge kernel: the SE(3) one already sits at 256 VGPR + 74 AGPR.  Here the three 7x7 products are ordered so that at most
// three 49-double matrices are live (J_j, J_i and one Omega J): W_e and the j share from Omega J_j first, then Omega J_i
// for the i share.  Registers and scratch per kernel: profiles/sim3_graph_resources.txt.
#ifndef S3G_HOST_ONLY                // a host build of the per-edge routines alone (the test suite's twin) defines it
#include "internal.h"
#endif
#include <math.h>
#include <stdint.h>

#pragma clang fp contract(off)

#ifdef S3G_HOST_ONLY
#define S3G_HD inline
#else
#define S3G_HD __device__ __forceinline__
#endif
#define S3G_ST_INDEX 1                        // status bits (SLAM_S3G_STATUS_* of the header)
#define S3G_ST_ANGLE 2
#define S3G_ST_PRECOND 4
#define S3G_ST_BREAKDOWN 8
#define S3G_ST_NONFINITE 16
#define S3G_ST_SCALE 32

// ---- Sim(3) ----------------------------------------------------------------------------------------------------------------
// With every s = 1 these are pose_graph.hip's pg_inv / pg_mul operation for operation (x / 1 and 1 * x are exact).
S3G_HD void s3g_inv(const double* S, double* o) {
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) o[i * 4 + j] = S[j * 4 + i];
        o[i * 4 + 3] = -(S[i] * S[3] + S[4 + i] * S[7] + S[8 + i] * S[11]) / S[12];
    }
    o[12] = 1.0 / S[12];
}
S3G_HD void s3g_mul(const double* A, const double* B, double* o) {
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) o[i * 4 + j] = A[i * 4] * B[j] + A[i * 4 + 1] * B[4 + j] + A[i * 4 + 2] * B[8 + j];
        o[i * 4 + 3] = A[12] * (A[i * 4] * B[3] + A[i * 4 + 1] * B[7] + A[i * 4 + 2] * B[11]) + A[i * 4 + 3];
    }
    o[12] = A[12] * B[12];
}
S3G_HD bool s3g_scale_ok(double s) { return isfinite(s) && s > 0.0; }
S3G_HD void s3g_hat(const double* w, double* W) {
    W[0] = 0; W[1] = -w[2]; W[2] = w[1]; W[3] = w[2]; W[4] = 0; W[5] = -w[0]; W[6] = -w[1]; W[7] = w[0]; W[8] = 0;
}
S3G_HD void s3g_mm3(const double* A, const double* B, double* C) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}

// Phi(d) o S: s' = e^sigma s, R' = Exp(w) R, t' = e^sigma Exp(w) t + V(w) v; the series of pg_apply_update below 1e-4 rad
S3G_HD void s3g_apply_update(const double* dx, const double* S, double* Sn) {
    const double th2 = dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2], th = sqrt(th2);
    double a, b, c;  // sin(th)/th, (1-cos)/th^2, (th-sin)/th^3
    if (th < 1e-4) { a = 1.0 - th2 / 6.0; b = 0.5 - th2 / 24.0; c = 1.0 / 6.0 - th2 / 120.0; }
    else {
        const double sn = sin(th), cs = cos(th);
        a = sn / th; b = (1.0 - cs) / th2; c = (th - sn) / (th2 * th);
    }
    const double es = exp(dx[6]);
    double W[9], W2[9], R[9], V[9];
    s3g_hat(dx, W);
    s3g_mm3(W, W, W2);
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const double I = (i % 4 == 0) ? 1.0 : 0.0;
        R[i] = I + a * W[i] + b * W2[i];
        V[i] = I + b * W[i] + c * W2[i];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) Sn[i * 4 + j] = R[i * 3] * S[j] + R[i * 3 + 1] * S[4 + j] + R[i * 3 + 2] * S[8 + j];
        Sn[i * 4 + 3] = es * (R[i * 3] * S[3] + R[i * 3 + 1] * S[7] + R[i * 3 + 2] * S[11]) +
                        (V[i * 3] * dx[3] + V[i * 3 + 1] * dx[4] + V[i * 3 + 2] * dx[5]);
    }
    Sn[12] = es * S[12];
}

// the coefficients of Jl^-1 and Q at angle th: pg_coeffs (four-term series below 0.2 rad)
S3G_HD void s3g_coeffs(double th2, double th, double* k, double* c1, double* c2, double* c3) {
    if (th < 0.2) {
        *k = 1.0 / 12.0 + th2 * (1.0 / 720.0 + th2 * (1.0 / 30240.0 + th2 * (1.0 / 1209600.0)));
        *c1 = 1.0 / 6.0 - th2 * (1.0 / 120.0 - th2 * (1.0 / 5040.0 - th2 * (1.0 / 362880.0)));
        *c2 = 1.0 / 24.0 - th2 * (1.0 / 720.0 - th2 * (1.0 / 40320.0 - th2 * (1.0 / 3628800.0)));
        *c3 = 1.0 / 120.0 - th2 * (1.0 / 2520.0 - th2 * (1.0 / 120960.0 - th2 * (1.0 / 9979200.0)));
    } else {
        const double sn = sin(th), cs = cos(th), th4 = th2 * th2;
        *k = (1.0 - (th * sn) / (2.0 * (1.0 - cs))) / th2;
        *c1 = (th - sn) / (th2 * th);
        *c2 = (th2 + 2.0 * cs - 2.0) / (2.0 * th4);
        *c3 = (2.0 * th - 3.0 * sn + th * cs) / (2.0 * th4 * th);
    }
}

// pg_log_jinv on the [R|t] part of D: r[0..5] = Log_SE3 in [w, v], Jr = Jl^-1(r) (6x6 row-major).  False beyond 3.1 rad or
// when something is not finite; the outputs are finite zeros then.
S3G_HD bool s3g_log_jinv(const double* D, double* r, double* Jr, bool want_j) {
    const double s[3] = {0.5 * (D[9] - D[6]), 0.5 * (D[2] - D[8]), 0.5 * (D[4] - D[1])};
    const double cs = 0.5 * (D[0] + D[5] + D[10] - 1.0);
    const double sn2 = s[0] * s[0] + s[1] * s[1] + s[2] * s[2], sn = sqrt(sn2);
    double th = atan2(sn, cs);
    const bool ok = isfinite(th) && th <= 3.1 && isfinite(D[3]) && isfinite(D[7]) && isfinite(D[11]);
    if (!ok) th = 0.0;
    const double th2 = th * th;
    const double f = sn > 1e-4 ? th / sn : 1.0 + th2 * (1.0 / 6.0 + th2 * (7.0 / 360.0));   // th / sin(th)
    double k, c1, c2, c3;
    s3g_coeffs(th2, th, &k, &c1, &c2, &c3);
    double W[9], W2[9], Ji[9];
#pragma unroll
    for (int i = 0; i < 3; i++) r[i] = ok ? f * s[i] : 0.0;
    s3g_hat(r, W);
    s3g_mm3(W, W, W2);
#pragma unroll
    for (int i = 0; i < 9; i++) Ji[i] = ((i % 4 == 0) ? 1.0 : 0.0) - 0.5 * W[i] + k * W2[i];
    const double t[3] = {ok ? D[3] : 0.0, ok ? D[7] : 0.0, ok ? D[11] : 0.0};
#pragma unroll
    for (int i = 0; i < 3; i++) r[3 + i] = Ji[i * 3] * t[0] + Ji[i * 3 + 1] * t[1] + Ji[i * 3 + 2] * t[2];
    if (!want_j) return ok;
    // Q = P/2 + c1 (WP + PW + WPW) + c2 (W2 P + P W2 - 3 WPW) + c3 (WPW2 + W2PW), P = hat(v)  (Barfoot eq. 7.86)
    double P[9], WP[9], PW[9], WPW[9], W2P[9], PW2[9], WPW2[9], W2PW[9], Q[9], JQ[9], C[9];
    s3g_hat(r + 3, P);
    s3g_mm3(W, P, WP); s3g_mm3(P, W, PW); s3g_mm3(WP, W, WPW); s3g_mm3(W2, P, W2P); s3g_mm3(P, W2, PW2);
    s3g_mm3(WP, W2, WPW2); s3g_mm3(W2, PW, W2PW);
#pragma unroll
    for (int i = 0; i < 9; i++)
        Q[i] = 0.5 * P[i] + c1 * (WP[i] + PW[i] + WPW[i]) + c2 * (W2P[i] + PW2[i] - 3.0 * WPW[i]) + c3 * (WPW2[i] + W2PW[i]);
    s3g_mm3(Ji, Q, JQ);
    s3g_mm3(JQ, Ji, C);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            Jr[i * 6 + j] = Ji[i * 3 + j];
            Jr[i * 6 + 3 + j] = 0.0;
            Jr[(3 + i) * 6 + j] = -C[i * 3 + j];
            Jr[(3 + i) * 6 + 3 + j] = Ji[i * 3 + j];
        }
    return ok;
}

// Ad((s, R, t)) = [[R, 0, 0], [t^ R, s R, -t], [0, 0, 1]] (7x7 row-major)
S3G_HD void s3g_adjoint(const double* A, double* Ad) {
    const double t[3] = {A[3], A[7], A[11]};
    double R[9], Th[9], TR[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) R[i * 3 + j] = A[i * 4 + j];
    s3g_hat(t, Th);
    s3g_mm3(Th, R, TR);
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            Ad[i * 7 + j] = R[i * 3 + j];
            Ad[i * 7 + 3 + j] = 0.0;
            Ad[(3 + i) * 7 + j] = TR[i * 3 + j];
            Ad[(3 + i) * 7 + 3 + j] = A[12] * R[i * 3 + j];
        }
        Ad[i * 7 + 6] = 0.0;
        Ad[(3 + i) * 7 + 6] = -t[i];
    }
#pragma unroll
    for (int j = 0; j < 6; j++) Ad[42 + j] = 0.0;
    Ad[48] = 1.0;
}

// 7x7 helpers (row-major): C = A B, (A^T B)[i][j]
S3G_HD void s3g_mm7(const double* A, const double* B, double* C) {
#pragma unroll
    for (int i = 0; i < 7; i++)
#pragma unroll
        for (int j = 0; j < 7; j++) {
            double v = A[i * 7] * B[j];
#pragma unroll
            for (int k = 1; k < 7; k++) v += A[i * 7 + k] * B[k * 7 + j];
            C[i * 7 + j] = v;
        }
}
S3G_HD double s3g_atb(const double* A, const double* B, int i, int j) {
    double v = A[i] * B[j];
#pragma unroll
    for (int k = 1; k < 7; k++) v += A[k * 7 + i] * B[k * 7 + j];
    return v;
}

// inverse of the SPD 7x7 A (full storage) by LDL^T, as pg_inverse6; false (and the identity) if not SPD
S3G_HD bool s3g_inverse7(const double* A, double* Inv) {
    double L[49], d[7], dinv[7];
    bool spd = true;
#pragma unroll
    for (int j = 0; j < 7; j++) {
        double v = A[j * 7 + j];
#pragma unroll
        for (int k = 0; k < j; k++) v -= L[j * 7 + k] * L[j * 7 + k] * d[k];
        spd = spd && (v > 0.0) && isfinite(v);
        d[j] = v;
        dinv[j] = 1.0 / v;
#pragma unroll
        for (int i = j + 1; i < 7; i++) {
            double u = A[i * 7 + j];
#pragma unroll
            for (int k = 0; k < j; k++) u -= L[i * 7 + k] * L[j * 7 + k] * d[k];
            L[i * 7 + j] = u * dinv[j];
        }
    }
#pragma unroll
    for (int c = 0; c < 7; c++) {          // column c of the inverse; the lower triangle is mirrored from the upper one
        double y[7], x[7];
#pragma unroll
        for (int i = 0; i < 7; i++) {
            double v = (i == c) ? 1.0 : 0.0;
#pragma unroll
            for (int k = 0; k < i; k++) v -= L[i * 7 + k] * y[k];
            y[i] = v;
        }
#pragma unroll
        for (int i = 6; i >= 0; i--) {
            double v = y[i] * dinv[i];
#pragma unroll
            for (int k = i + 1; k < 7; k++) v -= L[k * 7 + i] * x[k];
            x[i] = v;
        }
#pragma unroll
        for (int i = 0; i < 7; i++)
            if (i <= c) { Inv[i * 7 + c] = spd ? x[i] : (i == c ? 1.0 : 0.0); Inv[c * 7 + i] = Inv[i * 7 + c]; }
    }
    return spd;
}

// One edge.  Returns 0 for a live edge, else the status bit of the reason it left the sums (its cost is 0 and its blocks are
// finite zeros then, by a select: 0 * inf is NaN and one NaN block would reach every CG scalar).  FULL: W_e = w J_i^T Omega J_j
// into Wi [49] and its transpose into Wj [49], optionally into We [49]; Di / Dj [35] = each end's share of H_vv (28, upper
// triangle by rows) and of b (7).  !FULL: the robust cost only.
template <bool FULL>
S3G_HD int s3g_edge(const double* Si, const double* Sj, const double* Z, const double* Om, double huber, bool fix_scale, double* rho_out,
                    double* Wi, double* Wj, double* We, double* Di, double* Dj) {
    double Iv[13], A[13], D[13];
    s3g_inv(Si, Iv);
    s3g_mul(Sj, Iv, A);
    s3g_inv(Z, Iv);
    s3g_mul(A, Iv, D);
    const bool sok = s3g_scale_ok(Si[12]) && s3g_scale_ok(Sj[12]) && s3g_scale_ok(Z[12]) && s3g_scale_ok(D[12]);
    double r[7], Jr[36];
    const bool aok = s3g_log_jinv(D, r, Jr, FULL);
    r[6] = sok ? log(D[12]) : 0.0;
    double Or[7];
#pragma unroll
    for (int a = 0; a < 7; a++) {
        double v = Om[a * 7] * r[0];
#pragma unroll
        for (int b = 1; b < 7; b++) v += Om[a * 7 + b] * r[b];
        Or[a] = v;
    }
    double chi2 = r[0] * Or[0];
#pragma unroll
    for (int a = 1; a < 7; a++) chi2 += r[a] * Or[a];
    double w = 1.0, rho = chi2;
    if (huber > 0.0) {                               // rho' and rho of g2o's RobustKernelHuber, as pose_graph.hip
        const double en = sqrt(chi2);
        if (en > huber) { w = huber / en; rho = 2.0 * huber * en - huber * huber; }
    }
    const bool live = sok && aok && isfinite(rho);
    const int why = live ? 0 : !sok ? S3G_ST_SCALE : !aok ? S3G_ST_ANGLE : S3G_ST_NONFINITE;
    if (!live) { rho = 0.0; w = 0.0; }
    *rho_out = rho;
    if (FULL) {
        // J_j: Jl^-1 in the 6x6 corner; column 7 = Jl^-1 (0; t_D), whose upper half is 0 and whose lower half Jso3^-1 t_D is
        // the translation part of r, operation for operation; row 7 = [0 .. 0, 1].  fix_scale zeroes column 7.
        double Jj[49], Ji[49];
#pragma unroll
        for (int a = 0; a < 6; a++) {
#pragma unroll
            for (int b = 0; b < 6; b++) Jj[a * 7 + b] = Jr[a * 6 + b];
            Jj[a * 7 + 6] = (a < 3 || fix_scale) ? 0.0 : r[a];
            Jj[42 + a] = 0.0;
        }
        Jj[48] = fix_scale ? 0.0 : 1.0;
        {
            double Ad[49];
            s3g_adjoint(A, Ad);
            s3g_mm7(Jj, Ad, Ji);
        }
#pragma unroll
        for (int q = 0; q < 49; q++) Ji[q] = (fix_scale && q % 7 == 6) ? 0.0 : -Ji[q];
        {
            double OJ[49];
            s3g_mm7(Om, Jj, OJ);
#pragma unroll
            for (int a = 0; a < 7; a++)
#pragma unroll
                for (int b = 0; b < 7; b++) {
                    const double v = live ? w * s3g_atb(Ji, OJ, a, b) : 0.0;       // W_e = w J_i^T Omega J_j
                    Wi[a * 7 + b] = v;
                    Wj[b * 7 + a] = v;
                    if (We) We[a * 7 + b] = v;
                }
            int t = 0;
#pragma unroll
            for (int a = 0; a < 7; a++)
#pragma unroll
                for (int b = a; b < 7; b++) Dj[t++] = live ? w * s3g_atb(Jj, OJ, a, b) : 0.0;
#pragma unroll
            for (int a = 0; a < 7; a++) {
                double g = Jj[a] * Or[0];
#pragma unroll
                for (int k = 1; k < 7; k++) g += Jj[k * 7 + a] * Or[k];
                Dj[28 + a] = live ? w * g : 0.0;
            }
        }
        {
            double OJ[49];
            s3g_mm7(Om, Ji, OJ);
            int t = 0;
#pragma unroll
            for (int a = 0; a < 7; a++)
#pragma unroll
                for (int b = a; b < 7; b++) Di[t++] = live ? w * s3g_atb(Ji, OJ, a, b) : 0.0;
#pragma unroll
            for (int a = 0; a < 7; a++) {
                double g = Ji[a] * Or[0];
#pragma unroll
                for (int k = 1; k < 7; k++) g += Ji[k * 7 + a] * Or[k];
                Di[28 + a] = live ? w * g : 0.0;
            }
        }
    }
    return why;
}

#ifndef S3G_HOST_ONLY
// =============================================================== kernels =====================================================
#define S3G_THREADS 256                         // vector kernels: 4 waves
#define S3G_VPW 9                               // vertices per wave (seven lanes each)
#define S3G_VPB (S3G_VPW * (S3G_THREADS / 64))  // vertices per block and grid-stride step
#define S3G_MAX_PART 512                        // partial sums per reduction (blocks of the vector kernels)
#define S3G_HUB_DEG 128                         // more slots than this: the vertex is a hub (wave-per-vertex path)
#define S3G_HUB_BLOCKS 16                       // extra blocks of the product kernel that walk the hub list
#define S3G_CG_CHECK 32                         // CG iterations queued between two reads of the done flag
#define S3G_SLOT 49                             // doubles per slot block: seven packed rows of 56 bytes

static_assert(SLAM_S3G_MAX_VERTICES <= (1 << 24) && SLAM_S3G_MAX_EDGES <= (1 << 25), "56 E, 2 E + 1 and 7 V fit int32");
static_assert(SLAM_S3G_STATUS_INDEX == S3G_ST_INDEX && SLAM_S3G_STATUS_ANGLE == S3G_ST_ANGLE && SLAM_S3G_STATUS_PRECOND == S3G_ST_PRECOND &&
              SLAM_S3G_STATUS_BREAKDOWN == S3G_ST_BREAKDOWN && SLAM_S3G_STATUS_NONFINITE == S3G_ST_NONFINITE &&
              SLAM_S3G_STATUS_SCALE == S3G_ST_SCALE, "header and kernel agree");

// device-side scalars of one call (first block of the workspace)
struct s3g_scal {
    double cost, scale, bb, tol2bb, rr;
    unsigned long long maxdiag_bits;
    int status, done, iters, n_hub, n_fixed, pad;
};

// ---- reductions ------------------------------------------------------------------------------------------------------------
// sum of v over the block in a fixed order (xor tree inside a wave, then the waves in ascending order); every thread gets it
__device__ __forceinline__ double s3g_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ double s3g_block_sum(double v, double* sh /*[S3G_THREADS / 64]*/) {
    v = s3g_wave_sum(v);
    __syncthreads();                                  // sh may still be read from an earlier call
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = sh[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); w++) s += sh[w];
    return s;
}
// sum of part[0..n), the same value in every thread of every block that asks
__device__ __forceinline__ double s3g_sum_partials(const double* part, int n, double* sh) {
    double v = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) v += part[i];
    return s3g_block_sum(v, sh);
}

// ---- set-up: index checks, neighbour table, edge -> slot table, hub list ------------------------------------------------------
__global__ void s3g_check_edges_kernel(int V, int E, const int* __restrict__ edges, s3g_scal* sc) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int i = edges[2 * e], j = edges[2 * e + 1];
    if (i < 0 || i >= V || j < 0 || j >= V || i == j) atomicOr(&sc->status, S3G_ST_INDEX);
}
// one lane per vertex: its slots must name edges that have it at that end; writes nbr and slot_of (slot of (edge, side)).
// Nothing is read through an index that was not checked first: the edge check ran in the launch before this one.
__global__ void s3g_setup_vertices_kernel(int V, int E, const int* __restrict__ edges, const int* __restrict__ ptr,
                                          const int* __restrict__ adj, const uint8_t* __restrict__ fixed, int* __restrict__ nbr,
                                          int* __restrict__ slot_of, s3g_scal* sc) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    if (sc->status & S3G_ST_INDEX) return;
    const int lo = ptr[v], hi = ptr[v + 1];
    bool bad = lo < 0 || hi < lo || hi > 2 * E || (v == 0 && lo != 0) || (v == V - 1 && hi != 2 * E);
    if (!bad) {
        for (int k = lo; k < hi; k++) {
            const int a = adj[k];
            if (a < 0 || a >= 2 * E) { bad = true; break; }
            const int e = a >> 1, side = a & 1;
            if (edges[2 * e + side] != v) { bad = true; break; }
            const int u = edges[2 * e + 1 - side];
            nbr[k] = (fixed && fixed[u]) ? -1 : u;
            slot_of[a] = k;
        }
    }
    if (fixed && fixed[v]) atomicAdd(&sc->n_fixed, 1);
    if (bad) atomicOr(&sc->status, S3G_ST_INDEX);
}
// The hub list (vertices with more than S3G_HUB_DEG slots) in ASCENDING VERTEX ORDER, by an ordered compaction: hub h goes to
// wave h mod (waves of the hub blocks) and that wave's share of p.q is a sum over ITS hubs, so the list's order reaches the
// CG scalars.  count / scan (one block) / fill by ballot rank.  Only differences of ptr are read, no index is followed.
__device__ __forceinline__ bool s3g_is_hub(int V, const int* __restrict__ ptr, int v) { return v < V && ptr[v + 1] - ptr[v] > S3G_HUB_DEG; }
__global__ __launch_bounds__(S3G_THREADS) void s3g_hub_count_kernel(int V, const int* __restrict__ ptr, int* __restrict__ hub_off) {
    const int n = __syncthreads_count(s3g_is_hub(V, ptr, blockIdx.x * S3G_THREADS + threadIdx.x));
    if (threadIdx.x == 0) hub_off[blockIdx.x] = n;
}
__global__ __launch_bounds__(S3G_THREADS) void s3g_hub_scan_kernel(int nblocks, int* __restrict__ hub_off, s3g_scal* sc) {
    __shared__ int sh[S3G_THREADS];
    const int per = (nblocks + S3G_THREADS - 1) / S3G_THREADS, lo = threadIdx.x * per, hi = min(lo + per, nblocks);
    int mine = 0;
    for (int i = lo; i < hi; i++) mine += hub_off[i];
    sh[threadIdx.x] = mine;
    __syncthreads();
    int before = 0;
    for (int t = 0; t < (int)threadIdx.x; t++) before += sh[t];
    for (int i = lo; i < hi; i++) { const int c = hub_off[i]; hub_off[i] = before; before += c; }
    if (threadIdx.x == S3G_THREADS - 1) sc->n_hub = before;
}
__global__ __launch_bounds__(S3G_THREADS) void s3g_hub_fill_kernel(int V, const int* __restrict__ ptr, const int* __restrict__ hub_off,
                                                                   int* __restrict__ hubs) {
    __shared__ int wave_n[S3G_THREADS / 64];
    const int v = blockIdx.x * S3G_THREADS + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool hub = s3g_is_hub(V, ptr, v);
    const unsigned long long m = __ballot(hub);
    if (lane == 0) wave_n[wave] = __popcll(m);
    __syncthreads();
    if (!hub) return;
    int rank = __popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; w++) rank += wave_n[w];
    hubs[hub_off[blockIdx.x] + rank] = v;
}
// every (edge, side) must have got exactly one slot (slot_of was filled with -1 before)
__global__ void s3g_check_slots_kernel(int E, const int* __restrict__ adj, const int* __restrict__ slot_of, s3g_scal* sc) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= 2 * E) return;
    if (sc->status & S3G_ST_INDEX) return;
    const int k = slot_of[a];
    if (k < 0 || k >= 2 * E || adj[k] != a) atomicOr(&sc->status, S3G_ST_INDEX);
}

// ---- linearisation: one edge per lane ------------------------------------------------------------------------------------------
template <bool FULL>
__global__ __launch_bounds__(64) void s3g_edge_kernel(int E, const double* __restrict__ sims, const int* __restrict__ edges,
                                                      const double* __restrict__ meas, const double* __restrict__ info,
                                                      const int* __restrict__ slot_of, double huber, int fix_scale, double* __restrict__ S,
                                                      double* __restrict__ Dg, double* __restrict__ W_out,
                                                      double* __restrict__ part_cost, s3g_scal* sc) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    double rho = 0.0;
    if (e < E) {
        const int vi = edges[2 * e], vj = edges[2 * e + 1];
        double Si[13], Sj[13], Z[13];
#pragma unroll
        for (int q = 0; q < 13; q++) { Si[q] = sims[13 * (size_t)vi + q]; Sj[q] = sims[13 * (size_t)vj + q]; Z[q] = meas[13 * (size_t)e + q]; }
        const double* Om = info + 49 * (size_t)e;
        int why;
        if (FULL) {
            const int si = slot_of[2 * e], sj = slot_of[2 * e + 1];
            double* Pi = S + S3G_SLOT * (size_t)si; double* Pj = S + S3G_SLOT * (size_t)sj;
            why = s3g_edge<true>(Si, Sj, Z, Om, huber, fix_scale != 0, &rho, Pi, Pj, W_out ? W_out + 49 * (size_t)e : nullptr,
                                 Dg + 35 * (size_t)si, Dg + 35 * (size_t)sj);
        } else {
            why = s3g_edge<false>(Si, Sj, Z, Om, huber, fix_scale != 0, &rho, nullptr, nullptr, nullptr, nullptr, nullptr);
        }
        if (why) atomicOr(&sc->status, why);
    }
    rho = s3g_wave_sum(rho);
    if (threadIdx.x == 0) part_cost[blockIdx.x] = rho;
}

// H_vv (full 7x7) and b_v: 64 lanes per vertex, lane t < 35 adds term t of the vertex's slots in list order
__global__ __launch_bounds__(S3G_THREADS) void s3g_gather_kernel(int V, const int* __restrict__ ptr, const double* __restrict__ Dg,
                                                                 const uint8_t* __restrict__ fixed, double* __restrict__ Hd,
                                                                 double* __restrict__ b, s3g_scal* sc) {
    const int t = threadIdx.x & 63;
    const int v = blockIdx.x * (S3G_THREADS / 64) + (threadIdx.x >> 6);
    if (v >= V || t >= 35) return;
    const int lo = ptr[v], hi = ptr[v + 1];
    double s = 0.0;
    int k = lo;
    for (; k + 4 <= hi; k += 4) {
        const double d0 = Dg[35 * (size_t)k + t], d1 = Dg[35 * (size_t)(k + 1) + t], d2 = Dg[35 * (size_t)(k + 2) + t],
                     d3 = Dg[35 * (size_t)(k + 3) + t];
        s += d0; s += d1; s += d2; s += d3;
    }
    for (; k < hi; k++) s += Dg[35 * (size_t)k + t];
    if (t >= 28) { b[7 * (size_t)v + t - 28] = s; return; }
    int a = 0, c = t;
    while (c >= 7 - a) { c -= 7 - a; a++; }
    c += a;
    Hd[49 * (size_t)v + a * 7 + c] = s;
    Hd[49 * (size_t)v + c * 7 + a] = s;
    if (a == c && !(fixed && fixed[v]) && s > 0.0)      // largest diagonal entry of the free system (lambda_0): order-free
        atomicMax(&sc->maxdiag_bits, (unsigned long long)__double_as_longlong(s));
}

// *out = sum of part[0..n) in a fixed order (one block)
__global__ __launch_bounds__(S3G_THREADS) void s3g_finish_kernel(const double* __restrict__ part, int n, double* out) {
    __shared__ double sh[S3G_THREADS / 64];
    const double s = s3g_sum_partials(part, n, sh);
    if (threadIdx.x == 0) *out = s;
}
__global__ __launch_bounds__(S3G_THREADS) void s3g_finish_bb_kernel(const double* __restrict__ part, int n, double tol, s3g_scal* sc) {
    __shared__ double sh[S3G_THREADS / 64];
    const double s = s3g_sum_partials(part, n, sh);
    if (threadIdx.x == 0) {
        sc->bb = s; sc->rr = s; sc->tol2bb = tol * tol * s; sc->done = 0; sc->iters = 0;
        if (!isfinite(s)) atomicOr(&sc->status, S3G_ST_NONFINITE);      // a right-hand side that is not finite: no iteration will run
    }
}

// edge-ordered W_e -> the slots of both ends (the hooks that are handed blocks instead of similarities)
__global__ void s3g_pack_kernel(int E, const double* __restrict__ W, const int* __restrict__ slot_of, double* __restrict__ S) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 49 * E) return;
    const int e = idx / 49, q = idx - 49 * e, a = q / 7, c = q - 7 * a;
    const double v = W[idx];
    double* Pi = S + S3G_SLOT * (size_t)slot_of[2 * e]; double* Pj = S + S3G_SLOT * (size_t)slot_of[2 * e + 1];
    Pi[a * 7 + c] = v;
    Pj[c * 7 + a] = v;
}

// ---- the product -----------------------------------------------------------------------------------------------------------------
// one packed row of seven doubles (8-byte loads: alternate 56-byte rows are not 16-byte aligned) times x_u [7]; the additions
// in one stated order
__device__ __forceinline__ double s3g_row_dot(const double* __restrict__ m, const double* __restrict__ x) {
    return ((m[0] * x[0] + m[1] * x[1]) + (m[2] * x[2] + m[3] * x[3])) + ((m[4] * x[4] + m[5] * x[5]) + m[6] * x[6]);
}
__device__ __forceinline__ double s3g_slot_term(const double* __restrict__ S, const int* __restrict__ nbr, const double* __restrict__ x,
                                                int k, int row) {
    const int u = nbr[k];
    return u >= 0 ? s3g_row_dot(S + S3G_SLOT * (size_t)k + 7 * row, x + 7 * (size_t)u) : 0.0;
}
// row `row` of (H_vv + lambda I) x_v + sum over the slots [lo, hi) of v of S[k] x_nbr[k]
__device__ __forceinline__ double s3g_vertex_row(int v, int row, const int* __restrict__ nbr, const double* __restrict__ S,
                                                 const double* __restrict__ Hd, double lambda, const double* __restrict__ x, int lo,
                                                 int hi) {
    double y = s3g_row_dot(Hd + 49 * (size_t)v + 7 * row, x + 7 * (size_t)v) + lambda * x[7 * (size_t)v + row];
    int k = lo;
    for (; k + 4 <= hi; k += 4) {
        const double t0 = s3g_slot_term(S, nbr, x, k, row), t1 = s3g_slot_term(S, nbr, x, k + 1, row),
                     t2 = s3g_slot_term(S, nbr, x, k + 2, row), t3 = s3g_slot_term(S, nbr, x, k + 3, row);
        y += t0; y += t1; y += t2; y += t3;
    }
    for (; k < hi; k++) y += s3g_slot_term(S, nbr, x, k, row);
    return y;
}
// a hub: the wave's nine lane groups take the slots lo + g, lo + g + 9, ...; the nine partial rows meet in LDS and are added
// in group order behind the diagonal term (all 64 lanes of the wave call this together; lane 63 is group 9 and adds nothing)
__device__ __forceinline__ double s3g_hub_row(int v, int g, int row, const int* __restrict__ nbr, const double* __restrict__ S,
                                              const double* __restrict__ Hd, double lambda, const double* __restrict__ x, int lo,
                                              int hi, volatile double* sh /*[64] of this wave*/) {
    double part = 0.0;
    if (g < S3G_VPW)
        for (int k = lo + g; k < hi; k += S3G_VPW) part += s3g_slot_term(S, nbr, x, k, row);
    sh[threadIdx.x & 63] = part;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    double y = s3g_row_dot(Hd + 49 * (size_t)v + 7 * row, x + 7 * (size_t)v) + lambda * x[7 * (size_t)v + row];
    for (int q = 0; q < S3G_VPW; q++) y += sh[q * 7 + row];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    return y;
}

// MODE 0: y = A x.  MODE 1 (CG): q = A p and part[block] = the block's share of p.q; nothing once sc->done is set, which the
// kernel itself sets (block 0) when the residual of the iteration before met the tolerance.
template <int MODE>
__global__ __launch_bounds__(S3G_THREADS) void s3g_hmul_kernel(int V, int main_blocks, const int* __restrict__ ptr,
                                                               const int* __restrict__ nbr, const uint8_t* __restrict__ fixed,
                                                               const int* __restrict__ hubs, const double* __restrict__ S,
                                                               const double* __restrict__ Hd, double lambda,
                                                               const double* __restrict__ x, double* __restrict__ y,
                                                               double* __restrict__ part, s3g_scal* sc) {
    __shared__ double sh[S3G_THREADS];
    __shared__ double shw[S3G_THREADS / 64];
    if (MODE == 1) {
        if (sc->done) return;
        if (!(sc->rr > sc->tol2bb)) {                  // converged (or not a number): this launch and all later ones are no-ops
            if (blockIdx.x == 0 && threadIdx.x == 0) sc->done = 1;
            return;
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane / 7, row = lane - 7 * g;
    double dot = 0.0;
    if ((int)blockIdx.x < main_blocks) {
        for (int base = blockIdx.x * S3G_VPB; base < V; base += main_blocks * S3G_VPB) {
            const int v = base + wave * S3G_VPW + g;
            if (g >= S3G_VPW || v >= V) continue;
            const int lo = ptr[v], hi = ptr[v + 1];
            if (hi - lo > S3G_HUB_DEG) continue;       // a hub block writes it
            double r = 0.0;
            if (!fixed[v]) r = s3g_vertex_row(v, row, nbr, S, Hd, lambda, x, lo, hi);
            y[7 * (size_t)v + row] = r;
            if (MODE == 1) dot += r * x[7 * (size_t)v + row];
        }
    } else {
        const int n_hub = sc->n_hub, waves = (gridDim.x - main_blocks) * (S3G_THREADS / 64);
        for (int h = (blockIdx.x - main_blocks) * (S3G_THREADS / 64) + wave; h < n_hub; h += waves) {
            const int v = hubs[h];
            const double r = fixed[v] ? 0.0 : s3g_hub_row(v, g, row, nbr, S, Hd, lambda, x, ptr[v], ptr[v + 1], sh + 64 * wave);
            if (g == 0) {
                y[7 * (size_t)v + row] = r;
                if (MODE == 1) dot += r * x[7 * (size_t)v + row];
            }
        }
    }
    if (MODE == 1) {
        const double s = s3g_block_sum(dot, shw);
        if (threadIdx.x == 0) part[blockIdx.x] = s;
    }
}

// ---- CG vector kernels (the product's seven-lane mapping, `nblocks` blocks with a grid stride) -------------------------------------
// Minv_v = (H_vv + lambda I)^-1, one lane per vertex
__global__ __launch_bounds__(64) void s3g_precond_kernel(int V, const double* __restrict__ Hd, const uint8_t* __restrict__ fixed,
                                                         double lambda, double* __restrict__ Minv, s3g_scal* sc) {
    const int v = blockIdx.x * 64 + threadIdx.x;
    if (v >= V) return;
    double A[49], Inv[49];
#pragma unroll
    for (int q = 0; q < 49; q++) A[q] = Hd[49 * (size_t)v + q] + ((q % 8 == 0) ? lambda : 0.0);
    if (!s3g_inverse7(A, Inv) && !fixed[v]) atomicOr(&sc->status, S3G_ST_PRECOND);
#pragma unroll
    for (int q = 0; q < 49; q++) Minv[49 * (size_t)v + q] = Inv[q];
}
// x = 0, r = -b (0 on fixed vertices), z = Minv r, p = z; partials of r.z (parity 0) and of b.b
__global__ __launch_bounds__(S3G_THREADS) void s3g_cg_init_kernel(int V, int nblocks, const uint8_t* __restrict__ fixed,
                                                                  const double* __restrict__ b, const double* __restrict__ Minv,
                                                                  double* __restrict__ x, double* __restrict__ r, double* __restrict__ z,
                                                                  double* __restrict__ p, double* __restrict__ part_rz,
                                                                  double* __restrict__ part_rr) {
    __shared__ double shw[S3G_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane / 7, row = lane - 7 * g;
    double rz = 0.0, rr = 0.0;
    for (int base = blockIdx.x * S3G_VPB; base < V; base += nblocks * S3G_VPB) {
        const int v = base + wave * S3G_VPW + g;
        if (g >= S3G_VPW || v >= V) continue;
        const bool fx = fixed[v];
        double rv[7];
#pragma unroll
        for (int c = 0; c < 7; c++) rv[c] = fx ? 0.0 : -b[7 * (size_t)v + c];
        const double zr = fx ? 0.0 : s3g_row_dot(Minv + 49 * (size_t)v + 7 * row, rv);
        const size_t o = 7 * (size_t)v + row;
        x[o] = 0.0; r[o] = rv[row]; z[o] = zr; p[o] = zr;
        rz += rv[row] * zr;
        rr += rv[row] * rv[row];
    }
    const double s0 = s3g_block_sum(rz, shw), s1 = s3g_block_sum(rr, shw);
    if (threadIdx.x == 0) { part_rz[blockIdx.x] = s0; part_rr[blockIdx.x] = s1; }
}
// alpha = r.z / p.q; x += alpha p; r -= alpha q (into r_out: the seven lanes of a vertex all read r_v); z = Minv r; partials of
// the new r.z and r.r.  A p.q that is not positive ends the solve with the status bit (every block decides alike).
__global__ __launch_bounds__(S3G_THREADS) void s3g_cg_update_kernel(int V, int nblocks, int hmul_blocks, const double* __restrict__ Minv,
                                                                    const double* __restrict__ p, const double* __restrict__ q,
                                                                    double* __restrict__ x, const double* __restrict__ r,
                                                                    double* __restrict__ r_out, double* __restrict__ z,
                                                                    const double* __restrict__ part_pq, const double* __restrict__ part_rz_old,
                                                                    double* __restrict__ part_rz_new, double* __restrict__ part_rr,
                                                                    s3g_scal* sc) {
    __shared__ double shw[S3G_THREADS / 64];
    __shared__ int was_done;
    // read once per block: block 0 sets the flag on a breakdown inside this very launch, and waves of one block that saw
    // different values would part ways before a block-wide sum
    if (threadIdx.x == 0) was_done = sc->done;
    __syncthreads();
    if (was_done) return;
    const double pq = s3g_sum_partials(part_pq, hmul_blocks, shw), rz_old = s3g_sum_partials(part_rz_old, nblocks, shw);
    if (!(pq > 0.0) || !isfinite(pq) || !isfinite(rz_old)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { atomicOr(&sc->status, S3G_ST_BREAKDOWN); sc->done = 1; }
        return;
    }
    const double alpha = rz_old / pq;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane / 7, row = lane - 7 * g;
    double rz = 0.0, rr = 0.0;
    for (int base = blockIdx.x * S3G_VPB; base < V; base += nblocks * S3G_VPB) {
        const int v = base + wave * S3G_VPW + g;
        if (g >= S3G_VPW || v >= V) continue;
        double rv[7];
#pragma unroll
        for (int c = 0; c < 7; c++) rv[c] = r[7 * (size_t)v + c] - alpha * q[7 * (size_t)v + c];
        const double zr = s3g_row_dot(Minv + 49 * (size_t)v + 7 * row, rv);
        const size_t o = 7 * (size_t)v + row;
        x[o] = x[o] + alpha * p[o];
        r_out[o] = rv[row];
        z[o] = zr;
        rz += rv[row] * zr;
        rr += rv[row] * rv[row];
    }
    const double s0 = s3g_block_sum(rz, shw), s1 = s3g_block_sum(rr, shw);
    if (threadIdx.x == 0) { part_rz_new[blockIdx.x] = s0; part_rr[blockIdx.x] = s1; }
}
// beta = r.z new / r.z old; p = z + beta p; block 0 publishes r.r and the iteration count (the next product kernel turns
// r.r into the done flag)
__global__ __launch_bounds__(S3G_THREADS) void s3g_cg_direction_kernel(int V, int nblocks, const double* __restrict__ z, double* __restrict__ p,
                                                                       const double* __restrict__ part_rz_old,
                                                                       const double* __restrict__ part_rz_new,
                                                                       const double* __restrict__ part_rr, s3g_scal* sc) {
    __shared__ double shw[S3G_THREADS / 64];
    if (sc->done) return;
    const double rz_old = s3g_sum_partials(part_rz_old, nblocks, shw), rz_new = s3g_sum_partials(part_rz_new, nblocks, shw);
    const double rr = s3g_sum_partials(part_rr, nblocks, shw);
    const double beta = rz_new / rz_old;
    for (int i = blockIdx.x * S3G_THREADS + threadIdx.x; i < 7 * V; i += nblocks * S3G_THREADS) p[i] = z[i] + beta * p[i];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        sc->rr = rr;
        sc->iters = sc->iters + 1;
        if (!isfinite(rr) || !isfinite(beta)) atomicOr(&sc->status, S3G_ST_NONFINITE);
    }
}
__global__ void s3g_cg_close_kernel(s3g_scal* sc) {    // behind the last queued iteration: the decision the next product would take
    if (!(sc->rr > sc->tol2bb)) sc->done = 1;
}

// candidates Phi(x_v) o S_v (fixed ones copied), partials of the gain ratio's denominator x.(lambda x - b)
__global__ __launch_bounds__(S3G_THREADS) void s3g_candidate_kernel(int V, const double* __restrict__ sims, const uint8_t* __restrict__ fixed,
                                                                    const double* __restrict__ x, const double* __restrict__ b, double lambda,
                                                                    double* __restrict__ out, double* __restrict__ part_scale) {
    __shared__ double shw[S3G_THREADS / 64];
    const int v = blockIdx.x * S3G_THREADS + threadIdx.x;
    double sc = 0.0;
    if (v < V) {
        double T[13], Tn[13];
#pragma unroll
        for (int q = 0; q < 13; q++) T[q] = sims[13 * (size_t)v + q];
        if (fixed[v]) {
#pragma unroll
            for (int q = 0; q < 13; q++) out[13 * (size_t)v + q] = T[q];
        } else {
            double dx[7];
#pragma unroll
            for (int q = 0; q < 7; q++) { dx[q] = x[7 * (size_t)v + q]; sc += dx[q] * (lambda * dx[q] - b[7 * (size_t)v + q]); }
            s3g_apply_update(dx, T, Tn);
#pragma unroll
            for (int q = 0; q < 13; q++) out[13 * (size_t)v + q] = Tn[q];
        }
    }
    const double s = s3g_block_sum(sc, shw);
    if (threadIdx.x == 0) part_scale[blockIdx.x] = s;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
static inline uint64_t s3g_up(uint64_t b) { return (b + 255) & ~(uint64_t)255; }
static inline int s3g_vec_blocks(int64_t V) { int64_t n = (V + S3G_VPB - 1) / S3G_VPB; return (int)(n < 1 ? 1 : n > S3G_MAX_PART ? S3G_MAX_PART : n); }
static inline int s3g_edge_blocks(int64_t E) { return (int)((E + 63) / 64); }
static inline int s3g_cand_blocks(int64_t V) { return (int)((V + S3G_THREADS - 1) / S3G_THREADS); }

struct s3g_layout {
    uint64_t scal, nbr, slot_of, hubs, hub_off, S, Dg, Hd, b, Minv, x, r, r2, z, p, q, part_cost, part_a, part_b, part_c, part_d, sims2, total;
};
static s3g_layout s3g_make_layout(int64_t V, int64_t E) {
    s3g_layout L;
    uint64_t o = 0;
    const uint64_t v = (uint64_t)(V > 0 ? V : 1), e = (uint64_t)(E > 0 ? E : 1);
    auto take = [&](uint64_t bytes) { const uint64_t at = o; o += s3g_up(bytes); return at; };
    L.scal = take(sizeof(s3g_scal));
    L.nbr = take(2 * e * 4); L.slot_of = take(2 * e * 4); L.hubs = take(v * 4); L.hub_off = take((uint64_t)s3g_cand_blocks((int64_t)v) * 4);
    L.S = take(2 * e * S3G_SLOT * 8); L.Dg = take(2 * e * 35 * 8);
    L.Hd = take(v * 49 * 8); L.b = take(v * 7 * 8); L.Minv = take(v * 49 * 8);
    L.x = take(v * 56); L.r = take(v * 56); L.r2 = take(v * 56); L.z = take(v * 56); L.p = take(v * 56); L.q = take(v * 56);
    const int eb = s3g_edge_blocks((int64_t)e), cb = s3g_cand_blocks((int64_t)v);
    L.part_cost = take((uint64_t)(eb > cb ? eb : cb) * 8);
    const uint64_t pb = (uint64_t)(S3G_MAX_PART + S3G_HUB_BLOCKS) * 8;
    L.part_a = take(pb); L.part_b = take(pb); L.part_c = take(pb); L.part_d = take(pb);
    L.sims2 = take(2 * v * 104);
    L.total = o;
    return L;
}

static int s3g_common_checks(const char* who, slam_ctx* ctx, int64_t V, int64_t E) {
    SLAM_REQUIRE(ctx, "%s: null ctx", who);
    SLAM_REQUIRE(V >= 0 && V <= SLAM_S3G_MAX_VERTICES && E >= 0 && E <= SLAM_S3G_MAX_EDGES, "%s: bad sizes (V=%lld, E=%lld; limits 2^24 and 2^25)",
                 who, (long long)V, (long long)E);
    SLAM_REQUIRE(E == 0 || V > 0, "%s: edges without vertices", who);
    return SLAM_OK;
}

extern "C" int slam_s3g_workspace(int64_t V, int64_t E, uint64_t* bytes) {
    SLAM_REQUIRE(bytes, "slam_s3g_workspace: null bytes");
    SLAM_REQUIRE(V >= 0 && V <= SLAM_S3G_MAX_VERTICES && E >= 0 && E <= SLAM_S3G_MAX_EDGES, "bad sizes (V=%lld, E=%lld)", (long long)V, (long long)E);
    *bytes = s3g_make_layout(V, E).total;
    return SLAM_OK;
}

extern "C" int slam_s3g_plan(int64_t V, int64_t E, int32_t* plan) {
    SLAM_REQUIRE(plan, "slam_s3g_plan: null plan");
    SLAM_REQUIRE(V >= 0 && V <= SLAM_S3G_MAX_VERTICES && E >= 0 && E <= SLAM_S3G_MAX_EDGES, "bad sizes (V=%lld, E=%lld)", (long long)V, (long long)E);
    plan[0] = s3g_vec_blocks(V);         // blocks of the product's main path and of the CG vector kernels (= partial sums per dot)
    plan[1] = S3G_HUB_BLOCKS;            // extra blocks of the product kernel for the hub list
    plan[2] = S3G_VPB;                   // vertices per block and grid-stride step (seven lanes each)
    plan[3] = S3G_HUB_DEG;               // a vertex with more slots than this takes the wave-per-vertex path
    plan[4] = s3g_edge_blocks(E);        // blocks of the edge kernel (= partial sums of the cost)
    plan[5] = S3G_CG_CHECK;              // CG iterations queued between two reads of the done flag
    plan[6] = 3;                         // launches per CG iteration
    plan[7] = 7;                         // doubles per stored row of a slot block (packed)
    return SLAM_OK;
}

struct s3g_graph {                       // device views of one call
    int V, E;
    const int *edges, *ptr, *adj;
    const uint8_t* fixed;
    uint8_t* ws;
    s3g_layout L;
    s3g_scal* sc;
    int vb;                              // blocks of the vector kernels
    template <class T> T* at(uint64_t off) const { return (T*)(ws + off); }
};

static void s3g_open(s3g_graph& G, int64_t V, int64_t E, const int32_t* d_edges, const int32_t* d_ptr, const int32_t* d_adj,
                     const uint8_t* d_fixed, void* ws) {
    G.V = (int)V; G.E = (int)E; G.edges = d_edges; G.ptr = d_ptr; G.adj = d_adj; G.fixed = d_fixed;
    G.L = s3g_make_layout(V, E);
    G.ws = (uint8_t*)ws;
    G.sc = G.at<s3g_scal>(G.L.scal);
    G.vb = s3g_vec_blocks(V);
}

// checks and tables; reads the status back (ONE synchronisation per call, before any kernel follows an index)
static int s3g_setup(slam_ctx* ctx, s3g_graph& G, s3g_scal* h_scal /*pinned*/, const char* who, int64_t n_fixed_claimed) {
    hipStream_t st = ctx->stream;
    SLAM_HIP(hipMemsetAsync(G.sc, 0, sizeof(s3g_scal), st));
    if (G.E > 0) {
        SLAM_HIP(hipMemsetAsync(G.at<int>(G.L.slot_of), 0xFF, (size_t)2 * G.E * 4, st));
        s3g_check_edges_kernel<<<(G.E + 255) / 256, 256, 0, st>>>(G.V, G.E, G.edges, G.sc);
    }
    s3g_setup_vertices_kernel<<<(G.V + 255) / 256, 256, 0, st>>>(G.V, G.E, G.edges, G.ptr, G.adj, G.fixed, G.at<int>(G.L.nbr),
                                                                  G.at<int>(G.L.slot_of), G.sc);
    {
        const int hb = s3g_cand_blocks(G.V);
        s3g_hub_count_kernel<<<hb, S3G_THREADS, 0, st>>>(G.V, G.ptr, G.at<int>(G.L.hub_off));
        s3g_hub_scan_kernel<<<1, S3G_THREADS, 0, st>>>(hb, G.at<int>(G.L.hub_off), G.sc);
        s3g_hub_fill_kernel<<<hb, S3G_THREADS, 0, st>>>(G.V, G.ptr, G.at<int>(G.L.hub_off), G.at<int>(G.L.hubs));
    }
    if (G.E > 0) s3g_check_slots_kernel<<<(2 * G.E + 255) / 256, 256, 0, st>>>(G.E, G.adj, G.at<int>(G.L.slot_of), G.sc);
    SLAM_HIP(hipGetLastError());
    SLAM_HIP(hipMemcpyAsync(h_scal, G.sc, sizeof(s3g_scal), hipMemcpyDeviceToHost, st));
    SLAM_HIP(hipStreamSynchronize(st));
    if (h_scal->status & S3G_ST_INDEX)
        return slam_set_error(SLAM_ERR_INVALID, "%s: an edge index outside [0, V), a self-edge, or a vertex list that does not match the edges", who);
    if (n_fixed_claimed >= 0 && h_scal->n_fixed != n_fixed_claimed)
        return slam_set_error(SLAM_ERR_INVALID, "%s: n_fixed = %lld but the mask fixes %d vertices", who, (long long)n_fixed_claimed, h_scal->n_fixed);
    return SLAM_OK;
}

static int s3g_linearize(slam_ctx* ctx, const s3g_graph& G, const double* sims, const double* meas, const double* info, double huber,
                         int fix_scale, double* Hd, double* b, double* W_out, double* d_cost) {
    hipStream_t st = ctx->stream;
    SLAM_HIP(hipMemsetAsync(&G.sc->maxdiag_bits, 0, 8, st));
    if (G.E > 0)
        s3g_edge_kernel<true><<<s3g_edge_blocks(G.E), 64, 0, st>>>(G.E, sims, G.edges, meas, info, G.at<int>(G.L.slot_of), huber, fix_scale,
                                                                  G.at<double>(G.L.S), G.at<double>(G.L.Dg), W_out, G.at<double>(G.L.part_cost), G.sc);
    s3g_gather_kernel<<<(G.V + 3) / 4, S3G_THREADS, 0, st>>>(G.V, G.ptr, G.at<double>(G.L.Dg), G.fixed, Hd, b, G.sc);
    s3g_finish_kernel<<<1, S3G_THREADS, 0, st>>>(G.at<double>(G.L.part_cost), s3g_edge_blocks(G.E), d_cost);
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

static int s3g_hmul(slam_ctx* ctx, const s3g_graph& G, const double* Hd, double lambda, const double* x, double* y) {
    s3g_hmul_kernel<0><<<G.vb + S3G_HUB_BLOCKS, S3G_THREADS, 0, ctx->stream>>>(G.V, G.vb, G.ptr, G.at<int>(G.L.nbr), G.fixed, G.at<int>(G.L.hubs),
                                                                              G.at<double>(G.L.S), Hd, lambda, x, y, nullptr, G.sc);
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

// (H + lambda I) x = -b: at most max_iter iterations of three launches each, the done flag read every S3G_CG_CHECK iterations
static int s3g_pcg(slam_ctx* ctx, const s3g_graph& G, const double* Hd, const double* b, double lambda, double tol, int max_iter, double* x,
                   s3g_scal* h_scal) {
    hipStream_t st = ctx->stream;
    double *Minv = G.at<double>(G.L.Minv), *z = G.at<double>(G.L.z), *p = G.at<double>(G.L.p), *q = G.at<double>(G.L.q);
    double* r[2] = {G.at<double>(G.L.r), G.at<double>(G.L.r2)};
    double *part_pq = G.at<double>(G.L.part_a), *part_rr = G.at<double>(G.L.part_b);
    double* part_rz[2] = {G.at<double>(G.L.part_c), G.at<double>(G.L.part_d)};
    const int hb = G.vb + S3G_HUB_BLOCKS;
    s3g_precond_kernel<<<(G.V + 63) / 64, 64, 0, st>>>(G.V, Hd, G.fixed, lambda, Minv, G.sc);
    s3g_cg_init_kernel<<<G.vb, S3G_THREADS, 0, st>>>(G.V, G.vb, G.fixed, b, Minv, x, r[0], z, p, part_rz[0], part_rr);
    s3g_finish_bb_kernel<<<1, S3G_THREADS, 0, st>>>(part_rr, G.vb, tol, G.sc);
    SLAM_HIP(hipGetLastError());
    for (int n = 0; n < max_iter; n++) {
        const int a = n & 1, c = a ^ 1;
        s3g_hmul_kernel<1><<<hb, S3G_THREADS, 0, st>>>(G.V, G.vb, G.ptr, G.at<int>(G.L.nbr), G.fixed, G.at<int>(G.L.hubs), G.at<double>(G.L.S), Hd,
                                                       lambda, p, q, part_pq, G.sc);
        s3g_cg_update_kernel<<<G.vb, S3G_THREADS, 0, st>>>(G.V, G.vb, hb, Minv, p, q, x, r[a], r[c], z, part_pq, part_rz[a], part_rz[c], part_rr, G.sc);
        s3g_cg_direction_kernel<<<G.vb, S3G_THREADS, 0, st>>>(G.V, G.vb, z, p, part_rz[a], part_rz[c], part_rr, G.sc);
        if ((n + 1) % S3G_CG_CHECK == 0 && n + 1 < max_iter) {
            s3g_cg_close_kernel<<<1, 1, 0, st>>>(G.sc);
            SLAM_HIP(hipGetLastError());
            SLAM_HIP(hipMemcpyAsync(h_scal, G.sc, sizeof(s3g_scal), hipMemcpyDeviceToHost, st));
            SLAM_HIP(hipStreamSynchronize(st));
            if (h_scal->done) break;
        }
    }
    s3g_cg_close_kernel<<<1, 1, 0, st>>>(G.sc);
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

// workspace + a pinned block for the scalars (call lock held)
static int s3g_blocks(slam_ctx* ctx, int64_t V, int64_t E, void** ws, s3g_scal** hs) {
    void *dev = nullptr, *host = nullptr;
    if (int rc = slam_io_arena(ctx, 0, 256, &dev, &host)) return rc;
    if (int rc = slam_workspace(ctx, s3g_make_layout(V, E).total, ws)) return rc;
    *hs = (s3g_scal*)host;
    return SLAM_OK;
}

extern "C" int slam_s3g_linearize_f64(slam_ctx* ctx, int64_t V, int64_t E, const double* d_sims, const int32_t* d_edges, const double* d_meas,
                                      const double* d_info, const int32_t* d_vtx_ptr, const int32_t* d_vtx_adj, double huber_delta,
                                      double* d_cost, double* d_grad, double* d_Hdiag, double* d_W, int32_t* h_status) {
    if (int rc = s3g_common_checks("slam_s3g_linearize_f64", ctx, V, E)) return rc;
    SLAM_REQUIRE(huber_delta >= 0.0, "slam_s3g_linearize_f64: huber_delta must not be negative");
    SLAM_REQUIRE(d_cost && h_status && (V == 0 || (d_vtx_ptr && d_sims && d_grad && d_Hdiag)) &&
                     (E == 0 || (d_edges && d_meas && d_info && d_vtx_adj && d_W)), "slam_s3g_linearize_f64: null pointer");
    SLAM_HIP(hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> lk(ctx->call_mu);
    *h_status = 0;
    if (V == 0) { SLAM_HIP(hipMemsetAsync(d_cost, 0, 8, ctx->stream)); return SLAM_OK; }
    void* ws = nullptr;
    s3g_scal* hs = nullptr;
    if (int rc = s3g_blocks(ctx, V, E, &ws, &hs)) return rc;
    s3g_graph G;
    s3g_open(G, V, E, d_edges, d_vtx_ptr, d_vtx_adj, nullptr, ws);
    if (int rc = s3g_setup(ctx, G, hs, "slam_s3g_linearize_f64", -1)) return rc;
    if (int rc = s3g_linearize(ctx, G, d_sims, d_meas, d_info, huber_delta, 0, d_Hdiag, d_grad, d_W, d_cost)) return rc;
    SLAM_HIP(hipMemcpyAsync(hs, G.sc, sizeof(s3g_scal), hipMemcpyDeviceToHost, ctx->stream));
    SLAM_HIP(hipStreamSynchronize(ctx->stream));
    *h_status = hs->status;
    return SLAM_OK;
}

extern "C" int slam_s3g_hmul_f64(slam_ctx* ctx, int64_t V, int64_t E, const int32_t* d_edges, const int32_t* d_vtx_ptr, const int32_t* d_vtx_adj,
                                 const uint8_t* d_fixed, const double* d_Hdiag, const double* d_W, double lambda, const double* d_x, double* d_y) {
    if (int rc = s3g_common_checks("slam_s3g_hmul_f64", ctx, V, E)) return rc;
    if (V == 0) return SLAM_OK;
    SLAM_REQUIRE(d_vtx_ptr && d_fixed && d_Hdiag && d_x && d_y && (E == 0 || (d_edges && d_vtx_adj && d_W)), "slam_s3g_hmul_f64: null pointer");
    SLAM_HIP(hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> lk(ctx->call_mu);
    void* ws = nullptr;
    s3g_scal* hs = nullptr;
    if (int rc = s3g_blocks(ctx, V, E, &ws, &hs)) return rc;
    s3g_graph G;
    s3g_open(G, V, E, d_edges, d_vtx_ptr, d_vtx_adj, d_fixed, ws);
    if (int rc = s3g_setup(ctx, G, hs, "slam_s3g_hmul_f64", -1)) return rc;
    if (E > 0) s3g_pack_kernel<<<(unsigned)((49 * E + 255) / 256), 256, 0, ctx->stream>>>((int)E, d_W, G.at<int>(G.L.slot_of), G.at<double>(G.L.S));
    return s3g_hmul(ctx, G, d_Hdiag, lambda, d_x, d_y);
}

extern "C" int slam_s3g_pcg_f64(slam_ctx* ctx, int64_t V, int64_t E, const int32_t* d_edges, const int32_t* d_vtx_ptr, const int32_t* d_vtx_adj,
                                const uint8_t* d_fixed, const double* d_Hdiag, const double* d_W, const double* d_b, double lambda, double tol,
                                int max_iter, double* d_x, double* h_stats) {
    if (int rc = s3g_common_checks("slam_s3g_pcg_f64", ctx, V, E)) return rc;
    SLAM_REQUIRE(h_stats, "slam_s3g_pcg_f64: null h_stats");
    SLAM_REQUIRE(tol > 0.0 && tol < 1.0 && max_iter >= 1 && max_iter <= (1 << 20) && lambda >= 0.0,
                 "slam_s3g_pcg_f64: 0 < tol < 1, lambda >= 0, max_iter in [1, 2^20]");
    for (int i = 0; i < 4; i++) h_stats[i] = 0.0;
    if (V == 0) return SLAM_OK;
    SLAM_REQUIRE(d_vtx_ptr && d_fixed && d_Hdiag && d_b && d_x && (E == 0 || (d_edges && d_vtx_adj && d_W)), "slam_s3g_pcg_f64: null pointer");
    SLAM_HIP(hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> lk(ctx->call_mu);
    void* ws = nullptr;
    s3g_scal* hs = nullptr;
    if (int rc = s3g_blocks(ctx, V, E, &ws, &hs)) return rc;
    s3g_graph G;
    s3g_open(G, V, E, d_edges, d_vtx_ptr, d_vtx_adj, d_fixed, ws);
    if (int rc = s3g_setup(ctx, G, hs, "slam_s3g_pcg_f64", -1)) return rc;
    if (E > 0) s3g_pack_kernel<<<(unsigned)((49 * E + 255) / 256), 256, 0, ctx->stream>>>((int)E, d_W, G.at<int>(G.L.slot_of), G.at<double>(G.L.S));
    if (int rc = s3g_pcg(ctx, G, d_Hdiag, d_b, lambda, tol, max_iter, d_x, hs)) return rc;
    SLAM_HIP(hipMemcpyAsync(hs, G.sc, sizeof(s3g_scal), hipMemcpyDeviceToHost, ctx->stream));
    SLAM_HIP(hipStreamSynchronize(ctx->stream));
    // converged = the tolerance was met by a finite residual; `done` is only the stop flag (breakdown and NaN set it too)
    h_stats[0] = hs->iters; h_stats[1] = (isfinite(hs->rr) && hs->rr <= hs->tol2bb) ? 1.0 : 0.0;
    h_stats[2] = hs->bb == 0.0 ? 0.0 : sqrt(hs->rr / hs->bb); h_stats[3] = hs->status;
    return SLAM_OK;
}

// the LM loop on a set-up graph (call lock held).  hs: pinned.  d_sims in -> d_out.
static int s3g_optimize_locked(slam_ctx* ctx, s3g_graph& G, const double* d_sims, const double* d_meas, const double* d_info, int iterations,
                               double huber, double tol, int max_iter, int fix_scale, double* d_out, double* h_stats, s3g_scal* hs) {
    hipStream_t st = ctx->stream;
    const int V = G.V;
    double* cur = G.at<double>(G.L.sims2);
    double* cand = cur + 13 * (size_t)V;
    double *Hd = G.at<double>(G.L.Hd), *b = G.at<double>(G.L.b), *x = G.at<double>(G.L.x);
    const int bad_state = S3G_ST_ANGLE | S3G_ST_NONFINITE | S3G_ST_SCALE;
    SLAM_HIP(hipMemcpyAsync(cur, d_sims, (size_t)V * 104, hipMemcpyDeviceToDevice, st));
    if (int rc = s3g_linearize(ctx, G, cur, d_meas, d_info, huber, fix_scale, Hd, b, nullptr, &G.sc->cost)) return rc;
    SLAM_HIP(hipMemcpyAsync(hs, G.sc, sizeof(s3g_scal), hipMemcpyDeviceToHost, st));
    SLAM_HIP(hipStreamSynchronize(st));
    double F = hs->cost, maxdiag;
    memcpy(&maxdiag, &hs->maxdiag_bits, 8);
    const double F0 = F;
    double lambda = 1e-5 * (maxdiag > 1e-12 ? maxdiag : 1e-12), ni = 2.0;      // tau * max diagonal (g2o, as pose_graph.hip)
    int status = hs->status, accepted = 0, trials = 0;
    long long cg_total = 0;
    bool stop = !(F - F == 0.0) || (status & bad_state) != 0;
    for (int it = 0; it < iterations && !stop; it++) {
        bool taken = false;
        for (int trial = 0; trial < 10 && !stop; trial++) {                   // maxTrialsAfterFailure
            // the bits of this trial alone: a candidate that is turned down leaves none behind
            SLAM_HIP(hipMemsetAsync(&G.sc->status, 0, 4, st));
            if (int rc = s3g_pcg(ctx, G, Hd, b, lambda, tol, max_iter, x, hs)) return rc;
            s3g_candidate_kernel<<<s3g_cand_blocks(V), S3G_THREADS, 0, st>>>(V, cur, G.fixed, x, b, lambda, cand, G.at<double>(G.L.part_cost));
            s3g_finish_kernel<<<1, S3G_THREADS, 0, st>>>(G.at<double>(G.L.part_cost), s3g_cand_blocks(V), &G.sc->scale);
            s3g_edge_kernel<false><<<s3g_edge_blocks(G.E), 64, 0, st>>>(G.E, cand, G.edges, d_meas, d_info, nullptr, huber, fix_scale, nullptr, nullptr,
                                                                       nullptr, G.at<double>(G.L.part_cost), G.sc);
            s3g_finish_kernel<<<1, S3G_THREADS, 0, st>>>(G.at<double>(G.L.part_cost), s3g_edge_blocks(G.E), &G.sc->cost);
            SLAM_HIP(hipGetLastError());
            SLAM_HIP(hipMemcpyAsync(hs, G.sc, sizeof(s3g_scal), hipMemcpyDeviceToHost, st));
            SLAM_HIP(hipStreamSynchronize(st));
            trials++;
            cg_total += hs->iters;
            status |= hs->status & (S3G_ST_PRECOND | S3G_ST_BREAKDOWN);
            const double Fc = hs->cost, scale = hs->scale + 1e-3;
            const bool usable = !(hs->status & bad_state) && Fc - Fc == 0.0 && scale - scale == 0.0;
            const double rho = usable ? (F - Fc) / scale : -1.0;
            if (usable && rho > 0.0) {
                double* t = cur; cur = cand; cand = t;
                F = Fc;
                const double g = 2.0 * rho - 1.0;
                double f = 1.0 - g * g * g;
                f = f < 2.0 / 3.0 ? f : 2.0 / 3.0;
                lambda *= f > 1.0 / 3.0 ? f : 1.0 / 3.0;
                ni = 2.0;
                accepted++;
                taken = true;
                if (int rc = s3g_linearize(ctx, G, cur, d_meas, d_info, huber, fix_scale, Hd, b, nullptr, &G.sc->cost)) return rc;
                break;
            }
            lambda *= ni;
            ni *= 2.0;
            if (!(lambda - lambda == 0.0)) stop = true;
        }
        if (!taken) break;                                                    // ten trials turned down: g2o gives up
    }
    SLAM_HIP(hipMemcpyAsync(d_out, cur, (size_t)V * 104, hipMemcpyDeviceToDevice, st));
    SLAM_HIP(hipStreamSynchronize(st));
    h_stats[0] = F0; h_stats[1] = F; h_stats[2] = accepted; h_stats[3] = trials; h_stats[4] = (double)cg_total; h_stats[5] = lambda;
    h_stats[6] = status; h_stats[7] = 0.0;
    return SLAM_OK;
}

static int s3g_optimize_checks(const char* who, slam_ctx* ctx, int64_t V, int64_t E, int64_t n_fixed, int iterations, double huber, double tol,
                               int max_iter) {
    if (int rc = s3g_common_checks(who, ctx, V, E)) return rc;
    SLAM_REQUIRE(iterations >= 0 && iterations <= 10000, "%s: iterations out of range [0, 10000]", who);
    SLAM_REQUIRE(huber >= 0.0 && tol > 0.0 && tol < 1.0 && max_iter >= 1 && max_iter <= (1 << 20),
                 "%s: huber_delta >= 0, 0 < pcg_tol < 1, pcg_max_iter in [1, 2^20]", who);
    SLAM_REQUIRE(V == 0 || (n_fixed >= 1 && n_fixed <= V), "%s: a graph needs at least one fixed vertex (n_fixed=%lld)", who, (long long)n_fixed);
    return SLAM_OK;
}

extern "C" int slam_s3g_optimize_f64(slam_ctx* ctx, int64_t V, int64_t E, const double* d_sims, const int32_t* d_edges, const double* d_meas,
                                     const double* d_info, const uint8_t* d_fixed, int64_t n_fixed, const int32_t* d_vtx_ptr,
                                     const int32_t* d_vtx_adj, int iterations, double huber_delta, double pcg_tol, int pcg_max_iter,
                                     int fix_scale, double* d_sims_out, double* h_stats) {
    if (int rc = s3g_optimize_checks("slam_s3g_optimize_f64", ctx, V, E, n_fixed, iterations, huber_delta, pcg_tol, pcg_max_iter)) return rc;
    SLAM_REQUIRE(h_stats, "slam_s3g_optimize_f64: null h_stats");
    for (int i = 0; i < 8; i++) h_stats[i] = 0.0;
    if (V == 0) return SLAM_OK;
    SLAM_REQUIRE(d_sims && d_sims_out && d_fixed && d_vtx_ptr && (E == 0 || (d_edges && d_meas && d_info && d_vtx_adj)),
                 "slam_s3g_optimize_f64: null device pointer");
    SLAM_HIP(hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> lk(ctx->call_mu);
    if (E == 0) {                                        // nothing pulls on any vertex
        SLAM_HIP(hipMemcpyAsync(d_sims_out, d_sims, (size_t)V * 104, hipMemcpyDeviceToDevice, ctx->stream));
        return SLAM_OK;
    }
    void* ws = nullptr;
    s3g_scal* hs = nullptr;
    if (int rc = s3g_blocks(ctx, V, E, &ws, &hs)) return rc;
    s3g_graph G;
    s3g_open(G, V, E, d_edges, d_vtx_ptr, d_vtx_adj, d_fixed, ws);
    if (int rc = s3g_setup(ctx, G, hs, "slam_s3g_optimize_f64", n_fixed)) return rc;
    return s3g_optimize_locked(ctx, G, d_sims, d_meas, d_info, iterations, huber_delta, pcg_tol, pcg_max_iter, fix_scale != 0, d_sims_out, h_stats, hs);
}

// slam_s3g_optimize_f64 on HOST buffers: one upload (the vertex lists are built here by a stable counting sort: the slots of a
// vertex in ascending edge order), the LM loop, one download.  Edges with an index outside [0, V) get no slot; the device
// check then refuses the call (SLAM_ERR_INVALID) and h_sims_out is not written.
extern "C" int slam_s3g_optimize_host_f64(slam_ctx* ctx, int64_t V, int64_t E, const double* h_sims, const int32_t* h_edges, const double* h_meas,
                                          const double* h_info, const uint8_t* h_fixed, int iterations, double huber_delta, double pcg_tol,
                                          int pcg_max_iter, int fix_scale, double* h_sims_out, double* h_stats) {
    SLAM_REQUIRE(ctx, "slam_s3g_optimize_host_f64: null ctx");
    SLAM_REQUIRE(V >= 0 && V <= SLAM_S3G_MAX_VERTICES && (V == 0 || h_fixed), "slam_s3g_optimize_host_f64: V out of range [0, 2^24] or null mask");
    int64_t n_fixed = 0;
    for (int64_t v = 0; v < V; v++) n_fixed += h_fixed[v] ? 1 : 0;
    if (int rc = s3g_optimize_checks("slam_s3g_optimize_host_f64", ctx, V, E, n_fixed, iterations, huber_delta, pcg_tol, pcg_max_iter)) return rc;
    SLAM_REQUIRE(h_stats, "slam_s3g_optimize_host_f64: null h_stats");
    for (int i = 0; i < 8; i++) h_stats[i] = 0.0;
    if (V == 0) return SLAM_OK;
    SLAM_REQUIRE(h_sims && h_sims_out && (E == 0 || (h_edges && h_meas && h_info)), "slam_s3g_optimize_host_f64: null host pointer");
    if (E == 0) { memmove(h_sims_out, h_sims, (size_t)V * 104); return SLAM_OK; }
    std::lock_guard<std::mutex> lk(ctx->call_mu);
    SLAM_HIP(hipSetDevice(ctx->device));
    const uint64_t o_scal = 0, o_sims = 256, o_edges = o_sims + s3g_up((uint64_t)V * 104), o_meas = o_edges + s3g_up((uint64_t)E * 8);
    const uint64_t o_info = o_meas + s3g_up((uint64_t)E * 104), o_fixed = o_info + s3g_up((uint64_t)E * 392), o_ptr = o_fixed + s3g_up((uint64_t)V);
    const uint64_t o_adj = o_ptr + s3g_up((uint64_t)(V + 1) * 4), o_out = o_adj + s3g_up((uint64_t)E * 8), total = o_out + s3g_up((uint64_t)V * 104);
    void *ws = nullptr, *dev = nullptr, *host = nullptr;
    if (int rc = slam_io_arena(ctx, total, total, &dev, &host)) return rc;
    if (int rc = slam_workspace(ctx, s3g_make_layout(V, E).total, &ws)) return rc;
    uint8_t *hb = (uint8_t*)host, *db = (uint8_t*)dev;
    memcpy(hb + o_sims, h_sims, (size_t)V * 104);
    memcpy(hb + o_edges, h_edges, (size_t)E * 8);
    memcpy(hb + o_meas, h_meas, (size_t)E * 104);
    memcpy(hb + o_info, h_info, (size_t)E * 392);
    memcpy(hb + o_fixed, h_fixed, (size_t)V);
    int32_t* ptr = (int32_t*)(hb + o_ptr);
    int32_t* adj = (int32_t*)(hb + o_adj);
    memset(ptr, 0, (size_t)(V + 1) * 4);
    memset(adj, 0xFF, (size_t)E * 8);
    for (int64_t a = 0; a < 2 * E; a++)
        if (h_edges[a] >= 0 && h_edges[a] < V) ptr[h_edges[a] + 1]++;
    for (int64_t v = 0; v < V; v++) ptr[v + 1] += ptr[v];
    {
        std::vector<int32_t> at(ptr, ptr + V);
        for (int64_t a = 0; a < 2 * E; a++)
            if (h_edges[a] >= 0 && h_edges[a] < V) adj[at[h_edges[a]]++] = (int32_t)a;
    }
    ctx->io_h2d_bytes += o_out - o_sims;
    ctx->io_d2h_bytes += (uint64_t)V * 104;
    SLAM_HIP(hipMemcpyAsync(db + o_sims, hb + o_sims, o_out - o_sims, hipMemcpyHostToDevice, ctx->stream));
    s3g_graph G;
    s3g_open(G, V, E, (const int32_t*)(db + o_edges), (const int32_t*)(db + o_ptr), (const int32_t*)(db + o_adj), db + o_fixed, ws);
    if (int rc = s3g_setup(ctx, G, (s3g_scal*)(hb + o_scal), "slam_s3g_optimize_host_f64", n_fixed)) return rc;
    if (int rc = s3g_optimize_locked(ctx, G, (const double*)(db + o_sims), (const double*)(db + o_meas), (const double*)(db + o_info), iterations,
                                     huber_delta, pcg_tol, pcg_max_iter, fix_scale != 0, (double*)(db + o_out), h_stats, (s3g_scal*)(hb + o_scal)))
        return rc;
    SLAM_HIP(hipMemcpyAsync(hb + o_out, db + o_out, (size_t)V * 104, hipMemcpyDeviceToHost, ctx->stream));
    SLAM_HIP(hipStreamSynchronize(ctx->stream));
    memcpy(h_sims_out, hb + o_out, (size_t)V * 104);
    return SLAM_OK;
}
#endif  // S3G_HOST_ONLY
