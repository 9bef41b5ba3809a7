// sim3_graph.hip — Sim(3) pose-graph optimisation on gfx950: ORB-SLAM's OptimizeEssentialGraph (7-DoF loop closing) for this
// project's conventions, the consumer of slam_sim3_* models.
//
//   slam_s3g_linearize_f64   residual, Jacobians, robust weight per edge; diagonal blocks and gradient per vertex
//   slam_s3g_hmul_f64        y = (H + lambda I) x over the free vertices: the block-sparse 7x7 product (the hot path)
//   slam_s3g_pcg_f64         conjugate gradients on (H + lambda I) x = -b, preconditioner (H_vv + lambda I)^-1
//   slam_s3g_optimize_f64    the LM loop (g2o's schedule), slam_s3g_optimize_host_f64 on host buffers
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
// This file holds the manifold: the group, the chart, one edge's linearisation, and how a packed 56-byte row of a 7x7 block
// is read.  The solver around them - slots, the product, PCG, the LM loop, the guarantees about rounding and order - is
// graph_lm.h, shared with pose_graph.hip and instantiated at the end of this file with N = 7: seven lanes per vertex, nine
// vertices per wave (63 of 64 lanes).  A 7x7 row is 56 bytes, so alternate rows are not 16-byte aligned: rows are read with
// 8-byte loads from PACKED 49-double slots.  The padded alternative (7x8 slots, 64-byte rows read as four 16-byte loads, 14 %
// more bytes) was built behind a compile-time switch, measured 6 % slower per CG iteration on the 10^5-vertex scene
//  and deleted.
//
// The edge routine: the SE(3) one already sits at 256 VGPR + 74 AGPR.  Here the three 7x7 products are ordered so that at most
// three 49-double matrices are live (J_j, J_i and one Omega J): W_e and the j share from Omega J_j first, then Omega J_i
// for the i share.  Registers and scratch per kernel: profiles/sim3_graph_resources.txt.
#ifndef S3G_HOST_ONLY                // a host build of the per-edge routines alone (the test suite's twin) defines it
#include "graph_lm.h"
#endif
#include "ldlt_inverse.h"
#include <math.h>
#include <stdint.h>

#pragma clang fp contract(off)

#ifdef S3G_HOST_ONLY
#define S3G_HD inline
#else
#define S3G_HD __device__ __forceinline__
#endif
#define S3G_ST_ANGLE 2                        // the status bits an edge can raise (SLAM_S3G_STATUS_* of the header)
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

// inverse of the SPD 7x7 A by LDL^T under the name the host twin calls (the solver uses ldlt_inverse<N> itself)
S3G_HD bool s3g_inverse7(const double* A, double* Inv) { return ldlt_inverse<7>(A, Inv); }

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
// ---- the solver of graph_lm.h on Sim(3) ---------------------------------------------------------------------------------------
static_assert(SLAM_S3G_STATUS_INDEX == GLM_ST_INDEX && SLAM_S3G_STATUS_ANGLE == GLM_ST_ANGLE && SLAM_S3G_STATUS_PRECOND == GLM_ST_PRECOND &&
              SLAM_S3G_STATUS_BREAKDOWN == GLM_ST_BREAKDOWN && SLAM_S3G_STATUS_NONFINITE == GLM_ST_NONFINITE &&
              S3G_ST_ANGLE == GLM_ST_ANGLE && S3G_ST_NONFINITE == GLM_ST_NONFINITE && SLAM_S3G_STATUS_SCALE == S3G_ST_SCALE,
              "header and kernel agree");

struct s3g_sim3 {
    static constexpr int N = 7, STATE = 13, MAX_VERTICES = SLAM_S3G_MAX_VERTICES, MAX_EDGES = SLAM_S3G_MAX_EDGES;
    static constexpr int BAD_STATE = S3G_ST_ANGLE | S3G_ST_NONFINITE | S3G_ST_SCALE;
    static constexpr bool DONE_ONCE_PER_BLOCK = true;
    // named, not wrapped: behind one more level of inlining the compiler schedules the edge kernels differently
    template <bool FULL> static constexpr auto edge = &s3g_edge<FULL>;
    static constexpr auto apply_update = &s3g_apply_update;
    // one packed row of seven doubles (8-byte loads: alternate 56-byte rows are not 16-byte aligned) times x_u [7]; the
    // additions in one stated order
    static S3G_HD double row_dot(const double* __restrict__ m, const double* __restrict__ x) {
        return ((m[0] * x[0] + m[1] * x[1]) + (m[2] * x[2] + m[3] * x[3])) + ((m[4] * x[4] + m[5] * x[5]) + m[6] * x[6]);
    }
    static S3G_HD double minv_dot(const double* __restrict__ m, const double* __restrict__ r) { return row_dot(m, r); }
};

extern "C" int slam_s3g_workspace(int64_t V, int64_t E, uint64_t* bytes) { return glm_workspace<s3g_sim3>("slam_s3g_workspace", V, E, bytes); }

extern "C" int slam_s3g_plan(int64_t V, int64_t E, int32_t* plan) {
    if (int rc = glm_plan<s3g_sim3>("slam_s3g_plan", V, E, plan)) return rc;
    plan[7] = s3g_sim3::N;               // doubles per stored row of a slot block (packed)
    return SLAM_OK;
}

extern "C" int slam_s3g_linearize_f64(slam_ctx* ctx, int64_t V, int64_t E, const double* d_sims, const int32_t* d_edges, const double* d_meas,
                                      const double* d_info, const int32_t* d_vtx_ptr, const int32_t* d_vtx_adj, double huber_delta,
                                      double* d_cost, double* d_grad, double* d_Hdiag, double* d_W, int32_t* h_status) {
    if (int rc = glm_common_checks<s3g_sim3>("slam_s3g_linearize_f64", ctx, V, E)) return rc;
    SLAM_REQUIRE(huber_delta >= 0.0, "slam_s3g_linearize_f64: huber_delta must not be negative");
    SLAM_REQUIRE(d_cost && h_status && (V == 0 || (d_vtx_ptr && d_sims && d_grad && d_Hdiag)) &&
                     (E == 0 || (d_edges && d_meas && d_info && d_vtx_adj && d_W)), "slam_s3g_linearize_f64: null pointer");
    return glm_linearize_call<s3g_sim3>("slam_s3g_linearize_f64", ctx, V, E, d_sims, d_edges, d_meas, d_info, d_vtx_ptr, d_vtx_adj, huber_delta,
                                        d_cost, d_grad, d_Hdiag, d_W, h_status, 0);
}

extern "C" int slam_s3g_hmul_f64(slam_ctx* ctx, int64_t V, int64_t E, const int32_t* d_edges, const int32_t* d_vtx_ptr, const int32_t* d_vtx_adj,
                                 const uint8_t* d_fixed, const double* d_Hdiag, const double* d_W, double lambda, const double* d_x, double* d_y) {
    if (int rc = glm_common_checks<s3g_sim3>("slam_s3g_hmul_f64", ctx, V, E)) return rc;
    if (V == 0) return SLAM_OK;
    SLAM_REQUIRE(d_vtx_ptr && d_fixed && d_Hdiag && d_x && d_y && (E == 0 || (d_edges && d_vtx_adj && d_W)), "slam_s3g_hmul_f64: null pointer");
    return glm_hmul_call<s3g_sim3>("slam_s3g_hmul_f64", ctx, V, E, d_edges, d_vtx_ptr, d_vtx_adj, d_fixed, d_Hdiag, d_W, lambda, d_x, d_y);
}

extern "C" int slam_s3g_pcg_f64(slam_ctx* ctx, int64_t V, int64_t E, const int32_t* d_edges, const int32_t* d_vtx_ptr, const int32_t* d_vtx_adj,
                                const uint8_t* d_fixed, const double* d_Hdiag, const double* d_W, const double* d_b, double lambda, double tol,
                                int max_iter, double* d_x, double* h_stats) {
    if (int rc = glm_common_checks<s3g_sim3>("slam_s3g_pcg_f64", ctx, V, E)) return rc;
    SLAM_REQUIRE(h_stats, "slam_s3g_pcg_f64: null h_stats");
    SLAM_REQUIRE(tol > 0.0 && tol < 1.0 && max_iter >= 1 && max_iter <= (1 << 20) && lambda >= 0.0,
                 "slam_s3g_pcg_f64: 0 < tol < 1, lambda >= 0, max_iter in [1, 2^20]");
    for (int i = 0; i < 4; i++) h_stats[i] = 0.0;
    if (V == 0) return SLAM_OK;
    SLAM_REQUIRE(d_vtx_ptr && d_fixed && d_Hdiag && d_b && d_x && (E == 0 || (d_edges && d_vtx_adj && d_W)), "slam_s3g_pcg_f64: null pointer");
    return glm_pcg_call<s3g_sim3>("slam_s3g_pcg_f64", ctx, V, E, d_edges, d_vtx_ptr, d_vtx_adj, d_fixed, d_Hdiag, d_W, d_b, lambda, tol, max_iter,
                                  d_x, h_stats);
}

extern "C" int slam_s3g_optimize_f64(slam_ctx* ctx, int64_t V, int64_t E, const double* d_sims, const int32_t* d_edges, const double* d_meas,
                                     const double* d_info, const uint8_t* d_fixed, int64_t n_fixed, const int32_t* d_vtx_ptr,
                                     const int32_t* d_vtx_adj, int iterations, double huber_delta, double pcg_tol, int pcg_max_iter,
                                     int fix_scale, double* d_sims_out, double* h_stats) {
    if (int rc = glm_optimize_checks<s3g_sim3>("slam_s3g_optimize_f64", ctx, V, E, n_fixed, iterations, huber_delta, pcg_tol, pcg_max_iter))
        return rc;
    SLAM_REQUIRE(h_stats, "slam_s3g_optimize_f64: null h_stats");
    for (int i = 0; i < 8; i++) h_stats[i] = 0.0;
    if (V == 0) return SLAM_OK;
    SLAM_REQUIRE(d_sims && d_sims_out && d_fixed && d_vtx_ptr && (E == 0 || (d_edges && d_meas && d_info && d_vtx_adj)),
                 "slam_s3g_optimize_f64: null device pointer");
    return glm_optimize_call<s3g_sim3>("slam_s3g_optimize_f64", ctx, V, E, d_sims, d_edges, d_meas, d_info, d_fixed, n_fixed, d_vtx_ptr, d_vtx_adj,
                                       iterations, huber_delta, pcg_tol, pcg_max_iter, d_sims_out, h_stats, (int)(fix_scale != 0));
}

// slam_s3g_optimize_f64 on HOST buffers (the vertex lists are built on the way up)
extern "C" int slam_s3g_optimize_host_f64(slam_ctx* ctx, int64_t V, int64_t E, const double* h_sims, const int32_t* h_edges, const double* h_meas,
                                          const double* h_info, const uint8_t* h_fixed, int iterations, double huber_delta, double pcg_tol,
                                          int pcg_max_iter, int fix_scale, double* h_sims_out, double* h_stats) {
    SLAM_REQUIRE(ctx, "slam_s3g_optimize_host_f64: null ctx");
    SLAM_REQUIRE(V >= 0 && V <= SLAM_S3G_MAX_VERTICES && (V == 0 || h_fixed), "slam_s3g_optimize_host_f64: V out of range [0, 2^24] or null mask");
    int64_t n_fixed = 0;
    for (int64_t v = 0; v < V; v++) n_fixed += h_fixed[v] ? 1 : 0;
    if (int rc = glm_optimize_checks<s3g_sim3>("slam_s3g_optimize_host_f64", ctx, V, E, n_fixed, iterations, huber_delta, pcg_tol, pcg_max_iter))
        return rc;
    SLAM_REQUIRE(h_stats, "slam_s3g_optimize_host_f64: null h_stats");
    for (int i = 0; i < 8; i++) h_stats[i] = 0.0;
    if (V == 0) return SLAM_OK;
    SLAM_REQUIRE(h_sims && h_sims_out && (E == 0 || (h_edges && h_meas && h_info)), "slam_s3g_optimize_host_f64: null host pointer");
    return glm_optimize_host_call<s3g_sim3>("slam_s3g_optimize_host_f64", ctx, V, E, h_sims, h_edges, h_meas, h_info, h_fixed, n_fixed, iterations,
                                            huber_delta, pcg_tol, pcg_max_iter, h_sims_out, h_stats, (int)(fix_scale != 0));
}
#endif  // S3G_HOST_ONLY
