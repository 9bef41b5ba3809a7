// pose_graph.hip — SE(3) pose-graph optimisation on gfx950: what the reference's pose_graph_sphere_example.py gets from g2o
// (VertexSE3 / EdgeSE3, vertex 0 fixed, 15 Levenberg-Marquardt iterations with BlockSolverSE3(LinearSolverEigenSE3()),
// pose_graph_sphere_example.py:7,24-30,45-57), with the sparse direct solver replaced by block-Jacobi PCG.
//
//   slam_pg_linearize_f64   residual, Jacobians, robust weight per edge; diagonal blocks and gradient per vertex
//   slam_pg_hmul_f64        y = (H + lambda I) x over the free vertices: the block-sparse 6x6 product (the hot path)
//   slam_pg_pcg_f64         conjugate gradients on (H + lambda I) x = -b, preconditioner (H_vv + lambda I)^-1
//   slam_pg_optimize_f64    the LM loop (g2o's schedule, as pose_opt.hip restates it), slam_pg_optimize_host_f64 on host buffers
//
// Conventions (include/slamhip.h has them in full): T = [R|t] row-major 3x4, X_cam = R X_world + t, tangent [w, v] rotation
// first, update T <- Exp(d) T.  Edge (i, j) measures Z ~ T_j T_i^-1, r = Log(T_j T_i^-1 Z^-1), F = sum rho(r^T Omega r),
// dr/dd_j = Jl^-1(r), dr/dd_i = -Jl^-1(r) Ad(T_j T_i^-1).  PARITY UNPINNED against g2o (absent here): its EdgeSE3 error is
// [translation, quaternion vector part] of the inverse of our argument; slamhip/pose_graph.py maps the files.
//
// This file holds the manifold: the group, the retraction, the logarithm with its Jacobian, one edge's linearisation, and how
// a 48-byte row of a 6x6 block is read.  The solver around them - slots, the product, PCG, the LM loop, the guarantees about
// rounding and order - is graph_lm.h, shared with sim3_graph.hip and instantiated at the end of this file with N = 6:
// six lanes per vertex, ten vertices per wave (60 of 64 lanes), 36-double slot blocks read as six 48-byte rows with three
// 16-byte loads each.  Everything is f64 with floating-point contraction OFF.
#include "graph_lm.h"
#include <math.h>

#pragma clang fp contract(off)

#define PG_HD __device__ __forceinline__

static_assert(SLAM_PG_STATUS_INDEX == GLM_ST_INDEX && SLAM_PG_STATUS_ANGLE == GLM_ST_ANGLE && SLAM_PG_STATUS_PRECOND == GLM_ST_PRECOND &&
              SLAM_PG_STATUS_BREAKDOWN == GLM_ST_BREAKDOWN && SLAM_PG_STATUS_NONFINITE == GLM_ST_NONFINITE, "header and kernel agree");

// ---- SE(3) -----------------------------------------------------------------------------------------------------------------
PG_HD void pg_inv(const double* T, double* o) {
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) o[i * 4 + j] = T[j * 4 + i];
        o[i * 4 + 3] = -(T[i] * T[3] + T[4 + i] * T[7] + T[8 + i] * T[11]);
    }
}
PG_HD void pg_mul(const double* A, const double* B, double* o) {
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 4; j++) o[i * 4 + j] = A[i * 4] * B[j] + A[i * 4 + 1] * B[4 + j] + A[i * 4 + 2] * B[8 + j];
        o[i * 4 + 3] += A[i * 4 + 3];
    }
}
PG_HD void pg_hat(const double* w, double* W) {
    W[0] = 0; W[1] = -w[2]; W[2] = w[1]; W[3] = w[2]; W[4] = 0; W[5] = -w[0]; W[6] = -w[1]; W[7] = w[0]; W[8] = 0;
}
PG_HD void pg_mm3(const double* A, const double* B, double* C) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}

// Exp(d) T (rotation first), the update of pose_opt.hip's po_apply_update with a series below 1e-4 rad
PG_HD void pg_apply_update(const double* dx, const double* T, double* Tn) {
    const double th2 = dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2], th = sqrt(th2);
    double a, b, c;  // sin(th)/th, (1-cos)/th^2, (th-sin)/th^3
    if (th < 1e-4) { a = 1.0 - th2 / 6.0; b = 0.5 - th2 / 24.0; c = 1.0 / 6.0 - th2 / 120.0; }
    else {
        const double sn = sin(th), cs = cos(th);
        a = sn / th; b = (1.0 - cs) / th2; c = (th - sn) / (th2 * th);
    }
    double W[9], W2[9], R[9], V[9];
    pg_hat(dx, W);
    pg_mm3(W, W, W2);
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const double I = (i % 4 == 0) ? 1.0 : 0.0;
        R[i] = I + a * W[i] + b * W2[i];
        V[i] = I + b * W[i] + c * W2[i];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 4; j++) Tn[i * 4 + j] = R[i * 3] * T[j] + R[i * 3 + 1] * T[4 + j] + R[i * 3 + 2] * T[8 + j];
        Tn[i * 4 + 3] += V[i * 3] * dx[3] + V[i * 3 + 1] * dx[4] + V[i * 3 + 2] * dx[5];
    }
}

// The coefficients of Jl^-1 and Q at angle th (th2 = th^2): k of Jso3^-1 = I - W/2 + k W^2, and Barfoot's c1..c3 of Q
// (State Estimation for Robotics, eq. 7.86).  Below 0.2 rad the closed forms cancel (c3 loses eps / th^5) and four-term
// series take over: their first neglected term is th^8 / 4.8e7 (k) or smaller, under 6e-14 at the switch.
PG_HD void pg_coeffs(double th2, double th, double* k, double* c1, double* c2, double* c3) {
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

// r = Log(D) in [w, v] and Jr = Jl^-1(r) (6x6 row-major).  Returns false when the angle is beyond 3.1 rad (outside the
// contract: the vector part of R vanishes at pi) or something is not finite; the outputs are finite zeros then.
PG_HD bool pg_log_jinv(const double* D, double* r, double* Jr, bool want_j) {
    const double s[3] = {0.5 * (D[9] - D[6]), 0.5 * (D[2] - D[8]), 0.5 * (D[4] - D[1])};
    const double cs = 0.5 * (D[0] + D[5] + D[10] - 1.0);
    const double sn2 = s[0] * s[0] + s[1] * s[1] + s[2] * s[2], sn = sqrt(sn2);
    double th = atan2(sn, cs);
    const bool ok = isfinite(th) && th <= 3.1 && isfinite(D[3]) && isfinite(D[7]) && isfinite(D[11]);
    if (!ok) th = 0.0;
    const double th2 = th * th;
    const double f = sn > 1e-4 ? th / sn : 1.0 + th2 * (1.0 / 6.0 + th2 * (7.0 / 360.0));   // th / sin(th)
    double k, c1, c2, c3;
    pg_coeffs(th2, th, &k, &c1, &c2, &c3);
    double W[9], W2[9], Ji[9];
#pragma unroll
    for (int i = 0; i < 3; i++) r[i] = ok ? f * s[i] : 0.0;
    pg_hat(r, W);
    pg_mm3(W, W, W2);
#pragma unroll
    for (int i = 0; i < 9; i++) Ji[i] = ((i % 4 == 0) ? 1.0 : 0.0) - 0.5 * W[i] + k * W2[i];
    const double t[3] = {ok ? D[3] : 0.0, ok ? D[7] : 0.0, ok ? D[11] : 0.0};
#pragma unroll
    for (int i = 0; i < 3; i++) r[3 + i] = Ji[i * 3] * t[0] + Ji[i * 3 + 1] * t[1] + Ji[i * 3 + 2] * t[2];
    if (!want_j) return ok;
    // Q = P/2 + c1 (WP + PW + WPW) + c2 (W2 P + P W2 - 3 WPW) + c3 (WPW2 + W2PW), P = hat(v)
    double P[9], WP[9], PW[9], WPW[9], W2P[9], PW2[9], WPW2[9], W2PW[9], Q[9], JQ[9], C[9];
    pg_hat(r + 3, P);
    pg_mm3(W, P, WP); pg_mm3(P, W, PW); pg_mm3(WP, W, WPW); pg_mm3(W2, P, W2P); pg_mm3(P, W2, PW2);
    pg_mm3(WP, W2, WPW2); pg_mm3(W2, PW, W2PW);
#pragma unroll
    for (int i = 0; i < 9; i++)
        Q[i] = 0.5 * P[i] + c1 * (WP[i] + PW[i] + WPW[i]) + c2 * (W2P[i] + PW2[i] - 3.0 * WPW[i]) + c3 * (WPW2[i] + W2PW[i]);
    pg_mm3(Ji, Q, JQ);
    pg_mm3(JQ, Ji, C);
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

// Ad([R|t]) = [[R, 0], [t^ R, R]]
PG_HD void pg_adjoint(const double* A, double* Ad) {
    const double t[3] = {A[3], A[7], A[11]};
    double R[9], Th[9], TR[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) R[i * 3 + j] = A[i * 4 + j];
    pg_hat(t, Th);
    pg_mm3(Th, R, TR);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            Ad[i * 6 + j] = R[i * 3 + j];
            Ad[i * 6 + 3 + j] = 0.0;
            Ad[(3 + i) * 6 + j] = TR[i * 3 + j];
            Ad[(3 + i) * 6 + 3 + j] = R[i * 3 + j];
        }
}

// 6x6 helpers (row-major): C = A B, (A^T B)[i][j]
PG_HD void pg_mm6(const double* A, const double* B, double* C) {
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 6; j++) {
            double v = A[i * 6] * B[j];
#pragma unroll
            for (int k = 1; k < 6; k++) v += A[i * 6 + k] * B[k * 6 + j];
            C[i * 6 + j] = v;
        }
}
PG_HD double pg_atb(const double* A, const double* B, int i, int j) {
    double v = A[i] * B[j];
#pragma unroll
    for (int k = 1; k < 6; k++) v += A[k * 6 + i] * B[k * 6 + j];
    return v;
}

// One edge.  Returns 0 for a live edge, else the status bit of the reason it left the sums: its cost is 0 and its blocks are
// finite zeros then, by a select (0 * inf is NaN, and one NaN block would reach every CG scalar).  FULL: W_e = w J_i^T Omega J_j
// into Wi [36] and its transpose into Wj [36], optionally into We [36]; Di / Dj [27] = each end's share of H_vv (21, upper
// triangle by rows) and of b (6).  !FULL: the robust cost only.  Omega J_i and Omega J_j are live together here (256 VGPR +
// 74 AGPR, no scratch); sim3_graph.hip orders its products differently to stay there with 7x7 blocks.
template <bool FULL>
PG_HD int pg_edge(const double* Ti, const double* Tj, const double* Z, const double* Om, double huber, double* rho_out, double* Wi,
                  double* Wj, double* We, double* Di, double* Dj) {
    double Tinv[12], A[12], Zinv[12], D[12];
    pg_inv(Ti, Tinv);
    pg_mul(Tj, Tinv, A);
    pg_inv(Z, Zinv);
    pg_mul(A, Zinv, D);
    double r[6], Jj[36];
    const bool ok = pg_log_jinv(D, r, Jj, FULL);
    double Or[6];
#pragma unroll
    for (int a = 0; a < 6; a++) {
        double v = Om[a * 6] * r[0];
#pragma unroll
        for (int b = 1; b < 6; b++) v += Om[a * 6 + b] * r[b];
        Or[a] = v;
    }
    double chi2 = r[0] * Or[0];
#pragma unroll
    for (int a = 1; a < 6; a++) chi2 += r[a] * Or[a];
    double w = 1.0, rho = chi2;
    if (huber > 0.0) {                               // as pose_opt.hip: rho' and rho of g2o's RobustKernelHuber
        const double en = sqrt(chi2);
        if (en > huber) { w = huber / en; rho = 2.0 * huber * en - huber * huber; }
    }
    const bool live = ok && isfinite(rho);
    const int why = live ? 0 : ok ? GLM_ST_NONFINITE : GLM_ST_ANGLE;
    if (!live) { rho = 0.0; w = 0.0; }
    *rho_out = rho;
    if (FULL) {
        // The residual and cost above, the Jacobians and blocks below: scheduled apart.  Left to interleave the two across
        // this line the compiler needs 84 AGPRs for 74 (the parent's kernel had a branch here, around its status atomic).
        __builtin_amdgcn_sched_barrier(0);
        double Ji[36], OJi[36], OJj[36];
        {
            double Ad[36];
            pg_adjoint(A, Ad);
            pg_mm6(Jj, Ad, Ji);
        }
#pragma unroll
        for (int q = 0; q < 36; q++) Ji[q] = -Ji[q];
        pg_mm6(Om, Ji, OJi);
        pg_mm6(Om, Jj, OJj);
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int b = 0; b < 6; b++) {
                const double v = live ? w * pg_atb(Ji, OJj, a, b) : 0.0;       // W_e = w J_i^T Omega J_j
                Wi[a * 6 + b] = v;
                Wj[b * 6 + a] = v;
                if (We) We[a * 6 + b] = v;
            }
        int t = 0;
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int b = a; b < 6; b++) {
                Di[t] = live ? w * pg_atb(Ji, OJi, a, b) : 0.0;
                Dj[t] = live ? w * pg_atb(Jj, OJj, a, b) : 0.0;
                t++;
            }
#pragma unroll
        for (int a = 0; a < 6; a++) {
            double gi = Ji[a] * Or[0], gj = Jj[a] * Or[0];
#pragma unroll
            for (int k = 1; k < 6; k++) { gi += Ji[k * 6 + a] * Or[k]; gj += Jj[k * 6 + a] * Or[k]; }
            Di[21 + a] = live ? w * gi : 0.0;
            Dj[21 + a] = live ? w * gj : 0.0;
        }
    }
    return why;
}

// ---- the solver of graph_lm.h on SE(3) ----------------------------------------------------------------------------------------
struct pg_se3 {
    static constexpr int N = 6, STATE = 12, MAX_VERTICES = SLAM_PG_MAX_VERTICES, MAX_EDGES = SLAM_PG_MAX_EDGES;
    static constexpr int BAD_STATE = GLM_ST_ANGLE | GLM_ST_NONFINITE;
    static constexpr bool DONE_ONCE_PER_BLOCK = false;
    // named, not wrapped: behind one more level of inlining the compiler schedules the edge kernels differently
    template <bool FULL> static constexpr auto edge = &pg_edge<FULL>;
    static constexpr auto apply_update = &pg_apply_update;
    // a 48-byte row and x_u [6] are 16-byte aligned: three 16-byte loads each
    static PG_HD double row_dot(const double* __restrict__ m, const double* __restrict__ x) {
        const double2 m0 = *(const double2*)m, m1 = *(const double2*)(m + 2), m2 = *(const double2*)(m + 4);
        const double2 x0 = *(const double2*)x, x1 = *(const double2*)(x + 2), x2 = *(const double2*)(x + 4);
        return ((m0.x * x0.x + m0.y * x0.y) + (m1.x * x1.x + m1.y * x1.y)) + (m2.x * x2.x + m2.y * x2.y);
    }
    static PG_HD double minv_dot(const double* m, const double* r) {
        return ((m[0] * r[0] + m[1] * r[1]) + (m[2] * r[2] + m[3] * r[3])) + (m[4] * r[4] + m[5] * r[5]);
    }
};

extern "C" int slam_pg_workspace(int64_t V, int64_t E, uint64_t* bytes) { return glm_workspace<pg_se3>("slam_pg_workspace", V, E, bytes); }

extern "C" int slam_pg_plan(int64_t V, int64_t E, int32_t* plan) { return glm_plan<pg_se3>("slam_pg_plan", V, E, plan); }

extern "C" int slam_pg_linearize_f64(slam_ctx* ctx, int64_t V, int64_t E, const double* d_poses, const int32_t* d_edges, const double* d_meas,
                                     const double* d_info, const int32_t* d_vtx_ptr, const int32_t* d_vtx_adj, double huber_delta,
                                     double* d_cost, double* d_grad, double* d_Hdiag, double* d_W, int32_t* h_status) {
    if (int rc = glm_common_checks<pg_se3>("slam_pg_linearize_f64", ctx, V, E)) return rc;
    SLAM_REQUIRE(huber_delta >= 0.0, "slam_pg_linearize_f64: huber_delta must not be negative");
    SLAM_REQUIRE(d_cost && h_status && (V == 0 || (d_vtx_ptr && d_poses && d_grad && d_Hdiag)) &&
                     (E == 0 || (d_edges && d_meas && d_info && d_vtx_adj && d_W)), "slam_pg_linearize_f64: null pointer");
    return glm_linearize_call<pg_se3>("slam_pg_linearize_f64", ctx, V, E, d_poses, d_edges, d_meas, d_info, d_vtx_ptr, d_vtx_adj, huber_delta,
                                      d_cost, d_grad, d_Hdiag, d_W, h_status);
}

extern "C" int slam_pg_hmul_f64(slam_ctx* ctx, int64_t V, int64_t E, const int32_t* d_edges, const int32_t* d_vtx_ptr, const int32_t* d_vtx_adj,
                                const uint8_t* d_fixed, const double* d_Hdiag, const double* d_W, double lambda, const double* d_x, double* d_y) {
    if (int rc = glm_common_checks<pg_se3>("slam_pg_hmul_f64", ctx, V, E)) return rc;
    if (V == 0) return SLAM_OK;
    SLAM_REQUIRE(d_vtx_ptr && d_fixed && d_Hdiag && d_x && d_y && (E == 0 || (d_edges && d_vtx_adj && d_W)), "slam_pg_hmul_f64: null pointer");
    SLAM_REQUIRE((((uintptr_t)d_Hdiag | (uintptr_t)d_x) & 15) == 0, "slam_pg_hmul_f64: d_Hdiag / d_x must be 16-byte aligned");
    return glm_hmul_call<pg_se3>("slam_pg_hmul_f64", ctx, V, E, d_edges, d_vtx_ptr, d_vtx_adj, d_fixed, d_Hdiag, d_W, lambda, d_x, d_y);
}

extern "C" int slam_pg_pcg_f64(slam_ctx* ctx, int64_t V, int64_t E, const int32_t* d_edges, const int32_t* d_vtx_ptr, const int32_t* d_vtx_adj,
                               const uint8_t* d_fixed, const double* d_Hdiag, const double* d_W, const double* d_b, double lambda, double tol,
                               int max_iter, double* d_x, double* h_stats) {
    if (int rc = glm_common_checks<pg_se3>("slam_pg_pcg_f64", ctx, V, E)) return rc;
    SLAM_REQUIRE(h_stats, "slam_pg_pcg_f64: null h_stats");
    SLAM_REQUIRE(tol > 0.0 && tol < 1.0 && max_iter >= 1 && max_iter <= (1 << 20) && lambda >= 0.0,
                 "slam_pg_pcg_f64: 0 < tol < 1, lambda >= 0, max_iter in [1, 2^20]");
    for (int i = 0; i < 4; i++) h_stats[i] = 0.0;
    if (V == 0) return SLAM_OK;
    SLAM_REQUIRE(d_vtx_ptr && d_fixed && d_Hdiag && d_b && d_x && (E == 0 || (d_edges && d_vtx_adj && d_W)), "slam_pg_pcg_f64: null pointer");
    SLAM_REQUIRE((((uintptr_t)d_Hdiag | (uintptr_t)d_x) & 15) == 0, "slam_pg_pcg_f64: d_Hdiag / d_x must be 16-byte aligned");
    return glm_pcg_call<pg_se3>("slam_pg_pcg_f64", ctx, V, E, d_edges, d_vtx_ptr, d_vtx_adj, d_fixed, d_Hdiag, d_W, d_b, lambda, tol, max_iter, d_x,
                                h_stats);
}

extern "C" int slam_pg_optimize_f64(slam_ctx* ctx, int64_t V, int64_t E, const double* d_poses, const int32_t* d_edges, const double* d_meas,
                                    const double* d_info, const uint8_t* d_fixed, int64_t n_fixed, const int32_t* d_vtx_ptr,
                                    const int32_t* d_vtx_adj, int iterations, double huber_delta, double pcg_tol, int pcg_max_iter,
                                    double* d_poses_out, double* h_stats) {
    if (int rc = glm_optimize_checks<pg_se3>("slam_pg_optimize_f64", ctx, V, E, n_fixed, iterations, huber_delta, pcg_tol, pcg_max_iter)) return rc;
    SLAM_REQUIRE(h_stats, "slam_pg_optimize_f64: null h_stats");
    for (int i = 0; i < 8; i++) h_stats[i] = 0.0;
    if (V == 0) return SLAM_OK;
    SLAM_REQUIRE(d_poses && d_poses_out && d_fixed && d_vtx_ptr && (E == 0 || (d_edges && d_meas && d_info && d_vtx_adj)),
                 "slam_pg_optimize_f64: null device pointer");
    return glm_optimize_call<pg_se3>("slam_pg_optimize_f64", ctx, V, E, d_poses, d_edges, d_meas, d_info, d_fixed, n_fixed, d_vtx_ptr, d_vtx_adj,
                                     iterations, huber_delta, pcg_tol, pcg_max_iter, d_poses_out, h_stats);
}

// slam_pg_optimize_f64 on HOST buffers (the vertex lists are built on the way up)
extern "C" int slam_pg_optimize_host_f64(slam_ctx* ctx, int64_t V, int64_t E, const double* h_poses, const int32_t* h_edges, const double* h_meas,
                                         const double* h_info, const uint8_t* h_fixed, int iterations, double huber_delta, double pcg_tol,
                                         int pcg_max_iter, double* h_poses_out, double* h_stats) {
    SLAM_REQUIRE(ctx, "slam_pg_optimize_host_f64: null ctx");
    SLAM_REQUIRE(V >= 0 && V <= SLAM_PG_MAX_VERTICES && (V == 0 || h_fixed), "slam_pg_optimize_host_f64: V out of range [0, 2^24] or null mask");
    int64_t n_fixed = 0;
    for (int64_t v = 0; v < V; v++) n_fixed += h_fixed[v] ? 1 : 0;
    if (int rc = glm_optimize_checks<pg_se3>("slam_pg_optimize_host_f64", ctx, V, E, n_fixed, iterations, huber_delta, pcg_tol, pcg_max_iter))
        return rc;
    SLAM_REQUIRE(h_stats, "slam_pg_optimize_host_f64: null h_stats");
    for (int i = 0; i < 8; i++) h_stats[i] = 0.0;
    if (V == 0) return SLAM_OK;
    SLAM_REQUIRE(h_poses && h_poses_out && (E == 0 || (h_edges && h_meas && h_info)), "slam_pg_optimize_host_f64: null host pointer");
    return glm_optimize_host_call<pg_se3>("slam_pg_optimize_host_f64", ctx, V, E, h_poses, h_edges, h_meas, h_info, h_fixed, n_fixed, iterations,
                                          huber_delta, pcg_tol, pcg_max_iter, h_poses_out, h_stats);
}
