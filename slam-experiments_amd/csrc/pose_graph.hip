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
// Everything is f64 with floating-point contraction OFF: the cost of a candidate (pg_edge_kernel<false>) and the cost of the
// same poses once accepted (pg_edge_kernel<true>) must round identically, and a result must be a pure function of the inputs.
// There is no floating-point atomic: an edge writes its contributions to the SLOTS of its two ends (slot = position in the
// vertex -> edge CSR list, ascending edge index), a vertex adds its slots in list order, sums over the graph go through
// per-block partials added in a fixed order.  Integer atomics carry only order-free values (status bits, a maximum, counts).
//
// Storage per slot k of vertex v (k in [ptr[v], ptr[v+1]), adj[k] = 2 e + side, side 0: v is the edge's i, side 1: its j):
//   S[k]   36 doubles   the block that multiplies x of the OTHER end: w J_i^T Omega J_j for side 0, its transpose for side 1
//   D[k]   27 doubles   this end's share of H_vv (21, upper triangle by rows) and of b_v (6)
//   nbr[k] int32        the other end's vertex, or -1 when that vertex is fixed (its column has left the system)
// so the product walks S and nbr front to back per vertex: each W_e is read twice per product (576 B per edge), both times as
// part of a contiguous stream, never through an edge -> block indirection.
//
// Lane mapping of the product (and of the CG vector kernels): SIX lanes per vertex, lane (v, row) owns row `row` of every
// block of v and element `row` of y_v; a wave holds 10 vertices (60 of 64 lanes).  The six lanes of a vertex read the 288
// contiguous bytes of S[k] as six 48-byte rows (one coalesced request per slot instead of 18 scattered 16-byte ones with a
// lane per vertex), and all six load the same 48 bytes of x_u (one request, broadcast).  A lane per vertex would keep 36 + 6
// doubles of one block live per lane and leave a wave's 64 loads on 64 different lines; the six-lane form needs 12.  No DPP
// or LDS gather of x_u: the six identical addresses coalesce in the texture path and x (48 B per vertex) stays in L2.
// The slot loop is unrolled by four with the loads issued ahead of the arithmetic (fixed order of the additions); vertices
// above PG_HUB_DEG slots are handled by a whole wave each (ten slots in flight per step, the ten partial rows added in a
// fixed order through LDS), so a loop-closure hub of degree 1000 costs 100 steps of one wave, not 1000 of six lanes.
//
// The CG scalars never leave the device: every dot product is left as per-block partial sums, and every block of the NEXT
// kernel adds those partials itself in the same fixed order (at most PG_MAX_PART + PG_HUB_BLOCKS values), so alpha, beta
// and the stop decision are identical in all blocks with no hand-off inside a launch.  Three launches per iteration
// (product + p.q; x, r, z + r.z, r.r; p); once the residual meets the tolerance they return at their first instruction.
// The host reads the done flag every PG_CG_CHECK iterations, and the cost, gain denominator and status once per LM trial.
#include "internal.h"
#include <math.h>

#pragma clang fp contract(off)

#define PG_HD __device__ __forceinline__
#define PG_THREADS 256                       // vector kernels: 4 waves
#define PG_VPW 10                            // vertices per wave (six lanes each)
#define PG_VPB (PG_VPW * (PG_THREADS / 64))  // vertices per block and grid-stride step
#define PG_MAX_PART 512                      // partial sums per reduction (blocks of the vector kernels)
#define PG_HUB_DEG 128                       // more slots than this: the vertex is a hub (wave-per-vertex path)
#define PG_HUB_BLOCKS 16                     // extra blocks of the product kernel that walk the hub list
#define PG_CG_CHECK 32                       // CG iterations queued between two reads of the done flag
#define PG_ST_INDEX 1                        // status bits (SLAM_PG_STATUS_* of the header)
#define PG_ST_ANGLE 2
#define PG_ST_PRECOND 4
#define PG_ST_BREAKDOWN 8
#define PG_ST_NONFINITE 16

static_assert(SLAM_PG_MAX_VERTICES <= (1 << 24) && SLAM_PG_MAX_EDGES <= (1 << 25), "36 E, 2 E + 1 and 6 V fit int32");
static_assert(SLAM_PG_STATUS_INDEX == PG_ST_INDEX && SLAM_PG_STATUS_ANGLE == PG_ST_ANGLE && SLAM_PG_STATUS_PRECOND == PG_ST_PRECOND &&
              SLAM_PG_STATUS_BREAKDOWN == PG_ST_BREAKDOWN && SLAM_PG_STATUS_NONFINITE == PG_ST_NONFINITE, "header and kernel agree");

// device-side scalars of one call (first block of the workspace)
struct pg_scal {
    double cost, scale, bb, tol2bb, rr;
    unsigned long long maxdiag_bits;
    int status, done, iters, n_hub, n_fixed, pad;
};

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

// inverse of the SPD 6x6 A (full storage) by LDL^T, as po_solve of pose_opt.hip; false (and the identity) if not SPD
PG_HD bool pg_inverse6(const double* A, double* Inv) {
    double L[36], d[6], dinv[6];
    bool spd = true;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double v = A[j * 6 + j];
#pragma unroll
        for (int k = 0; k < j; k++) v -= L[j * 6 + k] * L[j * 6 + k] * d[k];
        spd = spd && (v > 0.0) && isfinite(v);
        d[j] = v;
        dinv[j] = 1.0 / v;
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double u = A[i * 6 + j];
#pragma unroll
            for (int k = 0; k < j; k++) u -= L[i * 6 + k] * L[j * 6 + k] * d[k];
            L[i * 6 + j] = u * dinv[j];
        }
    }
#pragma unroll
    for (int c = 0; c < 6; c++) {          // column c of the inverse; the lower triangle is mirrored from the upper one
        double y[6], x[6];
#pragma unroll
        for (int i = 0; i < 6; i++) {
            double v = (i == c) ? 1.0 : 0.0;
#pragma unroll
            for (int k = 0; k < i; k++) v -= L[i * 6 + k] * y[k];
            y[i] = v;
        }
#pragma unroll
        for (int i = 5; i >= 0; i--) {
            double v = y[i] * dinv[i];
#pragma unroll
            for (int k = i + 1; k < 6; k++) v -= L[k * 6 + i] * x[k];
            x[i] = v;
        }
#pragma unroll
        for (int i = 0; i < 6; i++)
            if (i <= c) { Inv[i * 6 + c] = spd ? x[i] : (i == c ? 1.0 : 0.0); Inv[c * 6 + i] = Inv[i * 6 + c]; }
    }
    return spd;
}

// ---- reductions ------------------------------------------------------------------------------------------------------------
// sum of v over the block in a fixed order (xor tree inside a wave, then the waves in ascending order); every thread gets it
__device__ __forceinline__ double pg_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ double pg_block_sum(double v, double* sh /*[PG_THREADS / 64]*/) {
    v = pg_wave_sum(v);
    __syncthreads();                                  // sh may still be read from an earlier call
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = sh[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); w++) s += sh[w];
    return s;
}
// sum of part[0..n), the same value in every thread of every block that asks
__device__ __forceinline__ double pg_sum_partials(const double* part, int n, double* sh) {
    double v = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) v += part[i];
    return pg_block_sum(v, sh);
}

// ---- set-up: index checks, neighbour table, edge -> slot table, hub list ------------------------------------------------------
__global__ void pg_check_edges_kernel(int V, int E, const int* __restrict__ edges, pg_scal* sc) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int i = edges[2 * e], j = edges[2 * e + 1];
    if (i < 0 || i >= V || j < 0 || j >= V || i == j) atomicOr(&sc->status, PG_ST_INDEX);
}
// one lane per vertex: its slots must name edges that have it at that end; writes nbr and slot_of (slot of (edge, side)).
// Nothing is read through an index that was not checked first: the edge check ran in the launch before this one.
__global__ void pg_setup_vertices_kernel(int V, int E, const int* __restrict__ edges, const int* __restrict__ ptr,
                                         const int* __restrict__ adj, const uint8_t* __restrict__ fixed, int* __restrict__ nbr,
                                         int* __restrict__ slot_of, pg_scal* sc) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    if (sc->status & PG_ST_INDEX) return;
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
    if (bad) atomicOr(&sc->status, PG_ST_INDEX);
}
// The hub list (vertices with more than PG_HUB_DEG slots) in ASCENDING VERTEX ORDER, by an ordered compaction: the product
// kernel deals hub h to wave h mod (waves of the hub blocks), and that wave's share of p.q is a sum over ITS hubs, so the
// list's order reaches the CG scalars - it has to be a function of the input, not of which lane finished first.
// count: hubs per block of PG_THREADS vertices; scan (one block): exclusive offsets and the total; fill: rank inside the
// block by ballot.  Only differences of ptr are read, no index is followed, so these run whatever the checks found.
__device__ __forceinline__ bool pg_is_hub(int V, const int* __restrict__ ptr, int v) { return v < V && ptr[v + 1] - ptr[v] > PG_HUB_DEG; }
__global__ __launch_bounds__(PG_THREADS) void pg_hub_count_kernel(int V, const int* __restrict__ ptr, int* __restrict__ hub_off) {
    const int n = __syncthreads_count(pg_is_hub(V, ptr, blockIdx.x * PG_THREADS + threadIdx.x));
    if (threadIdx.x == 0) hub_off[blockIdx.x] = n;
}
__global__ __launch_bounds__(PG_THREADS) void pg_hub_scan_kernel(int nblocks, int* __restrict__ hub_off, pg_scal* sc) {
    __shared__ int sh[PG_THREADS];
    const int per = (nblocks + PG_THREADS - 1) / PG_THREADS, lo = threadIdx.x * per, hi = min(lo + per, nblocks);
    int mine = 0;
    for (int i = lo; i < hi; i++) mine += hub_off[i];
    sh[threadIdx.x] = mine;
    __syncthreads();
    int before = 0;
    for (int t = 0; t < (int)threadIdx.x; t++) before += sh[t];
    for (int i = lo; i < hi; i++) { const int c = hub_off[i]; hub_off[i] = before; before += c; }
    if (threadIdx.x == PG_THREADS - 1) sc->n_hub = before;
}
__global__ __launch_bounds__(PG_THREADS) void pg_hub_fill_kernel(int V, const int* __restrict__ ptr, const int* __restrict__ hub_off,
                                                                 int* __restrict__ hubs) {
    __shared__ int wave_n[PG_THREADS / 64];
    const int v = blockIdx.x * PG_THREADS + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool hub = pg_is_hub(V, ptr, v);
    const unsigned long long m = __ballot(hub);
    if (lane == 0) wave_n[wave] = __popcll(m);
    __syncthreads();
    if (!hub) return;
    int rank = __popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; w++) rank += wave_n[w];
    hubs[hub_off[blockIdx.x] + rank] = v;
}

// every (edge, side) must have got exactly one slot (slot_of was filled with -1 before)
__global__ void pg_check_slots_kernel(int E, const int* __restrict__ adj, const int* __restrict__ slot_of, pg_scal* sc) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= 2 * E) return;
    if (sc->status & PG_ST_INDEX) return;
    const int k = slot_of[a];
    if (k < 0 || k >= 2 * E || adj[k] != a) atomicOr(&sc->status, PG_ST_INDEX);
}

// ---- linearisation: one edge per lane ------------------------------------------------------------------------------------------
// FULL: residual, Jacobians, blocks into the slots of both ends, optional edge-ordered copy of W_e.  !FULL: the robust cost only
// (the candidate of an LM trial).  part_cost[block] = the block's robust chi2 in a fixed order.
template <bool FULL>
__global__ __launch_bounds__(64) void pg_edge_kernel(int E, const double* __restrict__ poses, const int* __restrict__ edges,
                                                     const double* __restrict__ meas, const double* __restrict__ info,
                                                     const int* __restrict__ slot_of, double huber, double* __restrict__ S,
                                                     double* __restrict__ Dg, double* __restrict__ W_out,
                                                     double* __restrict__ part_cost, pg_scal* sc) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    double rho = 0.0;
    if (e < E) {
        const int vi = edges[2 * e], vj = edges[2 * e + 1];
        double Ti[12], Tj[12], Z[12], Tinv[12], A[12], Zinv[12], D[12];
#pragma unroll
        for (int q = 0; q < 12; q++) { Ti[q] = poses[12 * (size_t)vi + q]; Tj[q] = poses[12 * (size_t)vj + q]; Z[q] = meas[12 * (size_t)e + q]; }
        pg_inv(Ti, Tinv);
        pg_mul(Tj, Tinv, A);
        pg_inv(Z, Zinv);
        pg_mul(A, Zinv, D);
        double r[6], Jj[36];
        const bool ok = pg_log_jinv(D, r, Jj, FULL);
        const double* Om = info + 36 * (size_t)e;
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
        double w = 1.0;
        rho = chi2;
        if (huber > 0.0) {                               // as pose_opt.hip: rho' and rho of g2o's RobustKernelHuber
            const double en = sqrt(chi2);
            if (en > huber) { w = huber / en; rho = 2.0 * huber * en - huber * huber; }
        }
        // an edge that is reported leaves the sums: its cost is 0 and its blocks are finite zeros, by a select (0 * inf is NaN,
        // and one NaN block would reach every CG scalar)
        const bool live = ok && isfinite(rho);
        if (!live) { atomicOr(&sc->status, ok ? PG_ST_NONFINITE : PG_ST_ANGLE); rho = 0.0; w = 0.0; }
        if (FULL) {
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
            const int si = slot_of[2 * e], sj = slot_of[2 * e + 1];
            double* Si = S + 36 * (size_t)si; double* Sj = S + 36 * (size_t)sj;
            double* Di = Dg + 27 * (size_t)si; double* Dj = Dg + 27 * (size_t)sj;
#pragma unroll
            for (int a = 0; a < 6; a++)
#pragma unroll
                for (int b = 0; b < 6; b++) {
                    const double v = live ? w * pg_atb(Ji, OJj, a, b) : 0.0;       // W_e = w J_i^T Omega J_j
                    Si[a * 6 + b] = v;
                    Sj[b * 6 + a] = v;
                    if (W_out) W_out[36 * (size_t)e + a * 6 + b] = v;
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
    }
    rho = pg_wave_sum(rho);
    if (threadIdx.x == 0) part_cost[blockIdx.x] = rho;
}

// H_vv (full 6x6) and b_v: 32 lanes per vertex, lane t < 27 adds term t of the vertex's slots in list order
__global__ __launch_bounds__(PG_THREADS) void pg_gather_kernel(int V, const int* __restrict__ ptr, const double* __restrict__ Dg,
                                                               const uint8_t* __restrict__ fixed, double* __restrict__ Hd,
                                                               double* __restrict__ b, pg_scal* sc) {
    const int t = threadIdx.x & 31;
    const int v = blockIdx.x * (PG_THREADS / 32) + (threadIdx.x >> 5);
    if (v >= V || t >= 27) return;
    const int lo = ptr[v], hi = ptr[v + 1];
    double s = 0.0;
    int k = lo;
    for (; k + 4 <= hi; k += 4) {
        const double d0 = Dg[27 * (size_t)k + t], d1 = Dg[27 * (size_t)(k + 1) + t], d2 = Dg[27 * (size_t)(k + 2) + t],
                     d3 = Dg[27 * (size_t)(k + 3) + t];
        s += d0; s += d1; s += d2; s += d3;
    }
    for (; k < hi; k++) s += Dg[27 * (size_t)k + t];
    if (t >= 21) { b[6 * (size_t)v + t - 21] = s; return; }
    int a = 0, c = t;
    while (c >= 6 - a) { c -= 6 - a; a++; }
    c += a;
    Hd[36 * (size_t)v + a * 6 + c] = s;
    Hd[36 * (size_t)v + c * 6 + a] = s;
    if (a == c && !(fixed && fixed[v]) && s > 0.0)      // largest diagonal entry of the free system (lambda_0): order-free
        atomicMax(&sc->maxdiag_bits, (unsigned long long)__double_as_longlong(s));
}

// *out = sum of part[0..n) in a fixed order (one block)
__global__ __launch_bounds__(PG_THREADS) void pg_finish_kernel(const double* __restrict__ part, int n, double* out) {
    __shared__ double sh[PG_THREADS / 64];
    const double s = pg_sum_partials(part, n, sh);
    if (threadIdx.x == 0) *out = s;
}
__global__ __launch_bounds__(PG_THREADS) void pg_finish_bb_kernel(const double* __restrict__ part, int n, double tol, pg_scal* sc) {
    __shared__ double sh[PG_THREADS / 64];
    const double s = pg_sum_partials(part, n, sh);
    if (threadIdx.x == 0) {
        sc->bb = s; sc->rr = s; sc->tol2bb = tol * tol * s; sc->done = 0; sc->iters = 0;
        if (!isfinite(s)) atomicOr(&sc->status, PG_ST_NONFINITE);      // a right-hand side that is not finite: no iteration will run
    }
}

// edge-ordered W_e -> the slots of both ends (the hooks that are handed blocks instead of poses)
__global__ void pg_pack_kernel(int E, const double* __restrict__ W, const int* __restrict__ slot_of, double* __restrict__ S) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 36 * E) return;
    const int e = idx / 36, q = idx - 36 * e, a = q / 6, c = q - 6 * a;
    const double v = W[idx];
    S[36 * (size_t)slot_of[2 * e] + q] = v;
    S[36 * (size_t)slot_of[2 * e + 1] + c * 6 + a] = v;
}

// ---- the product -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double pg_row_dot(const double* __restrict__ m, const double* __restrict__ x) {
    const double2 m0 = *(const double2*)m, m1 = *(const double2*)(m + 2), m2 = *(const double2*)(m + 4);
    const double2 x0 = *(const double2*)x, x1 = *(const double2*)(x + 2), x2 = *(const double2*)(x + 4);
    return ((m0.x * x0.x + m0.y * x0.y) + (m1.x * x1.x + m1.y * x1.y)) + (m2.x * x2.x + m2.y * x2.y);
}
__device__ __forceinline__ double pg_slot_term(const double* __restrict__ S, const int* __restrict__ nbr, const double* __restrict__ x,
                                               int k, int row) {
    const int u = nbr[k];
    return u >= 0 ? pg_row_dot(S + 36 * (size_t)k + 6 * row, x + 6 * (size_t)u) : 0.0;
}
// row `row` of (H_vv + lambda I) x_v + sum over the slots [lo, hi) of v of S[k] x_nbr[k]
__device__ __forceinline__ double pg_vertex_row(int v, int row, const int* __restrict__ nbr, const double* __restrict__ S,
                                                const double* __restrict__ Hd, double lambda, const double* __restrict__ x, int lo,
                                                int hi) {
    double y = pg_row_dot(Hd + 36 * (size_t)v + 6 * row, x + 6 * (size_t)v) + lambda * x[6 * (size_t)v + row];
    int k = lo;
    for (; k + 4 <= hi; k += 4) {
        const double t0 = pg_slot_term(S, nbr, x, k, row), t1 = pg_slot_term(S, nbr, x, k + 1, row),
                     t2 = pg_slot_term(S, nbr, x, k + 2, row), t3 = pg_slot_term(S, nbr, x, k + 3, row);
        y += t0; y += t1; y += t2; y += t3;
    }
    for (; k < hi; k++) y += pg_slot_term(S, nbr, x, k, row);
    return y;
}
// a hub: the wave's ten lane groups take the slots lo + g, lo + g + 10, ...; the ten partial rows meet in LDS and are added
// in group order behind the diagonal term (all 64 lanes of the wave call this together)
__device__ __forceinline__ double pg_hub_row(int v, int g, int row, const int* __restrict__ nbr, const double* __restrict__ S,
                                             const double* __restrict__ Hd, double lambda, const double* __restrict__ x, int lo,
                                             int hi, volatile double* sh /*[64] of this wave*/) {
    double part = 0.0;
    if (g < PG_VPW)
        for (int k = lo + g; k < hi; k += PG_VPW) part += pg_slot_term(S, nbr, x, k, row);
    sh[threadIdx.x & 63] = part;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    double y = pg_row_dot(Hd + 36 * (size_t)v + 6 * row, x + 6 * (size_t)v) + lambda * x[6 * (size_t)v + row];
    for (int q = 0; q < PG_VPW; q++) y += sh[q * 6 + row];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    return y;
}

// MODE 0: y = A x.  MODE 1 (CG): q = A p and part[block] = the block's share of p.q; nothing once sc->done is set, which the
// kernel itself sets (block 0) when the residual of the iteration before met the tolerance.
template <int MODE>
__global__ __launch_bounds__(PG_THREADS) void pg_hmul_kernel(int V, int main_blocks, const int* __restrict__ ptr,
                                                             const int* __restrict__ nbr, const uint8_t* __restrict__ fixed,
                                                             const int* __restrict__ hubs, const double* __restrict__ S,
                                                             const double* __restrict__ Hd, double lambda,
                                                             const double* __restrict__ x, double* __restrict__ y,
                                                             double* __restrict__ part, pg_scal* sc) {
    __shared__ double sh[PG_THREADS];
    __shared__ double shw[PG_THREADS / 64];
    if (MODE == 1) {
        if (sc->done) return;
        if (!(sc->rr > sc->tol2bb)) {                  // converged (or not a number): this launch and all later ones are no-ops
            if (blockIdx.x == 0 && threadIdx.x == 0) sc->done = 1;
            return;
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane / 6, row = lane - 6 * g;
    double dot = 0.0;
    if ((int)blockIdx.x < main_blocks) {
        for (int base = blockIdx.x * PG_VPB; base < V; base += main_blocks * PG_VPB) {
            const int v = base + wave * PG_VPW + g;
            if (g >= PG_VPW || v >= V) continue;
            const int lo = ptr[v], hi = ptr[v + 1];
            if (hi - lo > PG_HUB_DEG) continue;        // a hub block writes it
            double r = 0.0;
            if (!fixed[v]) r = pg_vertex_row(v, row, nbr, S, Hd, lambda, x, lo, hi);
            y[6 * (size_t)v + row] = r;
            if (MODE == 1) dot += r * x[6 * (size_t)v + row];
        }
    } else {
        const int n_hub = sc->n_hub, waves = (gridDim.x - main_blocks) * (PG_THREADS / 64);
        for (int h = (blockIdx.x - main_blocks) * (PG_THREADS / 64) + wave; h < n_hub; h += waves) {
            const int v = hubs[h];
            const double r = fixed[v] ? 0.0 : pg_hub_row(v, g, row, nbr, S, Hd, lambda, x, ptr[v], ptr[v + 1], sh + 64 * wave);
            if (g == 0) {
                y[6 * (size_t)v + row] = r;
                if (MODE == 1) dot += r * x[6 * (size_t)v + row];
            }
        }
    }
    if (MODE == 1) {
        const double s = pg_block_sum(dot, shw);
        if (threadIdx.x == 0) part[blockIdx.x] = s;
    }
}

// ---- CG vector kernels (the product's six-lane mapping, `nblocks` blocks with a grid stride) ---------------------------------------
// Minv_v = (H_vv + lambda I)^-1, one lane per vertex
__global__ __launch_bounds__(64) void pg_precond_kernel(int V, const double* __restrict__ Hd, const uint8_t* __restrict__ fixed,
                                                        double lambda, double* __restrict__ Minv, pg_scal* sc) {
    const int v = blockIdx.x * 64 + threadIdx.x;
    if (v >= V) return;
    double A[36], Inv[36];
#pragma unroll
    for (int q = 0; q < 36; q++) A[q] = Hd[36 * (size_t)v + q] + ((q % 7 == 0) ? lambda : 0.0);
    if (!pg_inverse6(A, Inv) && !fixed[v]) atomicOr(&sc->status, PG_ST_PRECOND);
#pragma unroll
    for (int q = 0; q < 36; q++) Minv[36 * (size_t)v + q] = Inv[q];
}
// x = 0, r = -b (0 on fixed vertices), z = Minv r, p = z; partials of r.z (parity 0) and of b.b
__global__ __launch_bounds__(PG_THREADS) void pg_cg_init_kernel(int V, int nblocks, const uint8_t* __restrict__ fixed,
                                                                const double* __restrict__ b, const double* __restrict__ Minv,
                                                                double* __restrict__ x, double* __restrict__ r, double* __restrict__ z,
                                                                double* __restrict__ p, double* __restrict__ part_rz,
                                                                double* __restrict__ part_rr) {
    __shared__ double shw[PG_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane / 6, row = lane - 6 * g;
    double rz = 0.0, rr = 0.0;
    for (int base = blockIdx.x * PG_VPB; base < V; base += nblocks * PG_VPB) {
        const int v = base + wave * PG_VPW + g;
        if (g >= PG_VPW || v >= V) continue;
        const bool fx = fixed[v];
        double rv[6];
#pragma unroll
        for (int c = 0; c < 6; c++) rv[c] = fx ? 0.0 : -b[6 * (size_t)v + c];
        const double* M = Minv + 36 * (size_t)v + 6 * row;
        const double zr = fx ? 0.0 : ((M[0] * rv[0] + M[1] * rv[1]) + (M[2] * rv[2] + M[3] * rv[3])) + (M[4] * rv[4] + M[5] * rv[5]);
        const size_t o = 6 * (size_t)v + row;
        x[o] = 0.0; r[o] = rv[row]; z[o] = zr; p[o] = zr;
        rz += rv[row] * zr;
        rr += rv[row] * rv[row];
    }
    const double s0 = pg_block_sum(rz, shw), s1 = pg_block_sum(rr, shw);
    if (threadIdx.x == 0) { part_rz[blockIdx.x] = s0; part_rr[blockIdx.x] = s1; }
}
// alpha = r.z / p.q; x += alpha p; r -= alpha q (into r_out: the six lanes of a vertex all read r_v); z = Minv r; partials of the
// new r.z and r.r.  A p.q that is not positive ends the solve with the status bit (every block decides alike from the same sums).
__global__ __launch_bounds__(PG_THREADS) void pg_cg_update_kernel(int V, int nblocks, int hmul_blocks, const double* __restrict__ Minv,
                                                                  const double* __restrict__ p, const double* __restrict__ q,
                                                                  double* __restrict__ x, const double* __restrict__ r,
                                                                  double* __restrict__ r_out, double* __restrict__ z,
                                                                  const double* __restrict__ part_pq, const double* __restrict__ part_rz_old,
                                                                  double* __restrict__ part_rz_new, double* __restrict__ part_rr,
                                                                  pg_scal* sc) {
    __shared__ double shw[PG_THREADS / 64];
    if (sc->done) return;
    const double pq = pg_sum_partials(part_pq, hmul_blocks, shw), rz_old = pg_sum_partials(part_rz_old, nblocks, shw);
    if (!(pq > 0.0) || !isfinite(pq) || !isfinite(rz_old)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { atomicOr(&sc->status, PG_ST_BREAKDOWN); sc->done = 1; }
        return;
    }
    const double alpha = rz_old / pq;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane / 6, row = lane - 6 * g;
    double rz = 0.0, rr = 0.0;
    for (int base = blockIdx.x * PG_VPB; base < V; base += nblocks * PG_VPB) {
        const int v = base + wave * PG_VPW + g;
        if (g >= PG_VPW || v >= V) continue;
        double rv[6];
#pragma unroll
        for (int c = 0; c < 6; c++) rv[c] = r[6 * (size_t)v + c] - alpha * q[6 * (size_t)v + c];
        const double* M = Minv + 36 * (size_t)v + 6 * row;
        const double zr = ((M[0] * rv[0] + M[1] * rv[1]) + (M[2] * rv[2] + M[3] * rv[3])) + (M[4] * rv[4] + M[5] * rv[5]);
        const size_t o = 6 * (size_t)v + row;
        x[o] = x[o] + alpha * p[o];
        r_out[o] = rv[row];
        z[o] = zr;
        rz += rv[row] * zr;
        rr += rv[row] * rv[row];
    }
    const double s0 = pg_block_sum(rz, shw), s1 = pg_block_sum(rr, shw);
    if (threadIdx.x == 0) { part_rz_new[blockIdx.x] = s0; part_rr[blockIdx.x] = s1; }
}
// beta = r.z new / r.z old; p = z + beta p; block 0 publishes r.r and the iteration count (the next product kernel turns
// r.r into the done flag)
__global__ __launch_bounds__(PG_THREADS) void pg_cg_direction_kernel(int V, int nblocks, const double* __restrict__ z, double* __restrict__ p,
                                                                     const double* __restrict__ part_rz_old,
                                                                     const double* __restrict__ part_rz_new,
                                                                     const double* __restrict__ part_rr, pg_scal* sc) {
    __shared__ double shw[PG_THREADS / 64];
    if (sc->done) return;
    const double rz_old = pg_sum_partials(part_rz_old, nblocks, shw), rz_new = pg_sum_partials(part_rz_new, nblocks, shw);
    const double rr = pg_sum_partials(part_rr, nblocks, shw);
    const double beta = rz_new / rz_old;
    for (int i = blockIdx.x * PG_THREADS + threadIdx.x; i < 6 * V; i += nblocks * PG_THREADS) p[i] = z[i] + beta * p[i];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        sc->rr = rr;
        sc->iters = sc->iters + 1;
        if (!isfinite(rr) || !isfinite(beta)) atomicOr(&sc->status, PG_ST_NONFINITE);
    }
}
__global__ void pg_cg_close_kernel(pg_scal* sc) {      // behind the last queued iteration: the decision the next product would take
    if (!(sc->rr > sc->tol2bb)) sc->done = 1;
}

// candidate poses Exp(x_v) T_v (fixed ones copied), partials of the gain ratio's denominator x.(lambda x - b)
__global__ __launch_bounds__(PG_THREADS) void pg_candidate_kernel(int V, const double* __restrict__ poses, const uint8_t* __restrict__ fixed,
                                                                  const double* __restrict__ x, const double* __restrict__ b, double lambda,
                                                                  double* __restrict__ out, double* __restrict__ part_scale) {
    __shared__ double shw[PG_THREADS / 64];
    const int v = blockIdx.x * PG_THREADS + threadIdx.x;
    double sc = 0.0;
    if (v < V) {
        double T[12], Tn[12];
#pragma unroll
        for (int q = 0; q < 12; q++) T[q] = poses[12 * (size_t)v + q];
        if (fixed[v]) {
#pragma unroll
            for (int q = 0; q < 12; q++) out[12 * (size_t)v + q] = T[q];
        } else {
            double dx[6];
#pragma unroll
            for (int q = 0; q < 6; q++) { dx[q] = x[6 * (size_t)v + q]; sc += dx[q] * (lambda * dx[q] - b[6 * (size_t)v + q]); }
            pg_apply_update(dx, T, Tn);
#pragma unroll
            for (int q = 0; q < 12; q++) out[12 * (size_t)v + q] = Tn[q];
        }
    }
    const double s = pg_block_sum(sc, shw);
    if (threadIdx.x == 0) part_scale[blockIdx.x] = s;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
static inline uint64_t pg_up(uint64_t b) { return (b + 255) & ~(uint64_t)255; }
static inline int pg_vec_blocks(int64_t V) { int64_t n = (V + PG_VPB - 1) / PG_VPB; return (int)(n < 1 ? 1 : n > PG_MAX_PART ? PG_MAX_PART : n); }
static inline int pg_edge_blocks(int64_t E) { return (int)((E + 63) / 64); }
static inline int pg_cand_blocks(int64_t V) { return (int)((V + PG_THREADS - 1) / PG_THREADS); }

struct pg_layout {
    uint64_t scal, nbr, slot_of, hubs, hub_off, S, Dg, Hd, b, Minv, x, r, r2, z, p, q, part_cost, part_a, part_b, part_c, part_d, poses2, total;
};
static pg_layout pg_make_layout(int64_t V, int64_t E) {
    pg_layout L;
    uint64_t o = 0;
    const uint64_t v = (uint64_t)(V > 0 ? V : 1), e = (uint64_t)(E > 0 ? E : 1);
    auto take = [&](uint64_t bytes) { const uint64_t at = o; o += pg_up(bytes); return at; };
    L.scal = take(sizeof(pg_scal));
    L.nbr = take(2 * e * 4); L.slot_of = take(2 * e * 4); L.hubs = take(v * 4); L.hub_off = take((uint64_t)pg_cand_blocks((int64_t)v) * 4);
    L.S = take(2 * e * 36 * 8); L.Dg = take(2 * e * 27 * 8);
    L.Hd = take(v * 36 * 8); L.b = take(v * 6 * 8); L.Minv = take(v * 36 * 8);
    L.x = take(v * 48); L.r = take(v * 48); L.r2 = take(v * 48); L.z = take(v * 48); L.p = take(v * 48); L.q = take(v * 48);
    const int eb = pg_edge_blocks((int64_t)e), cb = pg_cand_blocks((int64_t)v);
    L.part_cost = take((uint64_t)(eb > cb ? eb : cb) * 8);
    const uint64_t pb = (uint64_t)(PG_MAX_PART + PG_HUB_BLOCKS) * 8;
    L.part_a = take(pb); L.part_b = take(pb); L.part_c = take(pb); L.part_d = take(pb);
    L.poses2 = take(2 * v * 96);
    L.total = o;
    return L;
}

static int pg_common_checks(const char* who, slam_ctx* ctx, int64_t V, int64_t E) {
    SLAM_REQUIRE(ctx, "%s: null ctx", who);
    SLAM_REQUIRE(V >= 0 && V <= SLAM_PG_MAX_VERTICES && E >= 0 && E <= SLAM_PG_MAX_EDGES, "%s: bad sizes (V=%lld, E=%lld; limits 2^24 and 2^25)", who,
                 (long long)V, (long long)E);
    SLAM_REQUIRE(E == 0 || V > 0, "%s: edges without vertices", who);
    return SLAM_OK;
}

extern "C" int slam_pg_workspace(int64_t V, int64_t E, uint64_t* bytes) {
    SLAM_REQUIRE(bytes, "slam_pg_workspace: null bytes");
    SLAM_REQUIRE(V >= 0 && V <= SLAM_PG_MAX_VERTICES && E >= 0 && E <= SLAM_PG_MAX_EDGES, "bad sizes (V=%lld, E=%lld)", (long long)V, (long long)E);
    *bytes = pg_make_layout(V, E).total;
    return SLAM_OK;
}

extern "C" int slam_pg_plan(int64_t V, int64_t E, int32_t* plan) {
    SLAM_REQUIRE(plan, "slam_pg_plan: null plan");
    SLAM_REQUIRE(V >= 0 && V <= SLAM_PG_MAX_VERTICES && E >= 0 && E <= SLAM_PG_MAX_EDGES, "bad sizes (V=%lld, E=%lld)", (long long)V, (long long)E);
    plan[0] = pg_vec_blocks(V);          // blocks of the product's main path and of the CG vector kernels (= partial sums per dot)
    plan[1] = PG_HUB_BLOCKS;             // extra blocks of the product kernel for the hub list
    plan[2] = PG_VPB;                    // vertices per block and grid-stride step (six lanes each)
    plan[3] = PG_HUB_DEG;                // a vertex with more slots than this takes the wave-per-vertex path
    plan[4] = pg_edge_blocks(E);         // blocks of the edge kernel (= partial sums of the cost)
    plan[5] = PG_CG_CHECK;               // CG iterations queued between two reads of the done flag
    plan[6] = 3;                         // launches per CG iteration
    plan[7] = 0;
    return SLAM_OK;
}

struct pg_graph {                        // device views of one call
    int V, E;
    const int *edges, *ptr, *adj;
    const uint8_t* fixed;
    uint8_t* ws;
    pg_layout L;
    pg_scal* sc;
    int vb;                              // blocks of the vector kernels
    template <class T> T* at(uint64_t off) const { return (T*)(ws + off); }
};

static void pg_open(pg_graph& G, int64_t V, int64_t E, const int32_t* d_edges, const int32_t* d_ptr, const int32_t* d_adj,
                    const uint8_t* d_fixed, void* ws) {
    G.V = (int)V; G.E = (int)E; G.edges = d_edges; G.ptr = d_ptr; G.adj = d_adj; G.fixed = d_fixed;
    G.L = pg_make_layout(V, E);
    G.ws = (uint8_t*)ws;
    G.sc = G.at<pg_scal>(G.L.scal);
    G.vb = pg_vec_blocks(V);
}

// checks and tables; reads the status back (ONE synchronisation per call, before any kernel follows an index)
static int pg_setup(slam_ctx* ctx, pg_graph& G, pg_scal* h_scal /*pinned*/, const char* who, int64_t n_fixed_claimed) {
    hipStream_t st = ctx->stream;
    SLAM_HIP(hipMemsetAsync(G.sc, 0, sizeof(pg_scal), st));
    if (G.E > 0) {
        SLAM_HIP(hipMemsetAsync(G.at<int>(G.L.slot_of), 0xFF, (size_t)2 * G.E * 4, st));
        pg_check_edges_kernel<<<(G.E + 255) / 256, 256, 0, st>>>(G.V, G.E, G.edges, G.sc);
    }
    pg_setup_vertices_kernel<<<(G.V + 255) / 256, 256, 0, st>>>(G.V, G.E, G.edges, G.ptr, G.adj, G.fixed, G.at<int>(G.L.nbr),
                                                                 G.at<int>(G.L.slot_of), G.sc);
    {
        const int hb = pg_cand_blocks(G.V);
        pg_hub_count_kernel<<<hb, PG_THREADS, 0, st>>>(G.V, G.ptr, G.at<int>(G.L.hub_off));
        pg_hub_scan_kernel<<<1, PG_THREADS, 0, st>>>(hb, G.at<int>(G.L.hub_off), G.sc);
        pg_hub_fill_kernel<<<hb, PG_THREADS, 0, st>>>(G.V, G.ptr, G.at<int>(G.L.hub_off), G.at<int>(G.L.hubs));
    }
    if (G.E > 0) pg_check_slots_kernel<<<(2 * G.E + 255) / 256, 256, 0, st>>>(G.E, G.adj, G.at<int>(G.L.slot_of), G.sc);
    SLAM_HIP(hipGetLastError());
    SLAM_HIP(hipMemcpyAsync(h_scal, G.sc, sizeof(pg_scal), hipMemcpyDeviceToHost, st));
    SLAM_HIP(hipStreamSynchronize(st));
    if (h_scal->status & PG_ST_INDEX)
        return slam_set_error(SLAM_ERR_INVALID, "%s: an edge index outside [0, V), a self-edge, or a vertex list that does not match the edges", who);
    if (n_fixed_claimed >= 0 && h_scal->n_fixed != n_fixed_claimed)
        return slam_set_error(SLAM_ERR_INVALID, "%s: n_fixed = %lld but the mask fixes %d vertices", who, (long long)n_fixed_claimed, h_scal->n_fixed);
    return SLAM_OK;
}

static int pg_linearize(slam_ctx* ctx, const pg_graph& G, const double* poses, const double* meas, const double* info, double huber,
                        double* Hd, double* b, double* W_out, double* d_cost) {
    hipStream_t st = ctx->stream;
    SLAM_HIP(hipMemsetAsync(&G.sc->maxdiag_bits, 0, 8, st));
    if (G.E > 0)
        pg_edge_kernel<true><<<pg_edge_blocks(G.E), 64, 0, st>>>(G.E, poses, G.edges, meas, info, G.at<int>(G.L.slot_of), huber, G.at<double>(G.L.S),
                                                                 G.at<double>(G.L.Dg), W_out, G.at<double>(G.L.part_cost), G.sc);
    pg_gather_kernel<<<(G.V + 7) / 8, PG_THREADS, 0, st>>>(G.V, G.ptr, G.at<double>(G.L.Dg), G.fixed, Hd, b, G.sc);
    pg_finish_kernel<<<1, PG_THREADS, 0, st>>>(G.at<double>(G.L.part_cost), pg_edge_blocks(G.E), d_cost);
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

static int pg_hmul(slam_ctx* ctx, const pg_graph& G, const double* Hd, double lambda, const double* x, double* y) {
    pg_hmul_kernel<0><<<G.vb + PG_HUB_BLOCKS, PG_THREADS, 0, ctx->stream>>>(G.V, G.vb, G.ptr, G.at<int>(G.L.nbr), G.fixed, G.at<int>(G.L.hubs),
                                                                           G.at<double>(G.L.S), Hd, lambda, x, y, nullptr, G.sc);
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

// (H + lambda I) x = -b: at most max_iter iterations of three launches each, the done flag read every PG_CG_CHECK iterations
static int pg_pcg(slam_ctx* ctx, const pg_graph& G, const double* Hd, const double* b, double lambda, double tol, int max_iter, double* x,
                  pg_scal* h_scal) {
    hipStream_t st = ctx->stream;
    double *Minv = G.at<double>(G.L.Minv), *z = G.at<double>(G.L.z), *p = G.at<double>(G.L.p), *q = G.at<double>(G.L.q);
    double* r[2] = {G.at<double>(G.L.r), G.at<double>(G.L.r2)};
    double *part_pq = G.at<double>(G.L.part_a), *part_rr = G.at<double>(G.L.part_b);
    double* part_rz[2] = {G.at<double>(G.L.part_c), G.at<double>(G.L.part_d)};
    const int hb = G.vb + PG_HUB_BLOCKS;
    pg_precond_kernel<<<(G.V + 63) / 64, 64, 0, st>>>(G.V, Hd, G.fixed, lambda, Minv, G.sc);
    pg_cg_init_kernel<<<G.vb, PG_THREADS, 0, st>>>(G.V, G.vb, G.fixed, b, Minv, x, r[0], z, p, part_rz[0], part_rr);
    pg_finish_bb_kernel<<<1, PG_THREADS, 0, st>>>(part_rr, G.vb, tol, G.sc);
    SLAM_HIP(hipGetLastError());
    for (int n = 0; n < max_iter; n++) {
        const int a = n & 1, c = a ^ 1;
        pg_hmul_kernel<1><<<hb, PG_THREADS, 0, st>>>(G.V, G.vb, G.ptr, G.at<int>(G.L.nbr), G.fixed, G.at<int>(G.L.hubs), G.at<double>(G.L.S), Hd,
                                                     lambda, p, q, part_pq, G.sc);
        pg_cg_update_kernel<<<G.vb, PG_THREADS, 0, st>>>(G.V, G.vb, hb, Minv, p, q, x, r[a], r[c], z, part_pq, part_rz[a], part_rz[c], part_rr, G.sc);
        pg_cg_direction_kernel<<<G.vb, PG_THREADS, 0, st>>>(G.V, G.vb, z, p, part_rz[a], part_rz[c], part_rr, G.sc);
        if ((n + 1) % PG_CG_CHECK == 0 && n + 1 < max_iter) {
            pg_cg_close_kernel<<<1, 1, 0, st>>>(G.sc);
            SLAM_HIP(hipGetLastError());
            SLAM_HIP(hipMemcpyAsync(h_scal, G.sc, sizeof(pg_scal), hipMemcpyDeviceToHost, st));
            SLAM_HIP(hipStreamSynchronize(st));
            if (h_scal->done) break;
        }
    }
    pg_cg_close_kernel<<<1, 1, 0, st>>>(G.sc);
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

// workspace + a pinned block for the scalars (call lock held)
static int pg_blocks(slam_ctx* ctx, int64_t V, int64_t E, void** ws, pg_scal** hs) {
    void *dev = nullptr, *host = nullptr;
    if (int rc = slam_io_arena(ctx, 0, 256, &dev, &host)) return rc;
    if (int rc = slam_workspace(ctx, pg_make_layout(V, E).total, ws)) return rc;
    *hs = (pg_scal*)host;
    return SLAM_OK;
}

extern "C" int slam_pg_linearize_f64(slam_ctx* ctx, int64_t V, int64_t E, const double* d_poses, const int32_t* d_edges, const double* d_meas,
                                     const double* d_info, const int32_t* d_vtx_ptr, const int32_t* d_vtx_adj, double huber_delta,
                                     double* d_cost, double* d_grad, double* d_Hdiag, double* d_W, int32_t* h_status) {
    if (int rc = pg_common_checks("slam_pg_linearize_f64", ctx, V, E)) return rc;
    SLAM_REQUIRE(huber_delta >= 0.0, "slam_pg_linearize_f64: huber_delta must not be negative");
    SLAM_REQUIRE(d_cost && h_status && (V == 0 || (d_vtx_ptr && d_poses && d_grad && d_Hdiag)) &&
                     (E == 0 || (d_edges && d_meas && d_info && d_vtx_adj && d_W)), "slam_pg_linearize_f64: null pointer");
    SLAM_HIP(hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> lk(ctx->call_mu);
    *h_status = 0;
    if (V == 0) { SLAM_HIP(hipMemsetAsync(d_cost, 0, 8, ctx->stream)); return SLAM_OK; }
    void* ws = nullptr;
    pg_scal* hs = nullptr;
    if (int rc = pg_blocks(ctx, V, E, &ws, &hs)) return rc;
    pg_graph G;
    pg_open(G, V, E, d_edges, d_vtx_ptr, d_vtx_adj, nullptr, ws);
    if (int rc = pg_setup(ctx, G, hs, "slam_pg_linearize_f64", -1)) return rc;
    if (int rc = pg_linearize(ctx, G, d_poses, d_meas, d_info, huber_delta, d_Hdiag, d_grad, d_W, d_cost)) return rc;
    SLAM_HIP(hipMemcpyAsync(hs, G.sc, sizeof(pg_scal), hipMemcpyDeviceToHost, ctx->stream));
    SLAM_HIP(hipStreamSynchronize(ctx->stream));
    *h_status = hs->status;
    return SLAM_OK;
}

extern "C" int slam_pg_hmul_f64(slam_ctx* ctx, int64_t V, int64_t E, const int32_t* d_edges, const int32_t* d_vtx_ptr, const int32_t* d_vtx_adj,
                                const uint8_t* d_fixed, const double* d_Hdiag, const double* d_W, double lambda, const double* d_x, double* d_y) {
    if (int rc = pg_common_checks("slam_pg_hmul_f64", ctx, V, E)) return rc;
    if (V == 0) return SLAM_OK;
    SLAM_REQUIRE(d_vtx_ptr && d_fixed && d_Hdiag && d_x && d_y && (E == 0 || (d_edges && d_vtx_adj && d_W)), "slam_pg_hmul_f64: null pointer");
    SLAM_REQUIRE((((uintptr_t)d_Hdiag | (uintptr_t)d_x) & 15) == 0, "slam_pg_hmul_f64: d_Hdiag / d_x must be 16-byte aligned");
    SLAM_HIP(hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> lk(ctx->call_mu);
    void* ws = nullptr;
    pg_scal* hs = nullptr;
    if (int rc = pg_blocks(ctx, V, E, &ws, &hs)) return rc;
    pg_graph G;
    pg_open(G, V, E, d_edges, d_vtx_ptr, d_vtx_adj, d_fixed, ws);
    if (int rc = pg_setup(ctx, G, hs, "slam_pg_hmul_f64", -1)) return rc;
    if (E > 0) pg_pack_kernel<<<(unsigned)((36 * E + 255) / 256), 256, 0, ctx->stream>>>((int)E, d_W, G.at<int>(G.L.slot_of), G.at<double>(G.L.S));
    return pg_hmul(ctx, G, d_Hdiag, lambda, d_x, d_y);
}

extern "C" int slam_pg_pcg_f64(slam_ctx* ctx, int64_t V, int64_t E, const int32_t* d_edges, const int32_t* d_vtx_ptr, const int32_t* d_vtx_adj,
                               const uint8_t* d_fixed, const double* d_Hdiag, const double* d_W, const double* d_b, double lambda, double tol,
                               int max_iter, double* d_x, double* h_stats) {
    if (int rc = pg_common_checks("slam_pg_pcg_f64", ctx, V, E)) return rc;
    SLAM_REQUIRE(h_stats, "slam_pg_pcg_f64: null h_stats");
    SLAM_REQUIRE(tol > 0.0 && tol < 1.0 && max_iter >= 1 && max_iter <= (1 << 20) && lambda >= 0.0,
                 "slam_pg_pcg_f64: 0 < tol < 1, lambda >= 0, max_iter in [1, 2^20]");
    for (int i = 0; i < 4; i++) h_stats[i] = 0.0;
    if (V == 0) return SLAM_OK;
    SLAM_REQUIRE(d_vtx_ptr && d_fixed && d_Hdiag && d_b && d_x && (E == 0 || (d_edges && d_vtx_adj && d_W)), "slam_pg_pcg_f64: null pointer");
    SLAM_REQUIRE((((uintptr_t)d_Hdiag | (uintptr_t)d_x) & 15) == 0, "slam_pg_pcg_f64: d_Hdiag / d_x must be 16-byte aligned");
    SLAM_HIP(hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> lk(ctx->call_mu);
    void* ws = nullptr;
    pg_scal* hs = nullptr;
    if (int rc = pg_blocks(ctx, V, E, &ws, &hs)) return rc;
    pg_graph G;
    pg_open(G, V, E, d_edges, d_vtx_ptr, d_vtx_adj, d_fixed, ws);
    if (int rc = pg_setup(ctx, G, hs, "slam_pg_pcg_f64", -1)) return rc;
    if (E > 0) pg_pack_kernel<<<(unsigned)((36 * E + 255) / 256), 256, 0, ctx->stream>>>((int)E, d_W, G.at<int>(G.L.slot_of), G.at<double>(G.L.S));
    if (int rc = pg_pcg(ctx, G, d_Hdiag, d_b, lambda, tol, max_iter, d_x, hs)) return rc;
    SLAM_HIP(hipMemcpyAsync(hs, G.sc, sizeof(pg_scal), hipMemcpyDeviceToHost, ctx->stream));
    SLAM_HIP(hipStreamSynchronize(ctx->stream));
    // converged = the tolerance was met by a finite residual; `done` is only the stop flag (breakdown and NaN set it too)
    h_stats[0] = hs->iters; h_stats[1] = (isfinite(hs->rr) && hs->rr <= hs->tol2bb) ? 1.0 : 0.0;
    h_stats[2] = hs->bb == 0.0 ? 0.0 : sqrt(hs->rr / hs->bb); h_stats[3] = hs->status;
    return SLAM_OK;
}

// the LM loop on a set-up graph (call lock held).  hs: pinned.  d_poses in -> d_out.
static int pg_optimize_locked(slam_ctx* ctx, pg_graph& G, const double* d_poses, const double* d_meas, const double* d_info, int iterations,
                              double huber, double tol, int max_iter, double* d_out, double* h_stats, pg_scal* hs) {
    hipStream_t st = ctx->stream;
    const int V = G.V;
    double* cur = G.at<double>(G.L.poses2);
    double* cand = cur + 12 * (size_t)V;
    double *Hd = G.at<double>(G.L.Hd), *b = G.at<double>(G.L.b), *x = G.at<double>(G.L.x);
    const int bad_state = PG_ST_ANGLE | PG_ST_NONFINITE;
    SLAM_HIP(hipMemcpyAsync(cur, d_poses, (size_t)V * 96, hipMemcpyDeviceToDevice, st));
    if (int rc = pg_linearize(ctx, G, cur, d_meas, d_info, huber, Hd, b, nullptr, &G.sc->cost)) return rc;
    SLAM_HIP(hipMemcpyAsync(hs, G.sc, sizeof(pg_scal), hipMemcpyDeviceToHost, st));
    SLAM_HIP(hipStreamSynchronize(st));
    double F = hs->cost, maxdiag;
    memcpy(&maxdiag, &hs->maxdiag_bits, 8);
    const double F0 = F;
    double lambda = 1e-5 * (maxdiag > 1e-12 ? maxdiag : 1e-12), ni = 2.0;      // tau * max diagonal (g2o, as pose_opt.hip)
    int status = hs->status, accepted = 0, trials = 0;
    long long cg_total = 0;
    bool stop = !(F - F == 0.0) || (status & bad_state) != 0;
    for (int it = 0; it < iterations && !stop; it++) {
        bool taken = false;
        for (int trial = 0; trial < 10 && !stop; trial++) {                   // maxTrialsAfterFailure
            // the bits of this trial alone: a candidate that is turned down leaves none behind
            SLAM_HIP(hipMemsetAsync(&G.sc->status, 0, 4, st));
            if (int rc = pg_pcg(ctx, G, Hd, b, lambda, tol, max_iter, x, hs)) return rc;
            pg_candidate_kernel<<<pg_cand_blocks(V), PG_THREADS, 0, st>>>(V, cur, G.fixed, x, b, lambda, cand, G.at<double>(G.L.part_cost));
            pg_finish_kernel<<<1, PG_THREADS, 0, st>>>(G.at<double>(G.L.part_cost), pg_cand_blocks(V), &G.sc->scale);
            pg_edge_kernel<false><<<pg_edge_blocks(G.E), 64, 0, st>>>(G.E, cand, G.edges, d_meas, d_info, nullptr, huber, nullptr, nullptr, nullptr,
                                                                      G.at<double>(G.L.part_cost), G.sc);
            pg_finish_kernel<<<1, PG_THREADS, 0, st>>>(G.at<double>(G.L.part_cost), pg_edge_blocks(G.E), &G.sc->cost);
            SLAM_HIP(hipGetLastError());
            SLAM_HIP(hipMemcpyAsync(hs, G.sc, sizeof(pg_scal), hipMemcpyDeviceToHost, st));
            SLAM_HIP(hipStreamSynchronize(st));
            trials++;
            cg_total += hs->iters;
            status |= hs->status & (PG_ST_PRECOND | PG_ST_BREAKDOWN);
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
                if (int rc = pg_linearize(ctx, G, cur, d_meas, d_info, huber, Hd, b, nullptr, &G.sc->cost)) return rc;
                break;
            }
            lambda *= ni;
            ni *= 2.0;
            if (!(lambda - lambda == 0.0)) stop = true;
        }
        if (!taken) break;                                                    // ten trials turned down: g2o gives up
    }
    SLAM_HIP(hipMemcpyAsync(d_out, cur, (size_t)V * 96, hipMemcpyDeviceToDevice, st));
    SLAM_HIP(hipStreamSynchronize(st));
    h_stats[0] = F0; h_stats[1] = F; h_stats[2] = accepted; h_stats[3] = trials; h_stats[4] = (double)cg_total; h_stats[5] = lambda;
    h_stats[6] = status; h_stats[7] = 0.0;
    return SLAM_OK;
}

static int pg_optimize_checks(const char* who, slam_ctx* ctx, int64_t V, int64_t E, int64_t n_fixed, int iterations, double huber, double tol,
                              int max_iter) {
    if (int rc = pg_common_checks(who, ctx, V, E)) return rc;
    SLAM_REQUIRE(iterations >= 0 && iterations <= 10000, "%s: iterations out of range [0, 10000]", who);
    SLAM_REQUIRE(huber >= 0.0 && tol > 0.0 && tol < 1.0 && max_iter >= 1 && max_iter <= (1 << 20),
                 "%s: huber_delta >= 0, 0 < pcg_tol < 1, pcg_max_iter in [1, 2^20]", who);
    SLAM_REQUIRE(V == 0 || (n_fixed >= 1 && n_fixed <= V), "%s: a graph needs at least one fixed vertex (n_fixed=%lld)", who, (long long)n_fixed);
    return SLAM_OK;
}

extern "C" int slam_pg_optimize_f64(slam_ctx* ctx, int64_t V, int64_t E, const double* d_poses, const int32_t* d_edges, const double* d_meas,
                                    const double* d_info, const uint8_t* d_fixed, int64_t n_fixed, const int32_t* d_vtx_ptr,
                                    const int32_t* d_vtx_adj, int iterations, double huber_delta, double pcg_tol, int pcg_max_iter,
                                    double* d_poses_out, double* h_stats) {
    if (int rc = pg_optimize_checks("slam_pg_optimize_f64", ctx, V, E, n_fixed, iterations, huber_delta, pcg_tol, pcg_max_iter)) return rc;
    SLAM_REQUIRE(h_stats, "slam_pg_optimize_f64: null h_stats");
    for (int i = 0; i < 8; i++) h_stats[i] = 0.0;
    if (V == 0) return SLAM_OK;
    SLAM_REQUIRE(d_poses && d_poses_out && d_fixed && d_vtx_ptr && (E == 0 || (d_edges && d_meas && d_info && d_vtx_adj)),
                 "slam_pg_optimize_f64: null device pointer");
    SLAM_HIP(hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> lk(ctx->call_mu);
    if (E == 0) {                                        // nothing pulls on any pose
        SLAM_HIP(hipMemcpyAsync(d_poses_out, d_poses, (size_t)V * 96, hipMemcpyDeviceToDevice, ctx->stream));
        return SLAM_OK;
    }
    void* ws = nullptr;
    pg_scal* hs = nullptr;
    if (int rc = pg_blocks(ctx, V, E, &ws, &hs)) return rc;
    pg_graph G;
    pg_open(G, V, E, d_edges, d_vtx_ptr, d_vtx_adj, d_fixed, ws);
    if (int rc = pg_setup(ctx, G, hs, "slam_pg_optimize_f64", n_fixed)) return rc;
    return pg_optimize_locked(ctx, G, d_poses, d_meas, d_info, iterations, huber_delta, pcg_tol, pcg_max_iter, d_poses_out, h_stats, hs);
}

// slam_pg_optimize_f64 on HOST buffers: one upload (the vertex lists are built here by a stable counting sort: the slots of a
// vertex in ascending edge order), the LM loop, one download.  Edges with an index outside [0, V) get no slot; the device
// check then refuses the call (SLAM_ERR_INVALID) and h_poses_out is not written.
extern "C" int slam_pg_optimize_host_f64(slam_ctx* ctx, int64_t V, int64_t E, const double* h_poses, const int32_t* h_edges, const double* h_meas,
                                         const double* h_info, const uint8_t* h_fixed, int iterations, double huber_delta, double pcg_tol,
                                         int pcg_max_iter, double* h_poses_out, double* h_stats) {
    SLAM_REQUIRE(ctx, "slam_pg_optimize_host_f64: null ctx");
    SLAM_REQUIRE(V >= 0 && V <= SLAM_PG_MAX_VERTICES && (V == 0 || h_fixed), "slam_pg_optimize_host_f64: V out of range [0, 2^24] or null mask");
    int64_t n_fixed = 0;
    for (int64_t v = 0; v < V; v++) n_fixed += h_fixed[v] ? 1 : 0;
    if (int rc = pg_optimize_checks("slam_pg_optimize_host_f64", ctx, V, E, n_fixed, iterations, huber_delta, pcg_tol, pcg_max_iter)) return rc;
    SLAM_REQUIRE(h_stats, "slam_pg_optimize_host_f64: null h_stats");
    for (int i = 0; i < 8; i++) h_stats[i] = 0.0;
    if (V == 0) return SLAM_OK;
    SLAM_REQUIRE(h_poses && h_poses_out && (E == 0 || (h_edges && h_meas && h_info)), "slam_pg_optimize_host_f64: null host pointer");
    if (E == 0) { memmove(h_poses_out, h_poses, (size_t)V * 96); return SLAM_OK; }
    std::lock_guard<std::mutex> lk(ctx->call_mu);
    SLAM_HIP(hipSetDevice(ctx->device));
    const uint64_t o_scal = 0, o_poses = 256, o_edges = o_poses + pg_up((uint64_t)V * 96), o_meas = o_edges + pg_up((uint64_t)E * 8);
    const uint64_t o_info = o_meas + pg_up((uint64_t)E * 96), o_fixed = o_info + pg_up((uint64_t)E * 288), o_ptr = o_fixed + pg_up((uint64_t)V);
    const uint64_t o_adj = o_ptr + pg_up((uint64_t)(V + 1) * 4), o_out = o_adj + pg_up((uint64_t)E * 8), total = o_out + pg_up((uint64_t)V * 96);
    void *ws = nullptr, *dev = nullptr, *host = nullptr;
    if (int rc = slam_io_arena(ctx, total, total, &dev, &host)) return rc;
    if (int rc = slam_workspace(ctx, pg_make_layout(V, E).total, &ws)) return rc;
    uint8_t *hb = (uint8_t*)host, *db = (uint8_t*)dev;
    memcpy(hb + o_poses, h_poses, (size_t)V * 96);
    memcpy(hb + o_edges, h_edges, (size_t)E * 8);
    memcpy(hb + o_meas, h_meas, (size_t)E * 96);
    memcpy(hb + o_info, h_info, (size_t)E * 288);
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
    ctx->io_h2d_bytes += o_out - o_poses;
    ctx->io_d2h_bytes += (uint64_t)V * 96;
    SLAM_HIP(hipMemcpyAsync(db + o_poses, hb + o_poses, o_out - o_poses, hipMemcpyHostToDevice, ctx->stream));
    pg_graph G;
    pg_open(G, V, E, (const int32_t*)(db + o_edges), (const int32_t*)(db + o_ptr), (const int32_t*)(db + o_adj), db + o_fixed, ws);
    if (int rc = pg_setup(ctx, G, (pg_scal*)(hb + o_scal), "slam_pg_optimize_host_f64", n_fixed)) return rc;
    if (int rc = pg_optimize_locked(ctx, G, (const double*)(db + o_poses), (const double*)(db + o_meas), (const double*)(db + o_info), iterations,
                                    huber_delta, pcg_tol, pcg_max_iter, (double*)(db + o_out), h_stats, (pg_scal*)(hb + o_scal)))
        return rc;
    SLAM_HIP(hipMemcpyAsync(hb + o_out, db + o_out, (size_t)V * 96, hipMemcpyDeviceToHost, ctx->stream));
    SLAM_HIP(hipStreamSynchronize(ctx->stream));
    memcpy(h_poses_out, hb + o_out, (size_t)V * 96);
    return SLAM_OK;
}
