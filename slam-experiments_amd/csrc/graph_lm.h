// graph_lm.h — the pose-graph solver of pose_graph.hip (SE(3), 6-DoF) and sim3_graph.hip (Sim(3), 7-DoF), once: block-sparse
// Levenberg-Marquardt with block-Jacobi PCG, generic in the tangent dimension N.  Each of the two files defines a traits type
// M for its manifold and instantiates everything here with it; the kernels are templates on M, so the two translation units
// of the one shared object get distinct symbols.
//
// M supplies:
//   N, STATE              tangent dimension (6 | 7), doubles per stored vertex and measurement (12 | 13)
//   MAX_VERTICES, MAX_EDGES, BAD_STATE (the status bits of a candidate that cannot be used), DONE_ONCE_PER_BLOCK (see cg_update)
//   edge<FULL>(Si, Sj, Z, Om, huber, opts..., &rho, Wi, Wj, We, Di, Dj) -> 0 or the status bit of the reason the edge left the sums.
//                         opts: what the manifold's edge routine takes beside the graph (nothing | int fix_scale); the calls
//                         below hand them through to the edge kernel's arguments as a pack.
//                         FULL: W_e = w J_i^T Omega J_j into Wi [N*N], its transpose into Wj, optionally into We; Di / Dj
//                         [N(N+1)/2 + N] = each end's share of H_vv (upper triangle by rows) and of b.  !FULL: the cost only.
//                         The traits NAME the manifold's force-inlined routine (static constexpr auto edge = &f<FULL>)
//                         and do not wrap it: one more level of inlining changes how the compiler schedules the kernel.
//   apply_update(d, S, Sn)   the retraction, named the same way
//   row_dot(m, x)         one stored row of a block times x_u [N], both in global memory, the additions in one stated order
//   minv_dot(m, r)        the same for a row of Minv and a residual held in registers
//
// Guarantees: f64 with floating-point contraction OFF: the cost of a candidate (edge<false>) and the cost of the same vertices
// once accepted (edge<true>) must round identically, and a result must be a pure function of the inputs.  There is no
// floating-point atomic: an edge writes its contributions to the SLOTS of its two ends (slot = position in the vertex -> edge
// CSR list, ascending edge index), a vertex adds its slots in list order, sums over the graph go through per-block partials
// added in a fixed order.  Integer atomics carry only order-free values (status bits, a maximum, counts).  Plain C++ and
// vector stores only.
//
// Storage per slot k of vertex v (k in [ptr[v], ptr[v+1]), adj[k] = 2 e + side, side 0: v is the edge's i, side 1: its j):
//   S[k]   N*N doubles          the block that multiplies x of the OTHER end: W_e for side 0, its transpose for side 1
//   D[k]   N(N+1)/2 + N doubles this end's share of H_vv (upper triangle by rows) and of b_v
//   nbr[k] int32                the other end's vertex, or -1 when that vertex is fixed (its column has left the system)
// so the product walks S and nbr front to back per vertex: each W_e is read twice per product, both times as part of a
// contiguous stream, never through an edge -> block indirection.
//
// Lane mapping of the product (and of the CG vector kernels): N lanes per vertex, lane (v, row) owns row `row` of every block
// of v and element `row` of y_v; a wave holds VPW = 64 / N vertices (60 or 63 of 64 lanes), a block 4 VPW.  The N lanes of a
// vertex read the contiguous bytes of S[k] as N rows (one coalesced request per slot), and all N load the same x_u (one
// request, broadcast).  No DPP or LDS gather of x_u: the identical addresses coalesce in the texture path and x stays in L2.
// The slot loop is unrolled by four with the loads issued ahead of the arithmetic (fixed order of the additions); vertices
// above GLM_HUB_DEG slots are handled by a whole wave each (VPW slots in flight per step, the VPW partial rows added in a
// fixed order through LDS), so a loop-closure hub of degree 1000 costs 100 steps of one wave, not 1000 of N lanes.
//
// The CG scalars never leave the device: every dot product is left as per-block partial sums, and every block of the NEXT
// kernel adds those partials itself in the same fixed order (at most GLM_MAX_PART + GLM_HUB_BLOCKS values), so alpha, beta
// and the stop decision are identical in all blocks with no hand-off inside a launch.  Three launches per iteration
// (product + p.q; x, r, z + r.z, r.r; p); once the residual meets the tolerance they return at their first instruction.
// The host reads the done flag every GLM_CG_CHECK iterations, and the cost, gain denominator and status once per LM trial.
#pragma once
#include "internal.h"
#include "ldlt_inverse.h"
#include <math.h>

#pragma clang fp contract(off)

#define GLM_THREADS 256                       // vector kernels: 4 waves
#define GLM_MAX_PART 512                      // partial sums per reduction (blocks of the vector kernels)
#define GLM_HUB_DEG 128                       // more slots than this: the vertex is a hub (wave-per-vertex path)
#define GLM_HUB_BLOCKS 16                     // extra blocks of the product kernel that walk the hub list
#define GLM_CG_CHECK 32                       // CG iterations queued between two reads of the done flag
#define GLM_ST_INDEX 1                        // status bits the two manifolds share (SLAM_PG_STATUS_* = SLAM_S3G_STATUS_*)
#define GLM_ST_ANGLE 2
#define GLM_ST_PRECOND 4
#define GLM_ST_BREAKDOWN 8
#define GLM_ST_NONFINITE 16

// the sizes that follow from M::N
template <class M>
struct glm_dims {
    static constexpr int N = M::N, NN = N * N, STATE = M::STATE;
    static constexpr int TRI = N * (N + 1) / 2, DSLOT = TRI + N;         // a slot's share of H_vv and of b
    static constexpr int VPW = 64 / N;                                    // vertices per wave (N lanes each)
    static constexpr int VPB = VPW * (GLM_THREADS / 64);                  // vertices per block and grid-stride step
    static constexpr int GATHER_LANES = DSLOT <= 32 ? 32 : 64;            // lanes per vertex of the gather kernel
    static_assert(M::MAX_VERTICES <= (1 << 24) && M::MAX_EDGES <= (1 << 25), "N*N E, 2 E + 1 and N V fit int32");
};

// device-side scalars of one call (first block of the workspace)
struct glm_scal {
    double cost, scale, bb, tol2bb, rr;
    unsigned long long maxdiag_bits;
    int status, done, iters, n_hub, n_fixed, pad;
};

// ---- reductions ------------------------------------------------------------------------------------------------------------
// sum of v over the block in a fixed order (xor tree inside a wave, then the waves in ascending order); every thread gets it
__device__ __forceinline__ double glm_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ double glm_block_sum(double v, double* sh /*[GLM_THREADS / 64]*/) {
    v = glm_wave_sum(v);
    __syncthreads();                                  // sh may still be read from an earlier call
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = sh[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); w++) s += sh[w];
    return s;
}
// sum of part[0..n), the same value in every thread of every block that asks
__device__ __forceinline__ double glm_sum_partials(const double* part, int n, double* sh) {
    double v = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) v += part[i];
    return glm_block_sum(v, sh);
}

// ---- set-up: index checks, neighbour table, edge -> slot table, hub list ------------------------------------------------------
template <class M>
__global__ void glm_check_edges_kernel(int V, int E, const int* __restrict__ edges, glm_scal* sc) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int i = edges[2 * e], j = edges[2 * e + 1];
    if (i < 0 || i >= V || j < 0 || j >= V || i == j) atomicOr(&sc->status, GLM_ST_INDEX);
}
// one lane per vertex: its slots must name edges that have it at that end; writes nbr and slot_of (slot of (edge, side)).
// Nothing is read through an index that was not checked first: the edge check ran in the launch before this one.
template <class M>
__global__ void glm_setup_vertices_kernel(int V, int E, const int* __restrict__ edges, const int* __restrict__ ptr,
                                          const int* __restrict__ adj, const uint8_t* __restrict__ fixed, int* __restrict__ nbr,
                                          int* __restrict__ slot_of, glm_scal* sc) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    if (sc->status & GLM_ST_INDEX) return;
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
    if (bad) atomicOr(&sc->status, GLM_ST_INDEX);
}
// The hub list (vertices with more than GLM_HUB_DEG slots) in ASCENDING VERTEX ORDER, by an ordered compaction: the product
// kernel deals hub h to wave h mod (waves of the hub blocks), and that wave's share of p.q is a sum over ITS hubs, so the
// list's order reaches the CG scalars - it has to be a function of the input, not of which lane finished first.
// count: hubs per block of GLM_THREADS vertices; scan (one block): exclusive offsets and the total; fill: rank inside the
// block by ballot.  Only differences of ptr are read, no index is followed, so these run whatever the checks found.
__device__ __forceinline__ bool glm_is_hub(int V, const int* __restrict__ ptr, int v) { return v < V && ptr[v + 1] - ptr[v] > GLM_HUB_DEG; }
template <class M>
__global__ __launch_bounds__(GLM_THREADS) void glm_hub_count_kernel(int V, const int* __restrict__ ptr, int* __restrict__ hub_off) {
    const int n = __syncthreads_count(glm_is_hub(V, ptr, blockIdx.x * GLM_THREADS + threadIdx.x));
    if (threadIdx.x == 0) hub_off[blockIdx.x] = n;
}
template <class M>
__global__ __launch_bounds__(GLM_THREADS) void glm_hub_scan_kernel(int nblocks, int* __restrict__ hub_off, glm_scal* sc) {
    __shared__ int sh[GLM_THREADS];
    const int per = (nblocks + GLM_THREADS - 1) / GLM_THREADS, lo = threadIdx.x * per, hi = min(lo + per, nblocks);
    int mine = 0;
    for (int i = lo; i < hi; i++) mine += hub_off[i];
    sh[threadIdx.x] = mine;
    __syncthreads();
    int before = 0;
    for (int t = 0; t < (int)threadIdx.x; t++) before += sh[t];
    for (int i = lo; i < hi; i++) { const int c = hub_off[i]; hub_off[i] = before; before += c; }
    if (threadIdx.x == GLM_THREADS - 1) sc->n_hub = before;
}
template <class M>
__global__ __launch_bounds__(GLM_THREADS) void glm_hub_fill_kernel(int V, const int* __restrict__ ptr, const int* __restrict__ hub_off,
                                                                   int* __restrict__ hubs) {
    __shared__ int wave_n[GLM_THREADS / 64];
    const int v = blockIdx.x * GLM_THREADS + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool hub = glm_is_hub(V, ptr, v);
    const unsigned long long m = __ballot(hub);
    if (lane == 0) wave_n[wave] = __popcll(m);
    __syncthreads();
    if (!hub) return;
    int rank = __popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; w++) rank += wave_n[w];
    hubs[hub_off[blockIdx.x] + rank] = v;
}
// every (edge, side) must have got exactly one slot (slot_of was filled with -1 before)
template <class M>
__global__ void glm_check_slots_kernel(int E, const int* __restrict__ adj, const int* __restrict__ slot_of, glm_scal* sc) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= 2 * E) return;
    if (sc->status & GLM_ST_INDEX) return;
    const int k = slot_of[a];
    if (k < 0 || k >= 2 * E || adj[k] != a) atomicOr(&sc->status, GLM_ST_INDEX);
}

// ---- linearisation: one edge per lane ------------------------------------------------------------------------------------------
// FULL: residual, Jacobians, blocks into the slots of both ends, optional edge-ordered copy of W_e.  !FULL: the robust cost only
// (the candidate of an LM trial).  An edge that M::edge reports leaves the sums (cost 0, finite zero blocks) and its reason
// joins the status word.  part_cost[block] = the block's robust chi2 in a fixed order.
template <class M, bool FULL, class... X>
__global__ __launch_bounds__(64) void glm_edge_kernel(int E, const double* __restrict__ states, const int* __restrict__ edges,
                                                      const double* __restrict__ meas, const double* __restrict__ info,
                                                      const int* __restrict__ slot_of, double huber, X... opts,
                                                      double* __restrict__ S, double* __restrict__ Dg, double* __restrict__ W_out,
                                                      double* __restrict__ part_cost, glm_scal* sc) {
    using D = glm_dims<M>;
    const int e = blockIdx.x * 64 + threadIdx.x;
    double rho = 0.0;
    if (e < E) {
        const int vi = edges[2 * e], vj = edges[2 * e + 1];
        double Si[D::STATE], Sj[D::STATE], Z[D::STATE];
#pragma unroll
        for (int q = 0; q < D::STATE; q++) {
            Si[q] = states[D::STATE * (size_t)vi + q]; Sj[q] = states[D::STATE * (size_t)vj + q]; Z[q] = meas[D::STATE * (size_t)e + q];
        }
        const double* Om = info + D::NN * (size_t)e;
        int why;
        if (FULL) {
            const int si = slot_of[2 * e], sj = slot_of[2 * e + 1];
            double* Pi = S + D::NN * (size_t)si; double* Pj = S + D::NN * (size_t)sj;
            why = M::template edge<true>(Si, Sj, Z, Om, huber, opts..., &rho, Pi, Pj, W_out ? W_out + D::NN * (size_t)e : nullptr,
                                         Dg + D::DSLOT * (size_t)si, Dg + D::DSLOT * (size_t)sj);
        } else {
            why = M::template edge<false>(Si, Sj, Z, Om, huber, opts..., &rho, nullptr, nullptr, nullptr, nullptr, nullptr);
        }
        if (why) atomicOr(&sc->status, why);
    }
    rho = glm_wave_sum(rho);
    if (threadIdx.x == 0) part_cost[blockIdx.x] = rho;
}

// H_vv (full NxN) and b_v: GATHER_LANES lanes per vertex, lane t < DSLOT adds term t of the vertex's slots in list order
template <class M>
__global__ __launch_bounds__(GLM_THREADS) void glm_gather_kernel(int V, const int* __restrict__ ptr, const double* __restrict__ Dg,
                                                                 const uint8_t* __restrict__ fixed, double* __restrict__ Hd,
                                                                 double* __restrict__ b, glm_scal* sc) {
    using D = glm_dims<M>;
    constexpr int N = D::N;
    const int t = threadIdx.x & (D::GATHER_LANES - 1);
    const int v = blockIdx.x * (GLM_THREADS / D::GATHER_LANES) + (threadIdx.x / D::GATHER_LANES);
    if (v >= V || t >= D::DSLOT) return;
    const int lo = ptr[v], hi = ptr[v + 1];
    double s = 0.0;
    int k = lo;
    for (; k + 4 <= hi; k += 4) {
        const double d0 = Dg[D::DSLOT * (size_t)k + t], d1 = Dg[D::DSLOT * (size_t)(k + 1) + t], d2 = Dg[D::DSLOT * (size_t)(k + 2) + t],
                     d3 = Dg[D::DSLOT * (size_t)(k + 3) + t];
        s += d0; s += d1; s += d2; s += d3;
    }
    for (; k < hi; k++) s += Dg[D::DSLOT * (size_t)k + t];
    if (t >= D::TRI) { b[N * (size_t)v + t - D::TRI] = s; return; }
    int a = 0, c = t;
    while (c >= N - a) { c -= N - a; a++; }
    c += a;
    Hd[D::NN * (size_t)v + a * N + c] = s;
    Hd[D::NN * (size_t)v + c * N + a] = s;
    if (a == c && !(fixed && fixed[v]) && s > 0.0)      // largest diagonal entry of the free system (lambda_0): order-free
        atomicMax(&sc->maxdiag_bits, (unsigned long long)__double_as_longlong(s));
}

// *out = sum of part[0..n) in a fixed order (one block)
template <class M>
__global__ __launch_bounds__(GLM_THREADS) void glm_finish_kernel(const double* __restrict__ part, int n, double* out) {
    __shared__ double sh[GLM_THREADS / 64];
    const double s = glm_sum_partials(part, n, sh);
    if (threadIdx.x == 0) *out = s;
}
template <class M>
__global__ __launch_bounds__(GLM_THREADS) void glm_finish_bb_kernel(const double* __restrict__ part, int n, double tol, glm_scal* sc) {
    __shared__ double sh[GLM_THREADS / 64];
    const double s = glm_sum_partials(part, n, sh);
    if (threadIdx.x == 0) {
        sc->bb = s; sc->rr = s; sc->tol2bb = tol * tol * s; sc->done = 0; sc->iters = 0;
        if (!isfinite(s)) atomicOr(&sc->status, GLM_ST_NONFINITE);      // a right-hand side that is not finite: no iteration will run
    }
}

// edge-ordered W_e -> the slots of both ends (the hooks that are handed blocks instead of vertices)
template <class M>
__global__ void glm_pack_kernel(int E, const double* __restrict__ W, const int* __restrict__ slot_of, double* __restrict__ S) {
    constexpr int N = M::N, NN = N * N;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= NN * E) return;
    const int e = idx / NN, q = idx - NN * e, a = q / N, c = q - N * a;
    const double v = W[idx];
    double* Pi = S + NN * (size_t)slot_of[2 * e]; double* Pj = S + NN * (size_t)slot_of[2 * e + 1];
    Pi[a * N + c] = v;
    Pj[c * N + a] = v;
}

// ---- the product -----------------------------------------------------------------------------------------------------------------
template <class M>
__device__ __forceinline__ double glm_slot_term(const double* __restrict__ S, const int* __restrict__ nbr, const double* __restrict__ x,
                                                int k, int row) {
    constexpr int N = M::N;
    const int u = nbr[k];
    return u >= 0 ? M::row_dot(S + N * N * (size_t)k + N * row, x + N * (size_t)u) : 0.0;
}
// row `row` of (H_vv + lambda I) x_v + sum over the slots [lo, hi) of v of S[k] x_nbr[k]
template <class M>
__device__ __forceinline__ double glm_vertex_row(int v, int row, const int* __restrict__ nbr, const double* __restrict__ S,
                                                 const double* __restrict__ Hd, double lambda, const double* __restrict__ x, int lo,
                                                 int hi) {
    constexpr int N = M::N;
    double y = M::row_dot(Hd + N * N * (size_t)v + N * row, x + N * (size_t)v) + lambda * x[N * (size_t)v + row];
    int k = lo;
    for (; k + 4 <= hi; k += 4) {
        const double t0 = glm_slot_term<M>(S, nbr, x, k, row), t1 = glm_slot_term<M>(S, nbr, x, k + 1, row),
                     t2 = glm_slot_term<M>(S, nbr, x, k + 2, row), t3 = glm_slot_term<M>(S, nbr, x, k + 3, row);
        y += t0; y += t1; y += t2; y += t3;
    }
    for (; k < hi; k++) y += glm_slot_term<M>(S, nbr, x, k, row);
    return y;
}
// a hub: the wave's VPW lane groups take the slots lo + g, lo + g + VPW, ...; the VPW partial rows meet in LDS and are added
// in group order behind the diagonal term (all 64 lanes of the wave call this together; lanes past VPW groups add nothing)
template <class M>
__device__ __forceinline__ double glm_hub_row(int v, int g, int row, const int* __restrict__ nbr, const double* __restrict__ S,
                                              const double* __restrict__ Hd, double lambda, const double* __restrict__ x, int lo,
                                              int hi, volatile double* sh /*[64] of this wave*/) {
    constexpr int N = M::N, VPW = glm_dims<M>::VPW;
    double part = 0.0;
    if (g < VPW)
        for (int k = lo + g; k < hi; k += VPW) part += glm_slot_term<M>(S, nbr, x, k, row);
    sh[threadIdx.x & 63] = part;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    double y = M::row_dot(Hd + N * N * (size_t)v + N * row, x + N * (size_t)v) + lambda * x[N * (size_t)v + row];
    for (int q = 0; q < VPW; q++) y += sh[q * N + row];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    return y;
}

// MODE 0: y = A x.  MODE 1 (CG): q = A p and part[block] = the block's share of p.q; nothing once sc->done is set, which the
// kernel itself sets (block 0) when the residual of the iteration before met the tolerance.
template <class M, int MODE>
__global__ __launch_bounds__(GLM_THREADS) void glm_hmul_kernel(int V, int main_blocks, const int* __restrict__ ptr,
                                                               const int* __restrict__ nbr, const uint8_t* __restrict__ fixed,
                                                               const int* __restrict__ hubs, const double* __restrict__ S,
                                                               const double* __restrict__ Hd, double lambda,
                                                               const double* __restrict__ x, double* __restrict__ y,
                                                               double* __restrict__ part, glm_scal* sc) {
    constexpr int N = M::N, VPW = glm_dims<M>::VPW, VPB = glm_dims<M>::VPB;
    __shared__ double sh[GLM_THREADS];
    __shared__ double shw[GLM_THREADS / 64];
    if (MODE == 1) {
        if (sc->done) return;
        if (!(sc->rr > sc->tol2bb)) {                  // converged (or not a number): this launch and all later ones are no-ops
            if (blockIdx.x == 0 && threadIdx.x == 0) sc->done = 1;
            return;
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane / N, row = lane - N * g;
    double dot = 0.0;
    if ((int)blockIdx.x < main_blocks) {
        for (int base = blockIdx.x * VPB; base < V; base += main_blocks * VPB) {
            const int v = base + wave * VPW + g;
            if (g >= VPW || v >= V) continue;
            const int lo = ptr[v], hi = ptr[v + 1];
            if (hi - lo > GLM_HUB_DEG) continue;       // a hub block writes it
            double r = 0.0;
            if (!fixed[v]) r = glm_vertex_row<M>(v, row, nbr, S, Hd, lambda, x, lo, hi);
            y[N * (size_t)v + row] = r;
            if (MODE == 1) dot += r * x[N * (size_t)v + row];
        }
    } else {
        const int n_hub = sc->n_hub, waves = (gridDim.x - main_blocks) * (GLM_THREADS / 64);
        for (int h = (blockIdx.x - main_blocks) * (GLM_THREADS / 64) + wave; h < n_hub; h += waves) {
            const int v = hubs[h];
            const double r = fixed[v] ? 0.0 : glm_hub_row<M>(v, g, row, nbr, S, Hd, lambda, x, ptr[v], ptr[v + 1], sh + 64 * wave);
            if (g == 0) {
                y[N * (size_t)v + row] = r;
                if (MODE == 1) dot += r * x[N * (size_t)v + row];
            }
        }
    }
    if (MODE == 1) {
        const double s = glm_block_sum(dot, shw);
        if (threadIdx.x == 0) part[blockIdx.x] = s;
    }
}

// ---- CG vector kernels (the product's N-lane mapping, `nblocks` blocks with a grid stride) ---------------------------------------
// Minv_v = (H_vv + lambda I)^-1, one lane per vertex
template <class M>
__global__ __launch_bounds__(64) void glm_precond_kernel(int V, const double* __restrict__ Hd, const uint8_t* __restrict__ fixed,
                                                         double lambda, double* __restrict__ Minv, glm_scal* sc) {
    constexpr int N = M::N, NN = N * N;
    const int v = blockIdx.x * 64 + threadIdx.x;
    if (v >= V) return;
    double A[NN], Inv[NN];
#pragma unroll
    for (int q = 0; q < NN; q++) A[q] = Hd[NN * (size_t)v + q] + ((q % (N + 1) == 0) ? lambda : 0.0);
    if (!ldlt_inverse<N>(A, Inv) && !fixed[v]) atomicOr(&sc->status, GLM_ST_PRECOND);
#pragma unroll
    for (int q = 0; q < NN; q++) Minv[NN * (size_t)v + q] = Inv[q];
}
// x = 0, r = -b (0 on fixed vertices), z = Minv r, p = z; partials of r.z (parity 0) and of b.b
template <class M>
__global__ __launch_bounds__(GLM_THREADS) void glm_cg_init_kernel(int V, int nblocks, const uint8_t* __restrict__ fixed,
                                                                  const double* __restrict__ b, const double* __restrict__ Minv,
                                                                  double* __restrict__ x, double* __restrict__ r, double* __restrict__ z,
                                                                  double* __restrict__ p, double* __restrict__ part_rz,
                                                                  double* __restrict__ part_rr) {
    constexpr int N = M::N, VPW = glm_dims<M>::VPW, VPB = glm_dims<M>::VPB;
    __shared__ double shw[GLM_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane / N, row = lane - N * g;
    double rz = 0.0, rr = 0.0;
    for (int base = blockIdx.x * VPB; base < V; base += nblocks * VPB) {
        const int v = base + wave * VPW + g;
        if (g >= VPW || v >= V) continue;
        const bool fx = fixed[v];
        double rv[N];
#pragma unroll
        for (int c = 0; c < N; c++) rv[c] = fx ? 0.0 : -b[N * (size_t)v + c];
        const double zr = fx ? 0.0 : M::minv_dot(Minv + N * N * (size_t)v + N * row, rv);
        const size_t o = N * (size_t)v + row;
        x[o] = 0.0; r[o] = rv[row]; z[o] = zr; p[o] = zr;
        rz += rv[row] * zr;
        rr += rv[row] * rv[row];
    }
    const double s0 = glm_block_sum(rz, shw), s1 = glm_block_sum(rr, shw);
    if (threadIdx.x == 0) { part_rz[blockIdx.x] = s0; part_rr[blockIdx.x] = s1; }
}
// alpha = r.z / p.q; x += alpha p; r -= alpha q (into r_out: the N lanes of a vertex all read r_v); z = Minv r; partials of the
// new r.z and r.r.  A p.q that is not positive ends the solve with the status bit (every block decides alike from the same sums).
// M::DONE_ONCE_PER_BLOCK: the done flag is read by one thread and shared, because block 0 sets it on a breakdown inside this
// very launch, and waves of one block that saw different values would part ways before a block-wide sum.  Without it every
// thread reads the flag itself.
template <class M>
__global__ __launch_bounds__(GLM_THREADS) void glm_cg_update_kernel(int V, int nblocks, int hmul_blocks, const double* __restrict__ Minv,
                                                                    const double* __restrict__ p, const double* __restrict__ q,
                                                                    double* __restrict__ x, const double* __restrict__ r,
                                                                    double* __restrict__ r_out, double* __restrict__ z,
                                                                    const double* __restrict__ part_pq, const double* __restrict__ part_rz_old,
                                                                    double* __restrict__ part_rz_new, double* __restrict__ part_rr,
                                                                    glm_scal* sc) {
    constexpr int N = M::N, VPW = glm_dims<M>::VPW, VPB = glm_dims<M>::VPB;
    __shared__ double shw[GLM_THREADS / 64];
    if constexpr (M::DONE_ONCE_PER_BLOCK) {
        __shared__ int was_done;
        if (threadIdx.x == 0) was_done = sc->done;
        __syncthreads();
        if (was_done) return;
    } else {
        if (sc->done) return;
    }
    const double pq = glm_sum_partials(part_pq, hmul_blocks, shw), rz_old = glm_sum_partials(part_rz_old, nblocks, shw);
    if (!(pq > 0.0) || !isfinite(pq) || !isfinite(rz_old)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { atomicOr(&sc->status, GLM_ST_BREAKDOWN); sc->done = 1; }
        return;
    }
    const double alpha = rz_old / pq;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane / N, row = lane - N * g;
    double rz = 0.0, rr = 0.0;
    for (int base = blockIdx.x * VPB; base < V; base += nblocks * VPB) {
        const int v = base + wave * VPW + g;
        if (g >= VPW || v >= V) continue;
        double rv[N];
#pragma unroll
        for (int c = 0; c < N; c++) rv[c] = r[N * (size_t)v + c] - alpha * q[N * (size_t)v + c];
        const double zr = M::minv_dot(Minv + N * N * (size_t)v + N * row, rv);
        const size_t o = N * (size_t)v + row;
        x[o] = x[o] + alpha * p[o];
        r_out[o] = rv[row];
        z[o] = zr;
        rz += rv[row] * zr;
        rr += rv[row] * rv[row];
    }
    const double s0 = glm_block_sum(rz, shw), s1 = glm_block_sum(rr, shw);
    if (threadIdx.x == 0) { part_rz_new[blockIdx.x] = s0; part_rr[blockIdx.x] = s1; }
}
// beta = r.z new / r.z old; p = z + beta p; block 0 publishes r.r and the iteration count (the next product kernel turns
// r.r into the done flag)
template <class M>
__global__ __launch_bounds__(GLM_THREADS) void glm_cg_direction_kernel(int V, int nblocks, const double* __restrict__ z, double* __restrict__ p,
                                                                       const double* __restrict__ part_rz_old,
                                                                       const double* __restrict__ part_rz_new,
                                                                       const double* __restrict__ part_rr, glm_scal* sc) {
    __shared__ double shw[GLM_THREADS / 64];
    if (sc->done) return;
    const double rz_old = glm_sum_partials(part_rz_old, nblocks, shw), rz_new = glm_sum_partials(part_rz_new, nblocks, shw);
    const double rr = glm_sum_partials(part_rr, nblocks, shw);
    const double beta = rz_new / rz_old;
    for (int i = blockIdx.x * GLM_THREADS + threadIdx.x; i < M::N * V; i += nblocks * GLM_THREADS) p[i] = z[i] + beta * p[i];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        sc->rr = rr;
        sc->iters = sc->iters + 1;
        if (!isfinite(rr) || !isfinite(beta)) atomicOr(&sc->status, GLM_ST_NONFINITE);
    }
}
template <class M>
__global__ void glm_cg_close_kernel(glm_scal* sc) {    // behind the last queued iteration: the decision the next product would take
    if (!(sc->rr > sc->tol2bb)) sc->done = 1;
}

// candidates: the retraction of x_v at vertex v (fixed ones copied), partials of the gain ratio's denominator x.(lambda x - b)
template <class M>
__global__ __launch_bounds__(GLM_THREADS) void glm_candidate_kernel(int V, const double* __restrict__ states, const uint8_t* __restrict__ fixed,
                                                                    const double* __restrict__ x, const double* __restrict__ b, double lambda,
                                                                    double* __restrict__ out, double* __restrict__ part_scale) {
    constexpr int N = M::N, STATE = M::STATE;
    __shared__ double shw[GLM_THREADS / 64];
    const int v = blockIdx.x * GLM_THREADS + threadIdx.x;
    double sc = 0.0;
    if (v < V) {
        double T[STATE], Tn[STATE];
#pragma unroll
        for (int q = 0; q < STATE; q++) T[q] = states[STATE * (size_t)v + q];
        if (fixed[v]) {
#pragma unroll
            for (int q = 0; q < STATE; q++) out[STATE * (size_t)v + q] = T[q];
        } else {
            double dx[N];
#pragma unroll
            for (int q = 0; q < N; q++) { dx[q] = x[N * (size_t)v + q]; sc += dx[q] * (lambda * dx[q] - b[N * (size_t)v + q]); }
            M::apply_update(dx, T, Tn);
#pragma unroll
            for (int q = 0; q < STATE; q++) out[STATE * (size_t)v + q] = Tn[q];
        }
    }
    const double s = glm_block_sum(sc, shw);
    if (threadIdx.x == 0) part_scale[blockIdx.x] = s;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
static inline uint64_t glm_up(uint64_t b) { return (b + 255) & ~(uint64_t)255; }
template <class M>
static inline int glm_vec_blocks(int64_t V) {
    const int64_t n = (V + glm_dims<M>::VPB - 1) / glm_dims<M>::VPB;
    return (int)(n < 1 ? 1 : n > GLM_MAX_PART ? GLM_MAX_PART : n);
}
static inline int glm_edge_blocks(int64_t E) { return (int)((E + 63) / 64); }
static inline int glm_cand_blocks(int64_t V) { return (int)((V + GLM_THREADS - 1) / GLM_THREADS); }

struct glm_layout {
    uint64_t scal, nbr, slot_of, hubs, hub_off, S, Dg, Hd, b, Minv, x, r, r2, z, p, q, part_cost, part_a, part_b, part_c, part_d, states2, total;
};
template <class M>
static glm_layout glm_make_layout(int64_t V, int64_t E) {
    using D = glm_dims<M>;
    glm_layout L;
    uint64_t o = 0;
    const uint64_t v = (uint64_t)(V > 0 ? V : 1), e = (uint64_t)(E > 0 ? E : 1), vec = v * D::N * 8;
    auto take = [&](uint64_t bytes) { const uint64_t at = o; o += glm_up(bytes); return at; };
    L.scal = take(sizeof(glm_scal));
    L.nbr = take(2 * e * 4); L.slot_of = take(2 * e * 4); L.hubs = take(v * 4); L.hub_off = take((uint64_t)glm_cand_blocks((int64_t)v) * 4);
    L.S = take(2 * e * D::NN * 8); L.Dg = take(2 * e * D::DSLOT * 8);
    L.Hd = take(v * D::NN * 8); L.b = take(vec); L.Minv = take(v * D::NN * 8);
    L.x = take(vec); L.r = take(vec); L.r2 = take(vec); L.z = take(vec); L.p = take(vec); L.q = take(vec);
    const int eb = glm_edge_blocks((int64_t)e), cb = glm_cand_blocks((int64_t)v);
    L.part_cost = take((uint64_t)(eb > cb ? eb : cb) * 8);
    const uint64_t pb = (uint64_t)(GLM_MAX_PART + GLM_HUB_BLOCKS) * 8;
    L.part_a = take(pb); L.part_b = take(pb); L.part_c = take(pb); L.part_d = take(pb);
    L.states2 = take(2 * v * D::STATE * 8);
    L.total = o;
    return L;
}

template <class M>
static int glm_common_checks(const char* who, slam_ctx* ctx, int64_t V, int64_t E) {
    SLAM_REQUIRE(ctx, "%s: null ctx", who);
    SLAM_REQUIRE(V >= 0 && V <= M::MAX_VERTICES && E >= 0 && E <= M::MAX_EDGES, "%s: bad sizes (V=%lld, E=%lld; limits 2^24 and 2^25)", who,
                 (long long)V, (long long)E);
    SLAM_REQUIRE(E == 0 || V > 0, "%s: edges without vertices", who);
    return SLAM_OK;
}

// the body of slam_*_workspace
template <class M>
static int glm_workspace(const char* who, int64_t V, int64_t E, uint64_t* bytes) {
    SLAM_REQUIRE(bytes, "%s: null bytes", who);
    SLAM_REQUIRE(V >= 0 && V <= M::MAX_VERTICES && E >= 0 && E <= M::MAX_EDGES, "bad sizes (V=%lld, E=%lld)", (long long)V, (long long)E);
    *bytes = glm_make_layout<M>(V, E).total;
    return SLAM_OK;
}

// the body of slam_*_plan; plan[7] is the manifold's own
template <class M>
static int glm_plan(const char* who, int64_t V, int64_t E, int32_t* plan) {
    SLAM_REQUIRE(plan, "%s: null plan", who);
    SLAM_REQUIRE(V >= 0 && V <= M::MAX_VERTICES && E >= 0 && E <= M::MAX_EDGES, "bad sizes (V=%lld, E=%lld)", (long long)V, (long long)E);
    plan[0] = glm_vec_blocks<M>(V);      // blocks of the product's main path and of the CG vector kernels (= partial sums per dot)
    plan[1] = GLM_HUB_BLOCKS;            // extra blocks of the product kernel for the hub list
    plan[2] = glm_dims<M>::VPB;          // vertices per block and grid-stride step (N lanes each)
    plan[3] = GLM_HUB_DEG;               // a vertex with more slots than this takes the wave-per-vertex path
    plan[4] = glm_edge_blocks(E);        // blocks of the edge kernel (= partial sums of the cost)
    plan[5] = GLM_CG_CHECK;              // CG iterations queued between two reads of the done flag
    plan[6] = 3;                         // launches per CG iteration
    plan[7] = 0;
    return SLAM_OK;
}

template <class M>
struct glm_graph {                       // device views of one call
    int V, E;
    const int *edges, *ptr, *adj;
    const uint8_t* fixed;
    uint8_t* ws;
    glm_layout L;
    glm_scal* sc;
    int vb;                              // blocks of the vector kernels
    template <class T> T* at(uint64_t off) const { return (T*)(ws + off); }
};

template <class M>
static void glm_open(glm_graph<M>& G, int64_t V, int64_t E, const int32_t* d_edges, const int32_t* d_ptr, const int32_t* d_adj,
                     const uint8_t* d_fixed, void* ws) {
    G.V = (int)V; G.E = (int)E; G.edges = d_edges; G.ptr = d_ptr; G.adj = d_adj; G.fixed = d_fixed;
    G.L = glm_make_layout<M>(V, E);
    G.ws = (uint8_t*)ws;
    G.sc = G.template at<glm_scal>(G.L.scal);
    G.vb = glm_vec_blocks<M>(V);
}

// checks and tables; reads the status back (ONE synchronisation per call, before any kernel follows an index)
template <class M>
static int glm_setup(slam_ctx* ctx, glm_graph<M>& G, glm_scal* h_scal /*pinned*/, const char* who, int64_t n_fixed_claimed) {
    hipStream_t st = ctx->stream;
    int *nbr = G.template at<int>(G.L.nbr), *slot_of = G.template at<int>(G.L.slot_of), *hub_off = G.template at<int>(G.L.hub_off);
    SLAM_HIP(hipMemsetAsync(G.sc, 0, sizeof(glm_scal), st));
    if (G.E > 0) {
        SLAM_HIP(hipMemsetAsync(slot_of, 0xFF, (size_t)2 * G.E * 4, st));
        glm_check_edges_kernel<M><<<(G.E + 255) / 256, 256, 0, st>>>(G.V, G.E, G.edges, G.sc);
    }
    glm_setup_vertices_kernel<M><<<(G.V + 255) / 256, 256, 0, st>>>(G.V, G.E, G.edges, G.ptr, G.adj, G.fixed, nbr, slot_of, G.sc);
    {
        const int hb = glm_cand_blocks(G.V);
        glm_hub_count_kernel<M><<<hb, GLM_THREADS, 0, st>>>(G.V, G.ptr, hub_off);
        glm_hub_scan_kernel<M><<<1, GLM_THREADS, 0, st>>>(hb, hub_off, G.sc);
        glm_hub_fill_kernel<M><<<hb, GLM_THREADS, 0, st>>>(G.V, G.ptr, hub_off, G.template at<int>(G.L.hubs));
    }
    if (G.E > 0) glm_check_slots_kernel<M><<<(2 * G.E + 255) / 256, 256, 0, st>>>(G.E, G.adj, slot_of, G.sc);
    SLAM_HIP(hipGetLastError());
    SLAM_HIP(hipMemcpyAsync(h_scal, G.sc, sizeof(glm_scal), hipMemcpyDeviceToHost, st));
    SLAM_HIP(hipStreamSynchronize(st));
    if (h_scal->status & GLM_ST_INDEX)
        return slam_set_error(SLAM_ERR_INVALID, "%s: an edge index outside [0, V), a self-edge, or a vertex list that does not match the edges", who);
    if (n_fixed_claimed >= 0 && h_scal->n_fixed != n_fixed_claimed)
        return slam_set_error(SLAM_ERR_INVALID, "%s: n_fixed = %lld but the mask fixes %d vertices", who, (long long)n_fixed_claimed, h_scal->n_fixed);
    return SLAM_OK;
}

template <class M, class... X>
static int glm_linearize(slam_ctx* ctx, const glm_graph<M>& G, const double* states, const double* meas, const double* info, double huber,
                         double* Hd, double* b, double* W_out, double* d_cost, X... opts) {
    hipStream_t st = ctx->stream;
    constexpr int per = GLM_THREADS / glm_dims<M>::GATHER_LANES;          // vertices per block of the gather
    double *Dg = G.template at<double>(G.L.Dg), *part_cost = G.template at<double>(G.L.part_cost);
    SLAM_HIP(hipMemsetAsync(&G.sc->maxdiag_bits, 0, 8, st));
    if (G.E > 0)
        glm_edge_kernel<M, true, X...><<<glm_edge_blocks(G.E), 64, 0, st>>>(G.E, states, G.edges, meas, info, G.template at<int>(G.L.slot_of), huber, opts...,
                                                                     G.template at<double>(G.L.S), Dg, W_out, part_cost, G.sc);
    glm_gather_kernel<M><<<(G.V + per - 1) / per, GLM_THREADS, 0, st>>>(G.V, G.ptr, Dg, G.fixed, Hd, b, G.sc);
    glm_finish_kernel<M><<<1, GLM_THREADS, 0, st>>>(part_cost, glm_edge_blocks(G.E), d_cost);
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

// the edge-ordered blocks d_W of a caller into the slots
template <class M>
static void glm_pack(slam_ctx* ctx, const glm_graph<M>& G, const double* d_W) {
    if (G.E > 0)
        glm_pack_kernel<M><<<(unsigned)((glm_dims<M>::NN * (int64_t)G.E + 255) / 256), 256, 0, ctx->stream>>>(
            G.E, d_W, G.template at<int>(G.L.slot_of), G.template at<double>(G.L.S));
}

template <class M>
static int glm_hmul(slam_ctx* ctx, const glm_graph<M>& G, const double* Hd, double lambda, const double* x, double* y) {
    glm_hmul_kernel<M, 0><<<G.vb + GLM_HUB_BLOCKS, GLM_THREADS, 0, ctx->stream>>>(G.V, G.vb, G.ptr, G.template at<int>(G.L.nbr), G.fixed,
                                                                                 G.template at<int>(G.L.hubs), G.template at<double>(G.L.S), Hd,
                                                                                 lambda, x, y, nullptr, G.sc);
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

// (H + lambda I) x = -b: at most max_iter iterations of three launches each, the done flag read every GLM_CG_CHECK iterations
template <class M>
static int glm_pcg(slam_ctx* ctx, const glm_graph<M>& G, const double* Hd, const double* b, double lambda, double tol, int max_iter, double* x,
                   glm_scal* h_scal) {
    hipStream_t st = ctx->stream;
    auto dbl = [&](uint64_t off) { return G.template at<double>(off); };
    double *Minv = dbl(G.L.Minv), *z = dbl(G.L.z), *p = dbl(G.L.p), *q = dbl(G.L.q), *S = dbl(G.L.S);
    double* r[2] = {dbl(G.L.r), dbl(G.L.r2)};
    double *part_pq = dbl(G.L.part_a), *part_rr = dbl(G.L.part_b);
    double* part_rz[2] = {dbl(G.L.part_c), dbl(G.L.part_d)};
    const int *nbr = G.template at<int>(G.L.nbr), *hubs = G.template at<int>(G.L.hubs);
    const int hb = G.vb + GLM_HUB_BLOCKS;
    glm_precond_kernel<M><<<(G.V + 63) / 64, 64, 0, st>>>(G.V, Hd, G.fixed, lambda, Minv, G.sc);
    glm_cg_init_kernel<M><<<G.vb, GLM_THREADS, 0, st>>>(G.V, G.vb, G.fixed, b, Minv, x, r[0], z, p, part_rz[0], part_rr);
    glm_finish_bb_kernel<M><<<1, GLM_THREADS, 0, st>>>(part_rr, G.vb, tol, G.sc);
    SLAM_HIP(hipGetLastError());
    for (int n = 0; n < max_iter; n++) {
        const int a = n & 1, c = a ^ 1;
        glm_hmul_kernel<M, 1><<<hb, GLM_THREADS, 0, st>>>(G.V, G.vb, G.ptr, nbr, G.fixed, hubs, S, Hd, lambda, p, q, part_pq, G.sc);
        glm_cg_update_kernel<M><<<G.vb, GLM_THREADS, 0, st>>>(G.V, G.vb, hb, Minv, p, q, x, r[a], r[c], z, part_pq, part_rz[a], part_rz[c], part_rr,
                                                             G.sc);
        glm_cg_direction_kernel<M><<<G.vb, GLM_THREADS, 0, st>>>(G.V, G.vb, z, p, part_rz[a], part_rz[c], part_rr, G.sc);
        if ((n + 1) % GLM_CG_CHECK == 0 && n + 1 < max_iter) {
            glm_cg_close_kernel<M><<<1, 1, 0, st>>>(G.sc);
            SLAM_HIP(hipGetLastError());
            SLAM_HIP(hipMemcpyAsync(h_scal, G.sc, sizeof(glm_scal), hipMemcpyDeviceToHost, st));
            SLAM_HIP(hipStreamSynchronize(st));
            if (h_scal->done) break;
        }
    }
    glm_cg_close_kernel<M><<<1, 1, 0, st>>>(G.sc);
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

// workspace + a pinned block for the scalars, and the graph opened on them (call lock held)
template <class M>
static int glm_blocks(slam_ctx* ctx, glm_graph<M>& G, int64_t V, int64_t E, const int32_t* d_edges, const int32_t* d_ptr, const int32_t* d_adj,
                      const uint8_t* d_fixed, glm_scal** hs) {
    void *dev = nullptr, *host = nullptr, *ws = nullptr;
    if (int rc = slam_io_arena(ctx, 0, 256, &dev, &host)) return rc;
    if (int rc = slam_workspace(ctx, glm_make_layout<M>(V, E).total, &ws)) return rc;
    *hs = (glm_scal*)host;
    glm_open(G, V, E, d_edges, d_ptr, d_adj, d_fixed, ws);
    return SLAM_OK;
}

// ---- the bodies of the extern "C" calls, behind their argument checks -------------------------------------------------------------
template <class M, class... X>
static int glm_linearize_call(const char* who, slam_ctx* ctx, int64_t V, int64_t E, const double* d_states, const int32_t* d_edges,
                              const double* d_meas, const double* d_info, const int32_t* d_vtx_ptr, const int32_t* d_vtx_adj, double huber,
                              double* d_cost, double* d_grad, double* d_Hdiag, double* d_W, int32_t* h_status, X... opts) {
    SLAM_HIP(hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> lk(ctx->call_mu);
    *h_status = 0;
    if (V == 0) { SLAM_HIP(hipMemsetAsync(d_cost, 0, 8, ctx->stream)); return SLAM_OK; }
    glm_graph<M> G;
    glm_scal* hs = nullptr;
    if (int rc = glm_blocks(ctx, G, V, E, d_edges, d_vtx_ptr, d_vtx_adj, nullptr, &hs)) return rc;
    if (int rc = glm_setup(ctx, G, hs, who, -1)) return rc;
    if (int rc = glm_linearize(ctx, G, d_states, d_meas, d_info, huber, d_Hdiag, d_grad, d_W, d_cost, opts...)) return rc;
    SLAM_HIP(hipMemcpyAsync(hs, G.sc, sizeof(glm_scal), hipMemcpyDeviceToHost, ctx->stream));
    SLAM_HIP(hipStreamSynchronize(ctx->stream));
    *h_status = hs->status;
    return SLAM_OK;
}

template <class M>
static int glm_hmul_call(const char* who, slam_ctx* ctx, int64_t V, int64_t E, const int32_t* d_edges, const int32_t* d_vtx_ptr,
                         const int32_t* d_vtx_adj, const uint8_t* d_fixed, const double* d_Hdiag, const double* d_W, double lambda,
                         const double* d_x, double* d_y) {
    SLAM_HIP(hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> lk(ctx->call_mu);
    glm_graph<M> G;
    glm_scal* hs = nullptr;
    if (int rc = glm_blocks(ctx, G, V, E, d_edges, d_vtx_ptr, d_vtx_adj, d_fixed, &hs)) return rc;
    if (int rc = glm_setup(ctx, G, hs, who, -1)) return rc;
    glm_pack(ctx, G, d_W);
    return glm_hmul(ctx, G, d_Hdiag, lambda, d_x, d_y);
}

template <class M>
static int glm_pcg_call(const char* who, slam_ctx* ctx, int64_t V, int64_t E, const int32_t* d_edges, const int32_t* d_vtx_ptr,
                        const int32_t* d_vtx_adj, const uint8_t* d_fixed, const double* d_Hdiag, const double* d_W, const double* d_b,
                        double lambda, double tol, int max_iter, double* d_x, double* h_stats) {
    SLAM_HIP(hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> lk(ctx->call_mu);
    glm_graph<M> G;
    glm_scal* hs = nullptr;
    if (int rc = glm_blocks(ctx, G, V, E, d_edges, d_vtx_ptr, d_vtx_adj, d_fixed, &hs)) return rc;
    if (int rc = glm_setup(ctx, G, hs, who, -1)) return rc;
    glm_pack(ctx, G, d_W);
    if (int rc = glm_pcg(ctx, G, d_Hdiag, d_b, lambda, tol, max_iter, d_x, hs)) return rc;
    SLAM_HIP(hipMemcpyAsync(hs, G.sc, sizeof(glm_scal), hipMemcpyDeviceToHost, ctx->stream));
    SLAM_HIP(hipStreamSynchronize(ctx->stream));
    // converged = the tolerance was met by a finite residual; `done` is only the stop flag (breakdown and NaN set it too)
    h_stats[0] = hs->iters; h_stats[1] = (isfinite(hs->rr) && hs->rr <= hs->tol2bb) ? 1.0 : 0.0;
    h_stats[2] = hs->bb == 0.0 ? 0.0 : sqrt(hs->rr / hs->bb); h_stats[3] = hs->status;
    return SLAM_OK;
}

// the LM loop on a set-up graph (g2o's schedule, as pose_opt.hip restates it; call lock held).  hs: pinned.  d_states in -> d_out.
template <class M, class... X>
static int glm_optimize_locked(slam_ctx* ctx, glm_graph<M>& G, const double* d_states, const double* d_meas, const double* d_info, int iterations,
                               double huber, double tol, int max_iter, double* d_out, double* h_stats, glm_scal* hs, X... opts) {
    constexpr int STATE = M::STATE;
    hipStream_t st = ctx->stream;
    const int V = G.V;
    double* cur = G.template at<double>(G.L.states2);
    double* cand = cur + STATE * (size_t)V;
    double *Hd = G.template at<double>(G.L.Hd), *b = G.template at<double>(G.L.b), *x = G.template at<double>(G.L.x);
    double* part_cost = G.template at<double>(G.L.part_cost);
    const int bad_state = M::BAD_STATE;
    SLAM_HIP(hipMemcpyAsync(cur, d_states, (size_t)V * STATE * 8, hipMemcpyDeviceToDevice, st));
    if (int rc = glm_linearize(ctx, G, cur, d_meas, d_info, huber, Hd, b, nullptr, &G.sc->cost, opts...)) return rc;
    SLAM_HIP(hipMemcpyAsync(hs, G.sc, sizeof(glm_scal), hipMemcpyDeviceToHost, st));
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
            if (int rc = glm_pcg(ctx, G, Hd, b, lambda, tol, max_iter, x, hs)) return rc;
            glm_candidate_kernel<M><<<glm_cand_blocks(V), GLM_THREADS, 0, st>>>(V, cur, G.fixed, x, b, lambda, cand, part_cost);
            glm_finish_kernel<M><<<1, GLM_THREADS, 0, st>>>(part_cost, glm_cand_blocks(V), &G.sc->scale);
            glm_edge_kernel<M, false, X...><<<glm_edge_blocks(G.E), 64, 0, st>>>(G.E, cand, G.edges, d_meas, d_info, nullptr, huber, opts..., nullptr, nullptr,
                                                                          nullptr, part_cost, G.sc);
            glm_finish_kernel<M><<<1, GLM_THREADS, 0, st>>>(part_cost, glm_edge_blocks(G.E), &G.sc->cost);
            SLAM_HIP(hipGetLastError());
            SLAM_HIP(hipMemcpyAsync(hs, G.sc, sizeof(glm_scal), hipMemcpyDeviceToHost, st));
            SLAM_HIP(hipStreamSynchronize(st));
            trials++;
            cg_total += hs->iters;
            status |= hs->status & (GLM_ST_PRECOND | GLM_ST_BREAKDOWN);
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
                if (int rc = glm_linearize(ctx, G, cur, d_meas, d_info, huber, Hd, b, nullptr, &G.sc->cost, opts...)) return rc;
                break;
            }
            lambda *= ni;
            ni *= 2.0;
            if (!(lambda - lambda == 0.0)) stop = true;
        }
        if (!taken) break;                                                    // ten trials turned down: g2o gives up
    }
    SLAM_HIP(hipMemcpyAsync(d_out, cur, (size_t)V * STATE * 8, hipMemcpyDeviceToDevice, st));
    SLAM_HIP(hipStreamSynchronize(st));
    h_stats[0] = F0; h_stats[1] = F; h_stats[2] = accepted; h_stats[3] = trials; h_stats[4] = (double)cg_total; h_stats[5] = lambda;
    h_stats[6] = status; h_stats[7] = 0.0;
    return SLAM_OK;
}

template <class M>
static int glm_optimize_checks(const char* who, slam_ctx* ctx, int64_t V, int64_t E, int64_t n_fixed, int iterations, double huber, double tol,
                               int max_iter) {
    if (int rc = glm_common_checks<M>(who, ctx, V, E)) return rc;
    SLAM_REQUIRE(iterations >= 0 && iterations <= 10000, "%s: iterations out of range [0, 10000]", who);
    SLAM_REQUIRE(huber >= 0.0 && tol > 0.0 && tol < 1.0 && max_iter >= 1 && max_iter <= (1 << 20),
                 "%s: huber_delta >= 0, 0 < pcg_tol < 1, pcg_max_iter in [1, 2^20]", who);
    SLAM_REQUIRE(V == 0 || (n_fixed >= 1 && n_fixed <= V), "%s: a graph needs at least one fixed vertex (n_fixed=%lld)", who, (long long)n_fixed);
    return SLAM_OK;
}

// slam_*_optimize_f64 from its checks on: V > 0, the device pointers are there
template <class M, class... X>
static int glm_optimize_call(const char* who, slam_ctx* ctx, int64_t V, int64_t E, const double* d_states, const int32_t* d_edges,
                             const double* d_meas, const double* d_info, const uint8_t* d_fixed, int64_t n_fixed, const int32_t* d_vtx_ptr,
                             const int32_t* d_vtx_adj, int iterations, double huber, double tol, int max_iter, double* d_out,
                             double* h_stats, X... opts) {
    SLAM_HIP(hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> lk(ctx->call_mu);
    if (E == 0) {                                        // nothing pulls on any vertex
        SLAM_HIP(hipMemcpyAsync(d_out, d_states, (size_t)V * M::STATE * 8, hipMemcpyDeviceToDevice, ctx->stream));
        return SLAM_OK;
    }
    glm_graph<M> G;
    glm_scal* hs = nullptr;
    if (int rc = glm_blocks(ctx, G, V, E, d_edges, d_vtx_ptr, d_vtx_adj, d_fixed, &hs)) return rc;
    if (int rc = glm_setup(ctx, G, hs, who, n_fixed)) return rc;
    return glm_optimize_locked(ctx, G, d_states, d_meas, d_info, iterations, huber, tol, max_iter, d_out, h_stats, hs, opts...);
}

// slam_*_optimize_host_f64 from its checks on (V > 0, the host pointers are there): one upload (the vertex lists are built here
// by a stable counting sort: the slots of a vertex in ascending edge order), the LM loop, one download.  Edges with an index
// outside [0, V) get no slot; the device check then refuses the call (SLAM_ERR_INVALID) and h_out is not written.
template <class M, class... X>
static int glm_optimize_host_call(const char* who, slam_ctx* ctx, int64_t V, int64_t E, const double* h_states, const int32_t* h_edges,
                                  const double* h_meas, const double* h_info, const uint8_t* h_fixed, int64_t n_fixed, int iterations, double huber,
                                  double tol, int max_iter, double* h_out, double* h_stats, X... opts) {
    constexpr uint64_t SB = M::STATE * 8, IB = glm_dims<M>::NN * 8;        // bytes of a vertex or measurement, of an information matrix
    if (E == 0) { memmove(h_out, h_states, (size_t)V * SB); return SLAM_OK; }
    std::lock_guard<std::mutex> lk(ctx->call_mu);
    SLAM_HIP(hipSetDevice(ctx->device));
    const uint64_t o_scal = 0, o_states = 256, o_edges = o_states + glm_up((uint64_t)V * SB), o_meas = o_edges + glm_up((uint64_t)E * 8);
    const uint64_t o_info = o_meas + glm_up((uint64_t)E * SB), o_fixed = o_info + glm_up((uint64_t)E * IB), o_ptr = o_fixed + glm_up((uint64_t)V);
    const uint64_t o_adj = o_ptr + glm_up((uint64_t)(V + 1) * 4), o_out = o_adj + glm_up((uint64_t)E * 8), total = o_out + glm_up((uint64_t)V * SB);
    void *ws = nullptr, *dev = nullptr, *host = nullptr;
    if (int rc = slam_io_arena(ctx, total, total, &dev, &host)) return rc;
    if (int rc = slam_workspace(ctx, glm_make_layout<M>(V, E).total, &ws)) return rc;
    uint8_t *hb = (uint8_t*)host, *db = (uint8_t*)dev;
    memcpy(hb + o_states, h_states, (size_t)V * SB);
    memcpy(hb + o_edges, h_edges, (size_t)E * 8);
    memcpy(hb + o_meas, h_meas, (size_t)E * SB);
    memcpy(hb + o_info, h_info, (size_t)E * IB);
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
    ctx->io_h2d_bytes += o_out - o_states;
    ctx->io_d2h_bytes += (uint64_t)V * SB;
    SLAM_HIP(hipMemcpyAsync(db + o_states, hb + o_states, o_out - o_states, hipMemcpyHostToDevice, ctx->stream));
    glm_graph<M> G;
    glm_open(G, V, E, (const int32_t*)(db + o_edges), (const int32_t*)(db + o_ptr), (const int32_t*)(db + o_adj), db + o_fixed, ws);
    if (int rc = glm_setup(ctx, G, (glm_scal*)(hb + o_scal), who, n_fixed)) return rc;
    if (int rc = glm_optimize_locked(ctx, G, (const double*)(db + o_states), (const double*)(db + o_meas), (const double*)(db + o_info), iterations,
                                     huber, tol, max_iter, (double*)(db + o_out), h_stats, (glm_scal*)(hb + o_scal), opts...))
        return rc;
    SLAM_HIP(hipMemcpyAsync(hb + o_out, db + o_out, (size_t)V * SB, hipMemcpyDeviceToHost, ctx->stream));
    SLAM_HIP(hipStreamSynchronize(ctx->stream));
    memcpy(h_out, hb + o_out, (size_t)V * SB);
    return SLAM_OK;
}
