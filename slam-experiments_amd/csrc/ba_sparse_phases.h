// ba_sparse_phases.h - the one copy of the four phases of the sparse bundle adjustment that read a measurement (obs, point,
// pose, cost) and of the lookup of one observation, as templates over an edge model: ba_sparse.hip runs them on bas_mono_edge
// (ba_linearise: two rows, weight w, every edge live), ba_stereo.hip on bast_edge (stereo_edge.h: three rows, weight w s, an
// edge live iff s > 0, informations checked and counted).  Lists, thread mapping, NaN poisoning and ba_block_sum are the same
// for both, so every sum has one order.
//
// This header carries NO floating-point contraction pragma of its own (the idiom of ba_common.h); both files include it BEHIND
// their `#pragma clang fp contract(off)`, after ba_common.h and ba_sparse_common.h.
//
// An edge model E supplies
//   E::ROWS, E::tab, E::cam, E::robust        residual rows; the observation table {obs_pose, obs_point, .., K, L, O}; the
//                                             camera; the Huber width(s)
//   m.residual(t, o, T, X, k, l, cam, delta)  residuals, weight and cost of observation o at pose k of T and point l of X
//   E::info_ok(t, o)                          false for an information that is none (counted by the obs phase, taken as 0)
//   m.live()                                  false for an edge that is switched off: it adds nothing anywhere
//   m.jacobians(P, cam)                       the Jacobians of a live edge, where residual() did not make them already
//   m.weight(), m.rho()                       the factor of every block term; the robust cost
//   m.e(), m.jp(), m.jq()                     ROWS residuals, ROWS x 6 pose Jacobian, ROWS x 3 point Jacobian (row-major)
#pragma once

// sum over the rows of a[i * sa] * b[i * sb], grouped from the left: a0 b0 + a1 b1 for two rows, (a0 b0 + a1 b1) + a2 b2 for three
template <int ROWS>
__device__ __forceinline__ double bas_row_dot(const double* a, const int sa, const double* b, const int sb) {
    double s = a[0] * b[0];
#pragma unroll
    for (int i = 1; i < ROWS; i++) s = s + a[i * sa] * b[i * sb];
    return s;
}

// observation o of an index table at (T, X); false (nothing dereferenced) when o or one of its indices is outside.  k and l
// come back for the Jacobians.
template <class E>
__device__ __forceinline__ bool bas_at(const typename E::tab& t, const double* __restrict__ T, const double* __restrict__ X, const int o,
                                       const typename E::cam& cam, const typename E::robust& delta, E& m, int& k, int& l) {
    if ((unsigned)o >= (unsigned)t.O) return false;
    k = t.obs_pose[o]; l = t.obs_point[o];
    if ((unsigned)k >= (unsigned)t.K || (unsigned)l >= (unsigned)t.L) return false;
    m.residual(t, o, T, X, k, l, cam, delta);
    return true;
}

// a thread per observation: Hpl_o = weight Jp^T Jq; the two indices and the information are checked here and counted
template <class E>
__global__ __launch_bounds__(BA_THREADS) void bas_obs_kernel(const typename E::tab t, const double* __restrict__ T, const double* __restrict__ X,
                                                              typename E::cam cam, typename E::robust delta,
                                                              unsigned int* __restrict__ index_errors, double* __restrict__ Hpl /*[O,18]*/) {
    const int o = (int)(blockIdx.x * BA_THREADS + threadIdx.x);
    if (o >= t.O) return;
    E m;
    int k, l;
    double* h = Hpl + (size_t)o * 18;
    if (!bas_at(t, T, X, o, cam, delta, m, k, l)) {          // reported, never dereferenced; its block poisons what reads it
        atomicAdd(index_errors, 1u);
#pragma unroll
        for (int i = 0; i < 18; i++) h[i] = __builtin_nan("");
        return;
    }
    if (!E::info_ok(t, o)) atomicAdd(index_errors, 1u);      // an information that is none: counted, taken as 0
    if (!m.live()) {                                          // switched off: adds nothing anywhere
#pragma unroll
        for (int i = 0; i < 18; i++) h[i] = 0.0;
        return;
    }
    m.jacobians(T + (size_t)k * 12, cam);
    const double w = m.weight();
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int c = 0; c < 3; c++) h[a * 3 + c] = w * bas_row_dot<E::ROWS>(m.jp() + a, 6, m.jq() + c, 3);
}

// a thread per point: Hll (6), bl (3) over its list pt_obs, in list order
template <class E>
__global__ __launch_bounds__(BA_THREADS) void bas_point_kernel(const typename E::tab t, const double* __restrict__ T, const double* __restrict__ X,
                                                                const int* __restrict__ pt_ptr, const int* __restrict__ pt_obs,
                                                                typename E::cam cam, typename E::robust delta,
                                                                unsigned int* __restrict__ index_errors, double* __restrict__ Hll /*[L,6]*/,
                                                                double* __restrict__ bl /*[L,3]*/) {
    const int l = (int)(blockIdx.x * BA_THREADS + threadIdx.x);
    if (l >= t.L) return;
    double h[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};
    int a0 = pt_ptr[l], a1 = pt_ptr[l + 1];
    if (a0 < 0 || a1 < a0 || a1 > t.O) { atomicAdd(index_errors, 1u); a1 = a0 = 0; }
    for (int i = a0; i < a1; i++) {
        E m;
        int k, l2;
        if (!bas_at(t, T, X, pt_obs[i], cam, delta, m, k, l2)) { h[0] = __builtin_nan(""); continue; }
        if (!m.live()) continue;
        m.jacobians(T + (size_t)k * 12, cam);
        const double w = m.weight();
        int n = 0;
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int c = a; c < 3; c++) h[n++] += w * bas_row_dot<E::ROWS>(m.jq() + a, 3, m.jq() + c, 3);
#pragma unroll
        for (int a = 0; a < 3; a++) b[a] += w * bas_row_dot<E::ROWS>(m.jq() + a, 3, m.e(), 1);
    }
#pragma unroll
    for (int i = 0; i < 6; i++) Hll[(size_t)l * 6 + i] = h[i];
#pragma unroll
    for (int i = 0; i < 3; i++) bl[(size_t)l * 3 + i] = b[i];
}

// a workgroup per pose: Hpp (21), bp (6), cost: thread t takes entries t, t + 256, .. of ps_obs, then ba_block_sum
template <class E>
__global__ __launch_bounds__(BA_THREADS) void bas_pose_kernel(const typename E::tab t, const double* __restrict__ T, const double* __restrict__ X,
                                                               const int* __restrict__ ps_ptr, const int* __restrict__ ps_obs,
                                                               typename E::cam cam, typename E::robust delta,
                                                               unsigned int* __restrict__ index_errors, double* __restrict__ Hpp /*[K,21]*/,
                                                               double* __restrict__ bp /*[K,6]*/, double* __restrict__ cost /*[K]*/) {
    __shared__ double sw[BAS_WAVES][28];
    __shared__ double out[28];
    const int k = (int)blockIdx.x;
    double acc[28];
#pragma unroll
    for (int i = 0; i < 28; i++) acc[i] = 0.0;
    int a0, a1;
    // the first phase to read ps_ptr reports a corrupt slice, once (bas_cost_kernel and bas_diag_kernel take it as empty too)
    if (!bas_pose_range(ps_ptr, k, t.O, a0, a1) && threadIdx.x == 0) atomicAdd(index_errors, 1u);
    for (int i = a0 + (int)threadIdx.x; i < a1; i += BA_THREADS) {
        E m;
        int k2, l;
        if (!bas_at(t, T, X, ps_obs[i], cam, delta, m, k2, l)) { acc[27] = __builtin_nan(""); continue; }
        if (!m.live()) continue;
        m.jacobians(T + (size_t)k2 * 12, cam);
        const double w = m.weight();
        int n = 0;
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int c = a; c < 6; c++) acc[n++] += w * bas_row_dot<E::ROWS>(m.jp() + a, 6, m.jp() + c, 6);
#pragma unroll
        for (int a = 0; a < 6; a++) acc[21 + a] += w * bas_row_dot<E::ROWS>(m.jp() + a, 6, m.e(), 1);
        acc[27] += m.rho();
    }
    ba_block_sum<28>(acc, sw, out);
    if (threadIdx.x < 21) Hpp[(size_t)k * 21 + threadIdx.x] = out[threadIdx.x];
    else if (threadIdx.x < 27) bp[(size_t)k * 6 + threadIdx.x - 21] = out[threadIdx.x];
    else if (threadIdx.x == 27) cost[k] = out[27];
}

// a workgroup per pose: the robust cost at a state, summed as bas_pose_kernel sums it
template <class E>
__global__ __launch_bounds__(BA_THREADS) void bas_cost_kernel(const typename E::tab t, const double* __restrict__ T, const double* __restrict__ X,
                                                               const int* __restrict__ ps_ptr, const int* __restrict__ ps_obs,
                                                               typename E::cam cam, typename E::robust delta, double* __restrict__ cost /*[K]*/) {
    __shared__ double sw[BAS_WAVES][1];
    __shared__ double out[1];
    const int k = (int)blockIdx.x;
    double acc[1] = {0.0};
    int a0, a1;
    bas_pose_range(ps_ptr, k, t.O, a0, a1);
    for (int i = a0 + (int)threadIdx.x; i < a1; i += BA_THREADS) {
        E m;
        int k2, l;
        if (!bas_at(t, T, X, ps_obs[i], cam, delta, m, k2, l)) { acc[0] = __builtin_nan(""); continue; }
        if (!m.live()) continue;
        acc[0] += m.rho();
    }
    ba_block_sum<1>(acc, sw, out);
    if (threadIdx.x == 0) cost[k] = out[0];
}
