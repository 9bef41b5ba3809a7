// bf_mx32_scan.inc - the text of the 32x32x64 search kernel, included by bf_mx32.hip once per feed with MX32_KERNEL (the
// kernel's name) and MX32_IMAGE_FEED (0 or 1) defined: two kernels of their own, so that neither's code depends on the other.
// The search, in its two feeds.  IMG = false: t is the compact train rows, every block expands the stages it scans (the file
// header).  IMG = true: t is the prepared image of the train set (bf_mx_image_kernel below) - the bytes of every LDS stage as
// they stand in `tile`, stage after stage - and a stage is four 16-byte copies per thread straight into LDS: no expand, no
// ds_write, no staged words in registers.  Everything else - geometry, trip order, folds, update path, tickets, exchanges,
// epilogue - is one text, so the two give the same tables bit for bit.
// grid = (query blocks, workers).  Block (x, y) works for query block (x + y) mod grid.x, as bf_top2_mx_kernel.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void MX32_KERNEL(
    const uint4* __restrict__ q, int N, const uint4* __restrict__ t, const int* __restrict__ tbl, bf_state st, int train_base,
    int2* __restrict__ out_idx, int2* __restrict__ out_dist, uint4* __restrict__ keep, int nchunks, bf_select sel) {
    constexpr bool IMG = MX32_IMAGE_FEED;
    __shared__ uint4 tile[2][SLAM_MX_STAGE * 8];
    __shared__ u32 s_ticket, s_last;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int hk = lane >> 5, col = lane & 31;
#ifdef SLAM_MX_PROBE
    unsigned long long pacc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, plast = __builtin_readcyclecounter();
#endif
    const int bx = ((int)blockIdx.x + (int)blockIdx.y) % (int)gridDim.x;
    // the lane's query in the epilogue and in the bound exchange: worked out afresh at each of them (the empty asm hides that the
    // value repeats), or it and the addresses built on it hold registers through the scan
    auto lane_query = [&]() -> int {
        int v = tid;
        asm volatile("" : "+v"(v));
        return bx * 256 + v;
    };

    // the wave's 64 queries as B operands: tile tt, K-quarter kq = word 2 kq + (lane >> 5) of query 64 wave + 32 tt + (lane & 31)
    uint4 qb[2][4];
    const u32* qw = (const u32*)q;
#pragma unroll
    for (int tt = 0; tt < 2; tt++) {
        int qi = bx * 256 + wave * 64 + tt * 32 + col;
        qi = qi < N ? qi : N - 1;                                // tail columns compute a duplicate and are never stored
#pragma unroll
        for (int kq = 0; kq < 4; kq++) qb[tt][kq] = mx_expand(qw[(size_t)qi * 8 + kq * 2 + hk]);
    }
    if (const int qbase = lane_query(); keep && blockIdx.y == 0 && qbase < N) {   // the caller wants the query rows left in device memory
        keep[2 * (size_t)qbase] = q[2 * (size_t)qbase];
        keep[2 * (size_t)qbase + 1] = q[2 * (size_t)qbase + 1];
    }

    // per tile: the lane's own top-2 over its rows, the exclusive threshold distance x and the pattern the fold compares against
    u32 b1[2], b2[2], xs[2];
    int thr[2];
    auto set_threshold = [&](int tt, u32 x) {
        xs[tt] = x;
        thr[tt] = x > 129u ? (int)0x80000000u : __float_as_int((float)(258 - 2 * (int)x));
    };
#pragma unroll
    for (int tt = 0; tt < 2; tt++) {
        b1[tt] = b2[tt] = SLAM_KEY_NONE;
        set_threshold(tt, SLAM_KEY_NONE >> SLAM_KEY_IDX_BITS);   // 511: everything passes
    }
    // the top-2 of one tile's query over the rows of the two lanes that hold it
    auto unite_tile = [&](int tt, u32& u1, u32& u2) {
        u1 = b1[tt];
        u2 = b2[tt];
        const u32 c1 = (u32)__shfl_xor((int)u1, 32, 64), c2 = (u32)__shfl_xor((int)u2, 32, 64);
        mx_unite(u1, u2, c1, c2);
    };
    // Exchange with the other workers of this query block through bound[], at the start of the chunk (or stage) that begins at
    // row c0; lane l speaks for query 64 wave + l, which tile (l >> 5) holds.  As bf_top2_mx_kernel's.
    u32 gkey = SLAM_BOUND_IDLE, pend[1] = {0u};
    auto exchange = [&](int c0) {
        u32 u1[2], u2[2];
#pragma unroll
        for (int tt = 0; tt < 2; tt++) unite_tile(tt, u1[tt], u2[tt]);
        if (const int qbase = lane_query(); qbase < N) {
            const u32 own = hk ? u2[1] : u2[0];
            asm volatile("" ::"v"(pend[0]));
            const u32 g = __hip_atomic_load(&st.bound[qbase], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (own < g && own < SLAM_MX_BOUND_LIMIT) pend[0] = atomicMin(&st.bound[qbase], own);
            gkey = g;
        }
#pragma unroll
        for (int tt = 0; tt < 2; tt++) {
            // the united pair comes from rows below c0: ties against it lose.  Another worker's key: mx_bound_x tests its row
            const u32 g = (u32)__shfl((int)gkey, tt * 32 + col, 64);
            set_threshold(tt, min(xs[tt], min(mx_bound_x(g, c0), u2[tt] >> SLAM_KEY_IDX_BITS)));
        }
    };

    // staging: thread tid carries half (tid & 1) of row (tid >> 1) of a stage, i.e. the source words 4 sh + j, j = 0 .. 3: word
    // j is the operand piece of K-quarter 2 sh + (j >> 1), lane (row & 31) + 32 (j & 1), in the row's group of 32
    const int srow = tid >> 1, sh = tid & 1;
    auto load_stage = [&](int s, int c1) -> uint4 {
        const uint4* ts = t + 2 * (size_t)s;
        if (s + SLAM_MX_STAGE <= c1) return ts[(u32)tid];
        return s + srow < c1 ? ts[(u32)tid] : make_uint4(0, 0, 0, 0);
    };
    const u32 fill = 0x22222222u;
    uint4* const dst0 = tile[0] + (srow >> 5) * 256 + sh * 128 + (srow & 31);
    auto store_word = [&](uint4* dst, int j, u32 v) { dst[(j >> 1) * 64 + (j & 1) * 32] = mx_expand_op(v, fill); };
    auto store_stage = [&](int b, uint4 v) {
        uint4* dst = dst0 + b * (SLAM_MX_STAGE * 8);
        store_word(dst, 0, v.x);
        store_word(dst, 1, v.y);
        store_word(dst, 2, v.z);
        store_word(dst, 3, v.w);
    };
    // IMG: the stage that begins at row s (a multiple of the stage: the planner's chunk boundaries) is 16 KiB of the image,
    // copied as it stands into buffer b.  Piece j of wave w is bytes 4096 j + 1024 w .. + 1024 of the stage, there and here.
    auto copy_stage = [&](int b, int s) {
        const u32 lds = (u32)(size_t)(__attribute__((address_space(3))) void*)(tile[b] + __builtin_amdgcn_readfirstlane(wave) * 64);
        mx32_copy_stage(t + (size_t)s * 8, (u32)tid * 16u, lds);
    };

    u32* const cursor = st.cursor + (size_t)(4 * bx) * SLAM_CURSOR_STRIDE;
    if (tid == 0) s_ticket = __hip_atomic_fetch_add(cursor, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    int ci = __builtin_amdgcn_readfirstlane((int)s_ticket);
    int scanned = 0;                                             // wave-uniform: the rows this block has scanned since launch
    MX_STAMP(0);
    while (ci < nchunks) {
        const int c0 = tbl[ci], c1 = tbl[ci + 1];
        if constexpr (IMG) {
            copy_stage(0, c0);
            exchange(c0);
            mx32_copies_done();
        } else {
            const uint4 first = load_stage(c0, c1);
            exchange(c0);
            store_stage(0, first);
        }
        __syncthreads();
        MX_STAMP(1);
        int buf = 0;
        for (int s0 = c0; s0 < c1; s0 += SLAM_MX_STAGE) {
            const int s1 = s0 + SLAM_MX_STAGE;
            const bool more = s1 < c1;
            // the next ticket is drawn while the chunk's last stage is scanned; read behind the stage's barrier
            if (!more && tid == 0) s_ticket = __hip_atomic_fetch_add(cursor, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            MX_STAMP(7);
            const uint4* tp = tile[buf];
            // fold the 16 results of tile tt of group g and, where some lane of the tile passes, take the update path.  A tile's
            // fold and update path touch that tile's accumulators and state only, so where the folds of the two tiles stand
            // relative to each other and to the other tile's MFMAs does not matter to the result
            auto fold_tile = [&](int tt, int g, const mx_v16f& acc, auto rag) {
                // the fold is a tree of eight maxima whose first level is the maxima of the gate groups (mx32_gate_index,
                // bf_mx32.hip): one maximum of two accumulators, seven of three
                auto a = [&](int i) { return __float_as_int(acc[i]); };
                int gm[MX32_GATES];
                gm[0] = max(a(0), a(1));
#pragma unroll
                for (int j = 1; j < MX32_GATES; j++) gm[j] = max(max(a(3 * j - 1), a(3 * j)), a(3 * j + 1));
                gm[0] = max(max(gm[0], a(14)), a(15));
                const int m = max(max(max(max(gm[1], gm[2]), gm[3]), gm[4]), gm[0]);
                if (__builtin_expect(__ballot(m >= thr[tt]) == 0ull, 1)) return;
                MX_STAMP(2);
                // the group's first row is taken from the scalar side here: as a per-lane value it would be carried through
                // every group that does not fire.  g is the group that is FOLDED, whichever group's MFMAs stand around the fold
                int row0 = s0 + g * MX32_GROUP;
                asm("" : "+s"(row0));
                const u32 rowk = (u32)row0 + (u32)(4 * hk);
                // key = (128 - D / 2) << 23 | row: base + (-D << 22), exact modulo 2^32 (D is an even integer)
                const u32 base = (128u << SLAM_KEY_IDX_BITS) + rowk;
                // a row of the lane: its key, exact whatever the row's distance, into the lane's sorted pair
                auto enter = [&](int i) {
                    const int off = 8 * (i >> 2) + (i & 3);
                    u32 key = base + (u32)off + ((u32)(int)(-acc[i]) << (SLAM_KEY_IDX_BITS - 1));
                    if constexpr (decltype(rag)::value)   // the rows past the end of a short stage never enter
                        key = (int)rowk + off < c1 ? key : SLAM_KEY_NONE;
                    b2[tt] = umed3(b1[tt], b2[tt], key);
                    b1[tt] = min(b1[tt], key);
                };
                // the five group gates: the compares back to back, each into an SGPR pair of its own (the threshold moves only
                // behind the rows), then scalar tests alone, so that no branch waits on the compare in front of it
                unsigned long long gate[MX32_GATES];
#pragma unroll
                for (int j = 0; j < MX32_GATES; j++) gate[j] = __ballot(gm[j] >= thr[tt]);
                asm volatile("" ::"s"(gate[0]), "s"(gate[1]), "s"(gate[2]), "s"(gate[3]), "s"(gate[4]));
#pragma unroll
                for (int j = 0; j < MX32_GATES; j++) {
                    if (gate[j] == 0ull) continue;
                    // an open group: all of its rows enter, no inner branch
#pragma unroll
                    for (int r = 0; r < mx32_gate_rows(j); r++) enter(mx32_gate_index(j, r));
                }
                set_threshold(tt, min(xs[tt], b2[tt] >> SLAM_KEY_IDX_BITS));
                MX_STAMP(3);
            };
            const mx_v16f zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            auto group = [&](int g, auto rag) {
                mx_v16f acc[2];
#pragma unroll
                for (int kq = 0; kq < 4; kq++) {
                    const uint4 a = tp[g * 256 + kq * 64 + lane];
#pragma unroll
                    for (int tt = 0; tt < 2; tt++) acc[tt] = mx32_dot(a, qb[tt][kq], kq ? acc[tt] : zero);
                }
#pragma unroll
                for (int tt = 0; tt < 2; tt++) fold_tile(tt, g, acc[tt], rag);
            };
            // A whole stage: one trip of four groups.  Group k issues, in this order,
            //     t0k0 t0k1 t0k2 t0k3 [fold of tile 1, group k - 1] t1k0 t1k1 t1k2 t1k3 [fold of tile 0, group k]
            // (t<tile>k<K-quarter>), so a fold - and the update path where the tile fires - runs while the last of four MFMAs of
            // the OTHER tile is in the pipe, and between the last MFMA that wrote its accumulators and its first read stand those
            // four and the other fold: more than the 11 wait states the compiler owes there, so it pads nothing (measured against
            // the alternating orders in tools/ubench/mx_issue.hip; DESIGN.md 3c).  Each tile still sees its own MFMAs, fold and
            // update path in the same order, before its next C = 0 MFMA; tile 1 of the last group folds bare, behind tile 0's
            // fold, so the stage end sees both tiles folded.
            // The A operand of K-quarter kq of group k + 1 is read once tile 1's MFMA of quarter kq of group k has issued, into the
            // registers it frees (three MFMAs before its first use); the last group reads nothing ahead, so no read
            // leaves the stage's own buffer.  With `shadow`, groups 1 to 3 also expand and store the thread's four source words
            // of the NEXT stage (into buffer buf ^ 1, free since the barrier that opened this stage) between their MFMAs.
            auto trip = [&](auto shadow) {
                constexpr bool SH = decltype(shadow)::value;
                const uint4* ap = tp + lane;
                uint4* const dst = dst0 + (buf ^ 1) * (SLAM_MX_STAGE * 8);
                // the thread's 16 bytes of the next stage, one load at the trip's start: its latency runs behind group 0.  Were
                // the next stage not whole, the rows past the chunk end would read its last row instead (what such a row holds
                // never matters, the scan tests its index); this keeps the load inside the train set whatever the table
                u32 nx[4] = {0, 0, 0, 0};
                if constexpr (SH && IMG) {
                    copy_stage(buf ^ 1, s1);                     // in flight behind the whole trip; waited for in front of the barrier
                } else if (SH) {
                    const uint4 x = (t + 2 * (size_t)s1)[2 * min(srow, c1 - 1 - s1) + sh];
                    nx[0] = x.x; nx[1] = x.y; nx[2] = x.z; nx[3] = x.w;
                }
                uint4 a[4];
#pragma unroll
                for (int kq = 0; kq < 4; kq++) a[kq] = ap[kq * 64];
                mx_v16f acc[2];
                auto dot = [&](int tt, int kq) {
                    __builtin_amdgcn_sched_barrier(0);
                    acc[tt] = mx32_dot(a[kq], qb[tt][kq], kq ? acc[tt] : zero);
                    __builtin_amdgcn_sched_barrier(0);
                };
#pragma unroll
                for (int k = 0; k < MX32_GROUPS; k++) {
                    auto ahead = [&](int kq) {                   // both MFMAs of quarter kq of this group have issued (tile 1's last)
                        if (k + 1 < MX32_GROUPS) a[kq] = ap[(k + 1) * 256 + kq * 64];
                        __builtin_amdgcn_sched_barrier(0);
                    };
                    dot(0, 0);
                    dot(0, 1);
                    dot(0, 2);
                    dot(0, 3);
                    if (k) fold_tile(1, k - 1, acc[1], std::false_type{});
                    dot(1, 0);
                    ahead(0);
                    dot(1, 1);
                    ahead(1);
                    // the next stage's words: word 0 in group 1, word 1 in group 2, words 2 and 3 in group 3
                    if (SH && !IMG && k >= 1) store_word(dst, k - 1, nx[k - 1]);
                    dot(1, 2);
                    ahead(2);
                    if (SH && !IMG && k == 3) store_word(dst, 3, nx[3]);
                    dot(1, 3);
                    ahead(3);
                    fold_tile(0, k, acc[0], std::false_type{});
                }
                __builtin_amdgcn_sched_barrier(0);
                fold_tile(1, MX32_GROUPS - 1, acc[1], std::false_type{});
            };
            if (more) {                                          // then this stage is whole
                trip(std::true_type{});
            } else if (s1 == c1) {
                trip(std::false_type{});
            } else {                                             // a short stage: the last of the train set
                const int ng = __builtin_amdgcn_readfirstlane((c1 - s0 + MX32_GROUP - 1) / MX32_GROUP);
                for (int g = 0; g < ng; g++) group(g, std::true_type{});
            }
            MX_STAMP(2);
            // No union of a query's two lanes here: a stage ends with each lane's threshold at its own 2nd-best.  The united
            // threshold spared 2 % of the fired tiles and cost two LDS round trips in front of the barrier in 41 % of the
            // tile-stages (tools/mx_fire_model.py; DESIGN.md 3c "The stage tail"); the exchanges and the epilogue still unite.
            // an early exchange (SLAM_MX_EARLY): per wave, no barrier; every row still to come is at or above s1.  Not after a
            // chunk's last stage: the chunk-start exchange follows anyway
            scanned += min(s1, c1) - s0;
            if (more && scanned < 32 * SLAM_MX_STAGE && (SLAM_MX_EARLY >> (scanned / SLAM_MX_STAGE) & 1u)) exchange(s1);
            MX_STAMP(4);
            if constexpr (IMG) mx32_copies_done();                    // each wave its own copies; the barrier makes them the block's
            __syncthreads();
            MX_STAMP(5);
            buf ^= 1;
        }
        ci = __builtin_amdgcn_readfirstlane((int)s_ticket);
    }

    u32 u1[2], u2[2];
#pragma unroll
    for (int tt = 0; tt < 2; tt++) unite_tile(tt, u1[tt], u2[tt]);
    const u32 f1[1] = {hk ? u1[1] : u1[0]}, f2[1] = {hk ? u2[1] : u2[0]};
    // the epilogue's skip test takes a DISTANCE that bounds the final 2nd-best one, or the idle pattern when there is none
    const u32 gk[1] = {gkey < SLAM_MX_BOUND_LIMIT ? gkey >> SLAM_KEY_IDX_BITS : SLAM_BOUND_IDLE};
    bf_top2_epilogue<1, true>(st, bx, tid, lane, lane_query(), false, false, f1, f2, gk, pend, N, (int)gridDim.y, train_base, out_idx,
                              out_dist, sel, s_last);
#ifdef SLAM_MX_PROBE
    MX_STAMP(6);
    if (g_mx32_probe && lane == 0) {
        unsigned long long* o = g_mx32_probe + ((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 4 + wave) * 8;
        for (int i = 0; i < 8; i++) o[i] = pacc[i];
    }
#endif
}
