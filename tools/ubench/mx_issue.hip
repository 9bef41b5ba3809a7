// Micro-benchmark: what the FP4 MFMA of the matrix-core top-2 search (bf_mx.hip) costs the SIMD's vector issue, in MEASURED
// shader cycles (s_memtime, as cycles.hip).
//
// The body is the shipped group of 16 train rows: 8 x v_mfma_scale_f32_16x16x128_f8f6f4 cbsz:4 blgp:4 with VGPR accumulators -
// four that start from the threshold quads, four that accumulate in place - on operands held in registers (random FP4 +-1
// nibbles 0x2 / 0xA).  Beside every MFMA go k = 0 .. 4 independent v_max3_i32 fillers (no register of an MFMA in them):
//   (i)   interleaved: k fillers after each MFMA, in the wave's own stream;
//   (ii)  bunched:     the 8 MFMAs, then 8 k fillers;
//   (iii) cross-wave:  the waves in even wave slots of a SIMD run bare groups, the waves in odd slots run ONLY fillers for a fixed
//                      1.5 M cycles of the shader clock - less than the MFMA waves need, so every filler counted was issued
//                      beside them - in bursts of 8 k with (4 - k) s_nop 15 between bursts (k = 4: back to back).
// at 1, 2 and 4 blocks per CU ((iii): 2 and 4).  Every wave records where it ran (HW_ID, XCC_ID), so a row is computed per
// SIMD from the waves that really shared it: only SIMDs that held exactly the asked number of waves count, and the share of
// their span in which all of them ran is printed beside (waves of equal priority are served by age).  Per row: the SIMD's cycles per MFMA (its span / its MFMAs, median over SIMDs), an MFMA wave's
// own cycles per group, and for (iii) the fillers a filler wave issued per MFMA time of its SIMD.
// It answers: how long an FP4 MFMA holds the vector issue, how many plain instructions per MFMA are free in-wave and
// cross-wave, and what the floor of the shipped mix (8 MFMAs + 25 plain instructions per group) is.
// build: hipcc --offload-arch=gfx950 -O3 mx_issue.hip -o mx_issue
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>
#include <map>
#include <vector>
#define CK(x) do{hipError_t e=(x); if(e!=hipSuccess){printf("%s: %s\n",#x,hipGetErrorString(e)); return 1;}}while(0)

// registers, as in the shipped listing: B operands v[2:33] (tile tt, K-half h at 2 + 8 tt + 4 h), threshold quads v[34:49], A
// operands v[50:53] / v[54:57], accumulators v[62:77], the scales in v96; the fillers use v[80:87] only
#define CLOB "v2","v3","v4","v5","v6","v7","v8","v9","v10","v11","v12","v13","v14","v15","v16","v17","v18","v19","v20","v21","v22","v23", \
             "v24","v25","v26","v27","v28","v29","v30","v31","v32","v33","v34","v35","v36","v37","v38","v39","v40","v41","v42","v43","v44","v45", \
             "v46","v47","v48","v49","v50","v51","v52","v53","v54","v55","v56","v57","v62","v63","v64","v65","v66","v67","v68","v69","v70","v71", \
             "v72","v73","v74","v75","v76","v77","v80","v81","v82","v83","v84","v85","v86","v87","v96"
#define MF(d, a, b, c) "v_mfma_scale_f32_16x16x128_f8f6f4 v[" d "], v[" a "], v[" b "], v[" c "], v96, v96 op_sel_hi:[0,0,0] cbsz:4 blgp:4\n"
#define F1 "v_max3_i32 v80, v84, v85, v86\n"
#define F2 F1 "v_max3_i32 v81, v85, v86, v87\n"
#define F3 F2 "v_max3_i32 v82, v86, v87, v84\n"
#define F4 F3 "v_max3_i32 v83, v87, v84, v85\n"
#define F0 ""
#define M0 MF("62:65", "50:53", "2:5", "34:37")
#define M1 MF("66:69", "50:53", "10:13", "38:41")
#define M2 MF("70:73", "50:53", "18:21", "42:45")
#define M3 MF("74:77", "50:53", "26:29", "46:49")
#define M4 MF("62:65", "54:57", "6:9", "62:65")
#define M5 MF("66:69", "54:57", "14:17", "66:69")
#define M6 MF("70:73", "54:57", "22:25", "70:73")
#define M7 MF("74:77", "54:57", "30:33", "74:77")
#define INTER(F) M0 F M1 F M2 F M3 F M4 F M5 F M6 F M7 F
#define BUNCH(F) M0 M1 M2 M3 M4 M5 M6 M7 F F F F F F F F
#define NOP16 "s_nop 15\n"
#define X4(a) a a a a
#define FILL_CYCLES 1500000ull

struct stamp { unsigned long long c0, r0, c1, r1; unsigned role, hwid, xcc, count; };

// PLACE 0 interleaved | 1 bunched | 2 cross-wave; K fillers per MFMA
template <int PLACE, int K>
__global__ __launch_bounds__(256) void k(uint32_t* out, stamp* st, int iters) {
    uint32_t seed = threadIdx.x * 2654435761u + blockIdx.x * 40503u + 1u;
    // FP4 +-1 operands: every nibble 0x2 or 0xA
#define RND(r) "v_mul_lo_u32 %0, %0, %1\n v_and_b32 " r ", 0x88888888, %0\n v_or_b32 " r ", 0x22222222, " r "\n"
    asm volatile(RND("v2") RND("v3") RND("v4") RND("v5") RND("v6") RND("v7") RND("v8") RND("v9") RND("v10") RND("v11") RND("v12") RND("v13")
                 RND("v14") RND("v15") RND("v16") RND("v17") RND("v18") RND("v19") RND("v20") RND("v21") RND("v22") RND("v23") RND("v24")
                 RND("v25") RND("v26") RND("v27") RND("v28") RND("v29") RND("v30") RND("v31") RND("v32") RND("v33") RND("v50") RND("v51")
                 RND("v52") RND("v53") RND("v54") RND("v55") RND("v56") RND("v57")
                 : "+v"(seed) : "v"(1664525u) : CLOB);
    // thresholds as in the kernel (2 x - 258 for some x), fillers' inputs, scale 2^0 on both sides
    asm volatile("v_mov_b32 v34, 0xc2a00000\n v_mov_b32 v35, v34\n v_mov_b32 v36, v34\n v_mov_b32 v37, v34\n v_mov_b32 v38, v34\n v_mov_b32 v39, v34\n"
                 "v_mov_b32 v40, v34\n v_mov_b32 v41, v34\n v_mov_b32 v42, v34\n v_mov_b32 v43, v34\n v_mov_b32 v44, v34\n v_mov_b32 v45, v34\n"
                 "v_mov_b32 v46, v34\n v_mov_b32 v47, v34\n v_mov_b32 v48, v34\n v_mov_b32 v49, v34\n"
                 "v_mov_b32 v84, %0\n v_mov_b32 v85, %0\n v_mov_b32 v86, %0\n v_mov_b32 v87, %0\n v_mov_b32 v80, 0\n v_mov_b32 v81, 0\n v_mov_b32 v82, 0\n"
                 "v_mov_b32 v83, 0\n v_mov_b32 v96, 0x7f7f7f7f\n"
                 M0 M1 M2 M3 "s_nop 15\n" ::"v"(seed) : CLOB);
    unsigned hwid, xcc, count = 0;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)\n s_getreg_b32 %1, hwreg(HW_REG_XCC_ID)" : "=s"(hwid), "=s"(xcc));
    const bool filler_wave = PLACE == 2 && (hwid & 1);             // HW_ID[3:0] = wave slot of the SIMD
    unsigned long long c0, r0, c1, r1;
    asm volatile("s_memtime %0\n s_memrealtime %1\n s_waitcnt lgkmcnt(0)" : "=s"(c0), "=s"(r0)::"memory");
    if (!filler_wave) {
        for (int it = 0; it < iters; it += 4) {
            if (PLACE == 1) {
                if (K == 0) asm volatile(X4(BUNCH(F0)) ::: CLOB);
                if (K == 1) asm volatile(X4(BUNCH(F1)) ::: CLOB);
                if (K == 2) asm volatile(X4(BUNCH(F2)) ::: CLOB);
                if (K == 3) asm volatile(X4(BUNCH(F3)) ::: CLOB);
                if (K == 4) asm volatile(X4(BUNCH(F4)) ::: CLOB);
            } else if (PLACE == 0) {
                if (K == 0) asm volatile(X4(INTER(F0)) ::: CLOB);
                if (K == 1) asm volatile(X4(INTER(F1)) ::: CLOB);
                if (K == 2) asm volatile(X4(INTER(F2)) ::: CLOB);
                if (K == 3) asm volatile(X4(INTER(F3)) ::: CLOB);
                if (K == 4) asm volatile(X4(INTER(F4)) ::: CLOB);
            } else {
                asm volatile(X4(INTER(F0)) ::: CLOB);
            }
        }
    } else {
        // bursts of 8 K fillers for FILL_CYCLES of the shader clock (looked at once per four bursts); count = bursts issued
        for (;;) {
            if (K == 0) asm volatile(X4(NOP16 NOP16 NOP16 NOP16) ::: CLOB);
            if (K == 1) asm volatile(X4(F1 F1 F1 F1 F1 F1 F1 F1 NOP16 NOP16 NOP16) ::: CLOB);
            if (K == 2) asm volatile(X4(F2 F2 F2 F2 F2 F2 F2 F2 NOP16 NOP16) ::: CLOB);
            if (K == 3) asm volatile(X4(F3 F3 F3 F3 F3 F3 F3 F3 NOP16) ::: CLOB);
            if (K == 4) asm volatile(X4(F4 F4 F4 F4 F4 F4 F4 F4) ::: CLOB);
            count += 4;
            unsigned long long now;
            asm volatile("s_memtime %0\n s_waitcnt lgkmcnt(0)" : "=s"(now)::"memory");
            if (now - c0 > FILL_CYCLES) break;
        }
    }
    asm volatile("s_memtime %0\n s_memrealtime %1\n s_waitcnt lgkmcnt(0)" : "=s"(c1), "=s"(r1)::"memory");
    uint32_t s;
    asm volatile("s_nop 15\n s_nop 15\n v_add_u32 %0, v62, v66\n v_add_u32 %0, %0, v70\n v_add_u32 %0, %0, v74\n v_add_u32 %0, %0, v80\n v_add_u32 %0, %0, v81\n"
                 "v_add_u32 %0, %0, v82\n v_add_u32 %0, %0, v83" : "=v"(s)::CLOB);
    out[blockIdx.x * 256 + threadIdx.x] = s;
    if ((threadIdx.x & 63) == 0) {
        stamp v = {c0, r0, c1, r1, filler_wave ? 1u : 0u, hwid, xcc, count};
        st[blockIdx.x * 4 + (threadIdx.x >> 6)] = v;
    }
}

static double median(std::vector<double>& v) { std::sort(v.begin(), v.end()); return v.empty() ? 0.0 : v[v.size() / 2]; }

static const int MAXW = 4, NCU = 256;

template <int PLACE, int K> int run(int waves, uint32_t* out, stamp* d_st, double spin_s) {
    const int iters = 20000, blocks = NCU * waves;
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    CK(hipEventRecord(e0));
    float spun = 0;
    while (spun < spin_s * 1e3f) {                      // spin-up: back-to-back launches of the same body
        for (int i = 0; i < 8; i++) k<PLACE, K><<<blocks, 256>>>(out, d_st, iters);
        CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
        CK(hipEventElapsedTime(&spun, e0, e1));
    }
    k<PLACE, K><<<blocks, 256>>>(out, d_st, iters);
    CK(hipDeviceSynchronize());
    std::vector<stamp> st(blocks * 4);
    CK(hipMemcpy(st.data(), d_st, st.size() * sizeof(stamp), hipMemcpyDeviceToHost));
    // group the waves by the SIMD they ran on: XCC, then HW_ID's SE / SH / CU (bits 15:8) and SIMD (bits 5:4)
    std::map<unsigned, std::vector<const stamp*>> simd;
    std::vector<double> clk, grp, per_mfma, fill_per_mfma, together;
    for (auto& s : st) {
        clk.push_back((double)(s.c1 - s.c0) / (double)(s.r1 - s.r0) * 100.0);                 // MHz
        if (!s.role) grp.push_back((double)(s.c1 - s.c0) / (double)iters);                    // this wave's own cycles per group
        simd[(s.xcc & 15u) << 16 | (s.hwid & 0xff00u) | (s.hwid >> 4 & 3u)].push_back(&s);
    }
    size_t used = 0;
    for (auto& kv : simd) {
        auto& w = kv.second;
        if ((int)w.size() != waves) continue;
        // s_memtime is one counter per XCC: the stamps of a SIMD's waves compare.  The MFMA waves set the span.
        unsigned long long lo = ~0ull, hi = 0, lo_max = 0, hi_min = ~0ull;
        double mfmas = 0, fillers = 0;
        for (auto* s : w) {
            if (s->role) { fillers += (double)s->count * 8 * K; continue; }
            lo = std::min(lo, s->c0); hi = std::max(hi, s->c1);
            lo_max = std::max(lo_max, s->c0); hi_min = std::min(hi_min, s->c1);
            mfmas += (double)iters * 8;
        }
        if (mfmas == 0) continue;
        together.push_back(hi_min > lo_max ? (double)(hi_min - lo_max) / (double)(hi - lo) : 0.0);
        bool beside = true;                              // (iii): the filler waves ran inside the MFMA waves' common span
        for (auto* s : w)
            if (s->role && (s->c0 + FILL_CYCLES / 5 < lo_max || s->c1 > hi_min)) beside = false;
        if (!beside) continue;
        used++;
        per_mfma.push_back((double)(hi - lo) / mfmas);
        if (fillers > 0) fill_per_mfma.push_back(fillers / ((double)FILL_CYCLES / ((double)(hi - lo) / mfmas)));
    }
    const double mclk = median(clk);
    const char* place[] = {"interleaved", "bunched", "cross-wave"};
    std::sort(grp.begin(), grp.end());
    printf("%-11s k %d  blocks/CU %d: %4zu of %4zu SIMDs held %d waves, all running for %3.0f %% of the span | %6.2f cycles/MFMA/SIMD | an MFMA wave's own "
           "group: p10 %6.1f median %6.1f p90 %6.1f cycles",
           place[PLACE], K, waves, used, simd.size(), waves, 100 * median(together), median(per_mfma), grp[grp.size() / 10], median(grp),
           grp[grp.size() * 9 / 10]);
    if (PLACE == 2 && K) printf(" | fillers issued beside the MFMAs: %5.2f per MFMA time", median(fill_per_mfma));
    printf(" | clock %4.0f MHz\n", mclk);
    fflush(stdout);
    return 0;
}

template <int PLACE> int sweep(int waves, uint32_t* out, stamp* d_st, double spin_s) {
    if (run<PLACE, 0>(waves, out, d_st, spin_s)) return 1;
    if (run<PLACE, 1>(waves, out, d_st, spin_s)) return 1;
    if (run<PLACE, 2>(waves, out, d_st, spin_s)) return 1;
    if (run<PLACE, 3>(waves, out, d_st, spin_s)) return 1;
    return run<PLACE, 4>(waves, out, d_st, spin_s);
}

int main(int argc, char** argv) {
    const double spin_s = argc > 1 ? atof(argv[1]) : 0.5;
    uint32_t* out; CK(hipMalloc(&out, (size_t)NCU * MAXW * 256 * 4));
    stamp* d_st; CK(hipMalloc(&d_st, (size_t)NCU * MAXW * 4 * sizeof(stamp)));
    for (int w : {1, 2, 4}) {
        if (sweep<0>(w, out, d_st, spin_s)) return 1;
        if (sweep<1>(w, out, d_st, spin_s)) return 1;
        if (w > 1 && sweep<2>(w, out, d_st, spin_s)) return 1;
    }
    return 0;
}
